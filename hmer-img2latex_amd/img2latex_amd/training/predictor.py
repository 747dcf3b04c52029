"""Predictor with the reference's surface (img2latex/training/predictor.py:20-394) on the HIP path.

Checkpoint compatibility: ``from_checkpoint`` reads the dict the reference's
``Trainer.save_checkpoint`` writes (trainer.py:209-224: ``model_state_dict``, ``config``,
``tokenizer_config{token_to_id, special_tokens, max_sequence_length}``) and rebuilds model and
token table exactly as predictor.py:80-129 does.  The greedy loop of ``predict_batch``
(predictor.py:283-358) runs as ONE persistent kernel launch (I2L_STOP_STICKY + argmax of softmax).

``predict`` / ``predict_batch`` take what the reference's take -- a path, a PIL image, a numpy array or a tensor
-- through ``_prepare_image`` (predictor.py:396-462, incl. its hard-coded 64x800 target and its range-dependent
normalisation of tensors); the pixels are resampled on the device (img2latex_amd.data).  ``predict_batch_ids`` /
``evaluate_batch`` are this package's batch entry points for tensors ALREADY shaped for the model (the benchmark
drivers: SURVEY 8b "feed tensors straight to the encoder").
"""
from __future__ import annotations

import os
import warnings
import weakref
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import _lib
from ..model import Seq2SeqModel

DEFAULT_SPECIAL_TOKENS = {"PAD": "<PAD>", "START": "<START>", "END": "<END>", "UNK": "<UNK>"}   # tokenizer.py:36-41


class TokenTable:
    """LaTeXTokenizer's host surface (tokenizer.py:24-321): id maps, special ids, encode() / decode(), save() / load() in
    the reference's file layout, and fit() / fit_on_formulas_file(), which count and order the tokens on the device
    (training/vocab.py, i2l_vocab_fit).  The batch calls are TokenizeTable / DetokenizeTable."""

    def __init__(self, token_to_id: Optional[Dict[str, int]] = None, special_tokens: Optional[Dict[str, str]] = None,
                 max_sequence_length: int = 141):
        self.special_tokens = dict(special_tokens or DEFAULT_SPECIAL_TOKENS)
        if token_to_id is None:
            token_to_id = {tok: i for i, tok in enumerate(self.special_tokens.values())}
        self.max_sequence_length = max_sequence_length
        self._set_vocabulary(token_to_id)

    def _set_vocabulary(self, token_to_id: Dict[str, int]) -> None:
        self.token_to_id = dict(token_to_id)
        self.id_to_token = {i: t for t, i in self.token_to_id.items()}
        self.vocab_size = len(self.token_to_id)
        self.pad_token_id = self.token_to_id[self.special_tokens["PAD"]]
        self.start_token_id = self.token_to_id[self.special_tokens["START"]]
        self.end_token_id = self.token_to_id[self.special_tokens["END"]]
        self.unk_token_id = self.token_to_id[self.special_tokens["UNK"]]

    def decode(self, ids: Sequence[int], skip_special_tokens: bool = True) -> str:
        special = {self.token_to_id[t] for t in self.special_tokens.values()} if skip_special_tokens else set()
        return " ".join(self.id_to_token.get(int(i), self.special_tokens["UNK"]) for i in ids if int(i) not in special)

    def config(self) -> Dict:
        return {"token_to_id": self.token_to_id, "special_tokens": self.special_tokens,
                "max_sequence_length": self.max_sequence_length}

    def encode(self, text: str, add_special_tokens: bool = False) -> List[int]:
        """tokenizer.py:143-164 on the host: ``str.split()``, unknown -> UNK, START / END around the text when asked."""
        if add_special_tokens:
            text = f"{self.special_tokens['START']} {text} {self.special_tokens['END']}"
        return [self.token_to_id.get(tok, self.unk_token_id) for tok in text.split()]

    def _refit(self, fitted) -> None:
        """Take a fitted vocabulary (training/vocab.py): the maps and the four special ids anew, as ``_init_special_tokens``
        + ``fit`` leave them, this object's cached device tables dropped (they hold the old vocabulary), and the
        reference's warning about rows longer than ``max_sequence_length`` (tokenizer.py:106-113)."""
        from . import constraint as _constraint, tokenizer as _tokenizer
        self._set_vocabulary(fitted.token_to_id)
        for cache in (_TABLES, _tokenizer._TABLES, _constraint._TABLES, _constraint._ARGUMENT_TABLES):
            cache.pop(self, None)
        if self.max_sequence_length is not None and fitted.longest_row > self.max_sequence_length:
            warnings.warn(f"Found sequences of length {fitted.longest_row}, which is longer than max_sequence_length "
                          f"({self.max_sequence_length}). Consider increasing max_sequence_length.")

    def fit(self, texts: Sequence[str], device=None):
        """LaTeXTokenizer.fit (tokenizer.py:80-117) with the counting and ordering on the device: the vocabulary is reset
        to the special tokens, then every other token of ``texts`` (``str.split()``) gets the next id by descending
        count, ties in first-seen order.  Returns the ``VocabFit`` (counts, total, longest row).  An empty ``texts``
        raises ValueError, as the reference's ``max()`` does."""
        from .vocab import fit_vocabulary
        fitted = fit_vocabulary(texts, self.special_tokens, device)
        self._refit(fitted)
        return fitted

    def fit_on_formulas_file(self, file_path: str, device=None):
        """tokenizer.py:119-141: one formula per line (UTF-8, universal newlines), each wrapped in START / END -- which
        changes no id and adds 2 to every row's length.  The file's bytes go to the device as they are."""
        from .vocab import fit_formulas_file
        fitted = fit_formulas_file(file_path, self.special_tokens, device)
        self._refit(fitted)
        return fitted

    def save(self, file_path: str) -> None:
        """tokenizer.py:257-275: ``torch.save`` of ``config()``'s three keys; LaTeXTokenizer.load reads it."""
        if os.path.dirname(file_path):
            os.makedirs(os.path.dirname(file_path), exist_ok=True)
        torch.save(self.config(), file_path)

    @classmethod
    def load(cls, file_path: str) -> "TokenTable":
        """tokenizer.py:277-321: reads what ``save`` or LaTeXTokenizer.save wrote."""
        if not os.path.exists(file_path):
            raise FileNotFoundError(f"Tokenizer file not found: {file_path}")
        saved = torch.load(file_path, map_location="cpu")
        return cls(saved["token_to_id"], saved["special_tokens"], saved["max_sequence_length"])


def token_image(tokenizer):
    """The vocabulary as i2l_detokenize reads it, built on the host: ``(tok_bytes uint8, tok_off int32 (V + 1), drop ids,
    unk id)``.  Slot v, for v in 0 .. max id, is ``id_to_token.get(v, UNK string)`` in UTF-8 at
    ``tok_bytes[tok_off[v]:tok_off[v + 1]]`` -- a gap in the id map reads as the UNK string, as ``decode`` reads it
    (tokenizer.py:166-192); the drop ids are the special tokens ``decode(skip_special_tokens=True)`` removes.  Works on
    anything with ``id_to_token``, ``token_to_id`` and ``special_tokens`` (TokenTable, the reference's LaTeXTokenizer).
    None -- the caller keeps the host ``decode`` -- for a tokenizer without them, with more than 8 special ids (the
    kernel's limit), or whose UNK slot does not hold the UNK string (an id beyond the map could not be spelled)."""
    try:
        id_to_token, token_to_id, special = tokenizer.id_to_token, tokenizer.token_to_id, tokenizer.special_tokens
        unk = special["UNK"]
        unk_id = int(token_to_id[unk])
        drop = sorted({int(token_to_id[t]) for t in special.values()})
    except (AttributeError, KeyError, TypeError):
        return None
    ids = [int(i) for i in id_to_token if int(i) >= 0]
    if not ids or len(drop) > 8 or min(drop) < 0 or id_to_token.get(unk_id) != unk:
        return None
    slots = [id_to_token.get(v, unk).encode("utf-8") for v in range(max(ids) + 1)]
    off = np.zeros(len(slots) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in slots], out=off[1:])
    if int(off[-1]) > 0x7fffffff:
        return None
    return np.frombuffer(b"".join(slots), dtype=np.uint8).copy(), off.astype(np.int32), drop, unk_id


class DetokenizeTable:
    """``token_image`` of one tokenizer on one device, and the calls that use it.  ``launch`` enqueues i2l_detokenize on the
    current stream and returns device tensors; ``strings`` slices host copies of them into Python strings."""

    def __init__(self, tokenizer, device):
        image = token_image(tokenizer)
        if image is None:
            raise ValueError("img2latex_amd: this tokenizer has no device vocabulary image (see token_image)")
        tok_bytes, tok_off, drop, self.unk_id = image
        self.device = torch.device(device)
        self.vocab = len(tok_off) - 1
        self.longest = int(np.diff(tok_off).max())
        self.n_drop = len(drop)
        self.tok_bytes = torch.from_numpy(tok_bytes if tok_bytes.size else np.zeros(1, np.uint8)).to(self.device)
        self.tok_off = torch.from_numpy(tok_off).to(self.device)
        self.drop = torch.tensor(drop, dtype=torch.int32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()         # i2l_detokenize reads tok_off from the host

    def capacity(self, rows: int, width: int) -> int:
        """Bytes that hold ANY (rows, width) id matrix: every position the longest token plus a separator."""
        return rows * width * (self.longest + 1)

    def buffers(self, rows: int, width: int):
        """(out_bytes, out_off with the status word behind it (rows + 2 int32), workspace) for ``launch``."""
        L = _lib.lib()
        return (torch.empty((max(self.capacity(rows, width), 1),), dtype=torch.uint8, device=self.device),
                torch.empty((rows + 2,), dtype=torch.int32, device=self.device),
                torch.empty((L.i2l_detokenize_workspace_bytes(rows),), dtype=torch.uint8, device=self.device))

    def launch(self, ids: torch.Tensor, end_id: int, buffers=None, width: Optional[int] = None):
        """ids (rows, >= width) int32 on the device -> (out_bytes, out_off + status) on the current stream."""
        rows, width = ids.shape[0], int(ids.shape[1] if width is None else width)
        out, off, ws = buffers if buffers is not None else self.buffers(rows, width)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().i2l_detokenize(
                ids.data_ptr(), rows, width, ids.stride(0), int(end_id), self.drop.data_ptr(), self.n_drop,
                self.tok_bytes.data_ptr(), self.tok_off.data_ptr(), self.vocab, self.unk_id, out.data_ptr(), out.numel(),
                off.data_ptr(), off.data_ptr() + 4 * (rows + 1), ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "detokenize")
        return out, off

    @staticmethod
    def strings(host_bytes: torch.Tensor, host_off: torch.Tensor) -> List[str]:
        """Host copies of ``launch``'s two tensors (complete: the caller has waited) -> one string per row."""
        off = host_off.tolist()
        if off[-1] != 0:
            raise RuntimeError(f"img2latex_amd: detokenize needs {off[-2]} bytes, the buffer holds {host_bytes.numel()}")
        text = host_bytes.numpy()[:off[-2]].tobytes()
        return [text[a:b].decode("utf-8") for a, b in zip(off[:-2], off[1:-1])]

    def decode_now(self, ids: torch.Tensor, end_id: int):
        """``launch`` + the copies + the wait, for the one-batch callers: (strings, first id of every row on the host --
        what ``_lib.ids_timed_out`` looks at)."""
        out, off = self.launch(ids, end_id)
        tail = torch.cat([off, ids[:, 0]]).cpu()                     # offsets, status, first column: one copy
        n = off.numel()
        total = int(tail[n - 2])
        return self.strings(out[:min(total, out.numel())].cpu(), tail[:n]), tail[n:]


_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def detokenize_table(tokenizer, device) -> Optional[DetokenizeTable]:
    """The DetokenizeTable of (tokenizer, device), built once (the cache dies with the tokenizer; a tokenizer edited
    afterwards needs a new table: build a DetokenizeTable directly).  None when ``token_image`` gives none."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    try:
        per_tok = _TABLES.setdefault(tokenizer, {})
    except TypeError:                                                # not hashable / not weakly referenceable: no cache
        per_tok = {}
    if device not in per_tok:
        per_tok[device] = DetokenizeTable(tokenizer, device) if token_image(tokenizer) is not None else None
    return per_tok[device]


def model_from_checkpoint_config(config: Dict, vocab_size: int) -> Seq2SeqModel:
    """predictor.py:83-126: config["model"] -> Seq2SeqModel constructor arguments."""
    model_config = config.get("model", {})
    model_type = model_config.get("name", "cnn_lstm")
    enc = dict(model_config.get("encoder", {}).get("cnn" if model_type == "cnn_lstm" else "resnet", {}))
    enc["embedding_dim"] = model_config.get("embedding_dim", 256)
    return Seq2SeqModel(model_type=model_type, vocab_size=vocab_size, encoder_params=enc,
                        decoder_params=model_config.get("decoder", {}))


def save_checkpoint(path: str, model: Seq2SeqModel, tokenizer: TokenTable, config: Dict, epoch: int = 0, step: int = 0,
                    metrics: Optional[Dict] = None, optimizer_state_dict: Optional[Dict] = None) -> None:
    """The dict of trainer.py:209-224, readable by the reference's Predictor.from_checkpoint / load_checkpoint."""
    torch.save({"epoch": epoch, "step": step,
                "model_state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
                "optimizer_state_dict": optimizer_state_dict or {}, "metrics": metrics or {}, "config": config,
                "tokenizer_config": tokenizer.config()}, path)


def _is_pil(obj) -> bool:
    try:
        from PIL import Image
    except ImportError:                                                     # pragma: no cover
        return False
    return isinstance(obj, Image.Image)


class Predictor:
    def __init__(self, model: Seq2SeqModel, tokenizer, device: Optional[torch.device] = None,
                 model_type: str = "cnn_lstm", decode_flags: int = 0, well_formed=False):
        # decode_flags (_lib.FLAG_DECODE_BATCHED: the step-batched matrix-core decode) are OR-ed into the flags of every
        # greedy and every sampling decode this predictor launches; 0 = the automatic kernel choice
        self.decode_flags = int(decode_flags)
        # well_formed: every greedy and sampling decode and every N-best beam search (predict_nbest, predict_batch_nbest) of
        # this predictor is the bracket-constrained one (training/constraint.py: groups nest, END within max_length) -- True: the table BracketTable.from_tokenizer gives, or a BracketTable of the
        # caller's; each call's own ``well_formed=`` overrides it.  Off by default: nothing changes without it.
        # "arguments" (or an ArgumentTable): the argument rules on top -- every command also gets the arguments it demands
        # (ArgumentTable.from_tokenizer) -- for the greedy and sampling decodes; the N-best beam search refuses it.
        self.well_formed = well_formed
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("img2latex_amd: Predictor runs on a ROCm device only (no CPU fallback)")
        self.model = model.to(self.device)
        self.tokenizer = tokenizer
        self.model_type = model_type
        self.model.eval()                                                   # predictor.py:55

    @classmethod
    def from_checkpoint(cls, checkpoint_path: str, device: Optional[torch.device] = None,
                        decode_flags: int = 0, well_formed=False) -> "Predictor":
        checkpoint = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        config = checkpoint.get("config", {})
        tcfg = checkpoint.get("tokenizer_config", {})
        tokenizer = TokenTable(tcfg.get("token_to_id"), tcfg.get("special_tokens"), tcfg.get("max_sequence_length", 141))
        model = model_from_checkpoint_config(config, tokenizer.vocab_size)
        model.load_state_dict(checkpoint["model_state_dict"])               # predictor.py:129, strict
        return cls(model=model, tokenizer=tokenizer, device=device,
                   model_type=config.get("model", {}).get("name", "cnn_lstm"), decode_flags=decode_flags,
                   well_formed=well_formed)

    @classmethod
    def from_checkpoints(cls, checkpoint_paths: Sequence[str], weights: Optional[Sequence[float]] = None,
                         combine: str = "logprob", device: Optional[torch.device] = None, decode_flags: int = 0,
                         well_formed=False) -> "Predictor":
        """An ENSEMBLE predictor (this package): the checkpoints' decoders choose every token together
        (model/ensemble.py, i2l_ensemble_decode) under ``combine`` = "logprob" (weighted geometric mean of the members'
        distributions) or "prob" (arithmetic mean), with ``weights`` one per checkpoint (None: equal).  The checkpoints
        must agree on ``token_to_id``, the special tokens, the model type and the encoder's input geometry (height,
        width, channels); the first difference raises ValueError.  ``predict``, ``predict_batch``, ``predict_batch_ids``
        and ``evaluate_batch`` work as for one checkpoint; the stream and N-best methods raise RuntimeError."""
        from ..model.ensemble import EnsembleModel, combine_rule, member_weights
        paths = list(checkpoint_paths)
        if not 1 <= len(paths) <= _lib.MAX_ENSEMBLE:
            raise ValueError(f"img2latex_amd: an ensemble has 1 .. {_lib.MAX_ENSEMBLE} checkpoints, got {len(paths)}")
        weights = member_weights(weights, len(paths))
        combine_rule(combine)
        models, first = [], None
        for path in paths:
            checkpoint = torch.load(path, map_location="cpu", weights_only=False)
            config = checkpoint.get("config", {})
            tcfg = checkpoint.get("tokenizer_config", {})
            tokenizer = TokenTable(tcfg.get("token_to_id"), tcfg.get("special_tokens"), tcfg.get("max_sequence_length", 141))
            model = model_from_checkpoint_config(config, tokenizer.vocab_size)
            enc = model.encoder
            facts = {"token_to_id": tokenizer.token_to_id, "special tokens": tokenizer.special_tokens,
                     "model type": config.get("model", {}).get("name", "cnn_lstm"),
                     "input geometry": (enc.img_height, enc.img_width), "channels": enc.channels}
            if first is None:
                first = (path, tokenizer, facts)
            for name, value in facts.items():
                if value != first[2][name]:
                    shown = "" if name == "token_to_id" else f" ({first[2][name]} / {value})"
                    raise ValueError(f"img2latex_amd: the checkpoints of an ensemble must agree on their {name}: "
                                     f"{first[0]} and {path} differ{shown}")
            model.load_state_dict(checkpoint["model_state_dict"])
            models.append(model)
        return cls(model=EnsembleModel(models, weights, combine), tokenizer=first[1], device=device,
                   model_type=first[2]["model type"], decode_flags=decode_flags, well_formed=well_formed)

    def _single_model(self, what: str) -> None:
        """Refuses ``what`` for an ensemble predictor, before anything is launched."""
        from ..model.ensemble import EnsembleModel
        if isinstance(self.model, EnsembleModel):
            raise RuntimeError(f"img2latex_amd: {what} is single-model (the look-ahead pipeline and the beam search have "
                               "no ensemble form); an ensemble predictor has predict, predict_batch, predict_batch_ids "
                               "and evaluate_batch")

    def _constraint(self, well_formed=None):
        """The BracketTable or ArgumentTable of a call: its own ``well_formed`` (None: the predictor's), True meaning the
        tokenizer's bracket table, "arguments" its argument table."""
        from .constraint import as_table
        return as_table(self.well_formed if well_formed is None else well_formed, self.tokenizer)

    # ------------------------------------------------------------------ predictor.py:396-521
    def _prepare_image(self, image) -> torch.Tensor:
        """One image of any accepted type -> (1, C, 64, 800) on the device, with the reference's rules per type:
        str -> load_image (aspect-preserving LANCZOS, pad / crop, [-1,1] or ImageNet statistics; a missing file gives
        a zero image); tensor / ndarray -> bilinear resize when the size differs, ``/255*2-1`` iff min < 0 or max > 1
        (:493-497 -- so a tensor already in [-1,1] is rescaled again, as in the reference); PIL image -> mode
        conversion, Image.resize((800, 64)) with Pillow's default BICUBIC (aspect NOT kept), ``/255*2-1``."""
        from ..data import load_image, preprocess_batch
        img_size = (64, 800)                                                # :409-414, both model types
        channels = 1 if self.model_type == "cnn_lstm" else 3
        if isinstance(image, str):
            t = load_image(image, img_size, channels).to(self.device)
        elif isinstance(image, torch.Tensor):
            t = self._preprocess_tensor(image, img_size, channels)
        elif isinstance(image, np.ndarray):
            t = self._preprocess_tensor(self._numpy_to_tensor(image, channels), img_size, channels)
        elif _is_pil(image):
            want = "L" if channels == 1 else "RGB"
            if image.mode not in ("L", "RGB"):                              # decoding-side conversion stays with PIL
                image = image.convert(want)
            with torch.cuda.device(self.device):
                t = preprocess_batch([np.array(image)], img_size, channels, "symmetric", keep_aspect=False,
                                     resample="bicubic")[0]
        else:
            raise TypeError(f"Unsupported image type: {type(image)}. "
                            "Expected str, torch.Tensor, numpy.ndarray, or PIL.Image.Image.")
        if self.model_type == "resnet_lstm" and t.shape[0] == 1:            # :453-455
            t = t.repeat(3, 1, 1)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        return t

    def _preprocess_tensor(self, tensor: torch.Tensor, img_size, channels: int) -> torch.Tensor:
        """predictor.py:464-499 on the device."""
        from ..data import resize_bilinear
        tensor = tensor.to(self.device, dtype=torch.float32)
        if tensor.dim() == 2:
            tensor = tensor.unsqueeze(0)
        if tuple(tensor.shape[-2:]) != tuple(img_size):
            tensor = resize_bilinear(tensor.unsqueeze(0) if tensor.dim() == 3 else tensor, img_size)
            if tensor.dim() == 4 and tensor.shape[0] == 1:
                tensor = tensor.squeeze(0)
        if bool(tensor.min() < 0) or bool(tensor.max() > 1):
            tensor = tensor / 255.0
            tensor = tensor * 2.0 - 1.0
        return tensor

    @staticmethod
    def _numpy_to_tensor(array: np.ndarray, channels: int) -> torch.Tensor:
        """predictor.py:501-521: (H,W) -> (1,H,W); (H,W,C) -> (C,H,W) unless the first axis already is 1 or 3."""
        if array.ndim == 2:
            array = np.expand_dims(array, axis=0)
        elif array.ndim == 3 and array.shape[0] not in [1, 3]:
            array = np.transpose(array, (2, 0, 1))
        return torch.from_numpy(np.ascontiguousarray(array)).float()

    def _as_batch(self, images) -> torch.Tensor:
        if isinstance(images, torch.Tensor):
            t = images if images.dim() == 4 else images.unsqueeze(0)
        else:
            items = []
            for im in images:
                if not isinstance(im, torch.Tensor):
                    raise TypeError("img2latex_amd Predictor takes image TENSORS already sized for the model; file / "
                                    "PIL / numpy preprocessing (predictor.py:396-499) is host-side work outside this path")
                items.append(im if im.dim() == 3 else im.squeeze(0))
            t = torch.stack(items)
        return t.to(self.device, dtype=torch.float32).contiguous()

    def predict_batch_ids(self, images, max_length: int = 141, temperature: float = 1.0, top_k: int = 0,
                          top_p: float = 0.0, seed: Optional[int] = None, well_formed=None) -> List[List[int]]:
        """Token ids of the batched loop (predictor.py:254-361): START kept, cut before the first END.
        Sampling (multinomial over the top-k / top-p masked softmax) iff temperature > 0 and
        (top_k > 0 or top_p > 0), exactly the reference's condition (:330); argmax of softmax otherwise."""
        x = self._as_batch(images)
        start, end = self.tokenizer.start_token_id, self.tokenizer.end_token_id
        constraint = self._constraint(well_formed)
        with torch.no_grad():
            enc = self.model.encoder(x)
            if temperature > 0 and (top_k > 0 or top_p > 0.0):
                ids = _lib.check_ids(self._sample_ids(enc, max_length, temperature, top_k, top_p, seed, constraint).cpu())
            else:       # same timeout fallback as Seq2SeqModel._greedy_search
                ids = self.model.greedy_ids_host(enc, start, end, max_length, temperature, stop=_lib.STOP_STICKY,
                                                 select=_lib.SELECT_SOFTMAX, flags=self.decode_flags, constraint=constraint)
        a = ids.numpy()
        stop = (a == end) | (a < 0)                           # first END, or the kernel's "row finished" filler
        lens = np.where(stop.any(axis=1), stop.argmax(axis=1), a.shape[1]).tolist()
        return [[start] + row[:n] for row, n in zip(a.tolist(), lens)]

    def _sample_ids(self, enc, max_length, temperature, top_k, top_p, seed, constraint=None) -> torch.Tensor:
        """The sampling branch of the batched loop (predictor.py:295-331): (B, max_length) ids on the device."""
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        tok0 = torch.full((enc.shape[0],), int(self.tokenizer.start_token_id), dtype=torch.int32, device=enc.device)
        ids, _ = self.model.decoder.sample_steps(enc, max_length, tok0, temperature, top_k, top_p, seed,
                                                 stop=_lib.STOP_STICKY, end_id=self.tokenizer.end_token_id,
                                                 flags=self.decode_flags, constraint=constraint)
        return ids

    def _greedy_strings(self, table: DetokenizeTable, enc, max_length, temperature, **loop) -> List[str]:
        """greedy_ids -> i2l_detokenize -> strings, with ``Seq2SeqModel.greedy_ids_host``'s timeout fallback: the first id
        of every row comes back with the row offsets."""
        import warnings
        start, end = self.tokenizer.start_token_id, self.tokenizer.end_token_id
        loop = dict(loop, flags=int(loop.get("flags", 0)) | self.decode_flags)
        ids, _ = self.model.greedy_ids(enc, start, end, max_length, temperature, **loop)
        texts, first = table.decode_now(ids, end)
        if _lib.ids_timed_out(first):
            warnings.warn("img2latex_amd: grouped decode timed out (GPU oversubscribed?); "
                          "re-running on the row-per-workgroup kernel", RuntimeWarning)
            ids, _ = self.model.greedy_ids(enc, start, end, max_length, temperature, rows_per_workgroup=1, **loop)
            texts, first = table.decode_now(ids, end)
            _lib.check_ids(first)
        return texts

    def _batch_strings(self, table: DetokenizeTable, x: torch.Tensor, max_length, temperature, top_k, top_p, seed,
                       constraint=None) -> List[str]:
        """``predict_batch_ids`` + START / END stripping + ``tokenizer.decode`` (predictor.py:384-391) with the ids staying
        on the device: the same loop launches, then i2l_detokenize (cut before END, drop the special ids, join)."""
        x = self._as_batch(x)
        with torch.no_grad():
            enc = self.model.encoder(x)
            if temperature > 0 and (top_k > 0 or top_p > 0.0):
                ids = self._sample_ids(enc, max_length, temperature, top_k, top_p, seed, constraint)
                texts, first = table.decode_now(ids, self.tokenizer.end_token_id)
                _lib.check_ids(first)
                return texts
            return self._greedy_strings(table, enc, max_length, temperature, stop=_lib.STOP_STICKY,
                                        select=_lib.SELECT_SOFTMAX, constraint=constraint)

    def predict_ids_stream(self, batches, max_length: int = 141, temperature: float = 1.0):
        """``predict_batch_ids`` (the greedy branch: argmax of softmax, sticky stop) for a STREAM of image batches, through
        ``GreedyPipeline``: the decode of batch i shares the GPU with the encoder of batch i + 1 (two batches in flight, the
        schedule bench.py times).  Yields one ``List[List[int]]`` per batch, in order, equal to what ``predict_batch_ids``
        returns for that batch (up to fp32 near-ties between the two decode kernels).  A ResNet encoder's bf16 trunk also
        picks other tile shapes with two trunks in flight, which can move ids; with ``model.encoder.eval_precision =
        "fp32"`` the features of the two paths are bit-identical."""
        self._single_model("predict_ids_stream")
        return self._stream(batches, max_length, temperature, None)

    def predict_strings_stream(self, batches, max_length: int = 141, temperature: float = 1.0, well_formed=None):
        """``predict_ids_stream`` with the strings built on the device: per batch exactly
        ``[tokenizer.decode(seq[1:]) for seq in <that batch of predict_ids_stream>]``.  The pipeline runs i2l_detokenize
        behind each decode and copies the packed bytes + row offsets beside the ids; the host slices them.  A tokenizer
        without a device image (``token_image`` gives None) takes the host ``decode`` on the id stream.  ``well_formed``:
        the bracket-constrained decode; the pipeline then runs the step-batched kernels, not the grouped co-resident ones."""
        self._single_model("predict_strings_stream")
        return self._strings_stream(batches, max_length, temperature, well_formed)

    def _strings_stream(self, batches, max_length, temperature, well_formed):
        table = detokenize_table(self.tokenizer, self.device)
        constraint = self._constraint(well_formed)
        if table is None:
            for seqs in self._stream(batches, max_length, temperature, None, constraint):
                yield [self.tokenizer.decode(seq[1:]) for seq in seqs]
            return
        yield from self._stream(batches, max_length, temperature, table, constraint)

    def _stream(self, batches, max_length, temperature, table, constraint=None):
        from ..pipeline import GreedyPipeline
        start, end = self.tokenizer.start_token_id, self.tokenizer.end_token_id
        n_enc = 2 if hasattr(self.model.encoder, "_trunk_train") else 1      # ResNet trunk: two in flight
        # a constrained decode is a step-batched one: the grouped co-resident kernels have no constrained form
        group = _lib.FLAG_DECODE_GROUP16 if constraint is None else _lib.FLAG_DECODE_BATCHED
        pipe = GreedyPipeline(self.model, start, end, max_length, temperature, rows_per_workgroup=0,
                              decode_flags=group | self.decode_flags, decode_priority=-1, encoder_streams=n_enc,
                              stop=_lib.STOP_STICKY, select=_lib.SELECT_SOFTMAX, detokenize=table, constraint=constraint)

        def finish(ids_host):
            a = ids_host.numpy()
            stop = (a == end) | (a < 0)
            lens = np.where(stop.any(axis=1), stop.argmax(axis=1), a.shape[1]).tolist()
            return [[start] + row[:n] for row, n in zip(a.tolist(), lens)]

        collect = (lambda: finish(pipe.collect())) if table is None else pipe.collect_strings
        try:
            for images in batches:
                if pipe.pending() >= pipe.depth:
                    yield collect()
                pipe.submit(self._as_batch(images))
            while pipe.pending():
                yield collect()
        finally:
            pipe.close()                                     # gives its decoder workspaces back

    def evaluate_batch(self, images, targets: Union[torch.Tensor, Sequence[str]], max_length: Optional[int] = None,
                       return_strings: bool = False, well_formed=None, return_statistics: bool = False,
                       errors=None) -> Dict:
        """One batch of the reference's ``evaluate`` command (cli.py:449-495) with every stage on the device and
        the token ids never leaving HBM between them:

            images    a (B,C,H,W) tensor already shaped for the model, or a list of decoded uint8 arrays
                      ((h,w) / (h,w,3)) that first go through ``preprocess_batch`` (= load_image, data/utils.py:18-90)
            targets   a (B, L) id tensor padded with PAD, or a list of B ``str``: the raw formulas as the data set holds
                      them, tokenized on the device by ``TokenizeTable.collate`` (START formula END, never cut, padded
                      to the longest row: dataset.py:333-335, collator :59-66) and entering the chain as that tensor would
            encoder -> sticky greedy loop (predictor.py:283-358) -> i2l_compact_ids (cut before END, drop the special
            tokens: what tokenizer.decode + tokenizer.encode do to a prediction at cli.py:466-481; targets: drop PAD)
            -> i2l_sequence_metrics -> ONE small device->host copy of the integer statistics -> the reference's
            float64 formulas (calculate_metrics, metrics.py:184-223).

        Returns {"bleu", "levenshtein", "batch_size"} as ``calculate_metrics`` does, plus "pred_ids"/"pred_len"
        (device tensors) for callers that also want the strings.  ``return_strings``: also "pred_text", the
        ``tokenizer.decode`` of every row of "pred_ids", built by i2l_detokenize in the same chain (from the decode's ids
        under the compaction's own cut and drop rule: the compacted rows are zero-padded and the kernel takes no
        lengths) and copied beside the statistics; a tokenizer without a device image decodes "pred_ids" on the host.
        ``return_statistics``: also "statistics", as in ``evaluate_stream``.  ``errors``: a ``metrics.ErrorAnalysis``; its
        i2l_edit_alignment launch then follows i2l_sequence_metrics on the same stream over the same compacted ids and adds
        the batch to its confusion matrix, and the batch's edit distances -- already on the host with the statistics -- go
        into its buckets.  None (the default): not one launch or copy more."""
        launched = self._evaluate_launch(images, targets, max_length, return_strings=return_strings,
                                         constraint=self._constraint(well_formed), errors=errors)
        launched["return_statistics"] = return_statistics
        return self._evaluate_finish(launched)

    def evaluate_stream(self, batches, max_length: Optional[int] = None, lookahead: int = 2, return_strings: bool = False,
                        return_statistics: bool = False, well_formed=None, errors=None):
        """``evaluate_batch`` over an iterable of (images, targets), one result per batch in order, software-pipelined:
        the host work of batch i+1 (shape pass, packing the ragged pages into pinned memory, their upload on a side
        stream) runs while the device is still busy with batch i, and the host only waits for batch i's statistics
        after batch i+1 has been enqueued.  On the device the two batches in flight share the GPU the way GreedyPipeline's
        do: preprocessing + encoder + decoder prepare of batch i+1 on one stream, the decode (8-member grouped kernel) +
        id compaction + statistics of batch i on another, the first held back until the second's decode is resident.
        ``lookahead`` batches are enqueued beyond the one whose statistics the host waits for (r04: 2 -- with 1 the host only
        began batch i + 2 once batch i had finished, its 0.7 ms of packing then landed inside decode(i + 1), and the
        encoder of batch i + 2 started where that decode ended instead of beside it: profiles/r04/evaluate_chain.txt).
        This is the loop of cli.py:449-495.

        A batch's targets may be a list of ``str`` (raw formulas) instead of a tensor; batches of both kinds may be mixed.
        The text is packed and uploaded where a tensor's upload goes, and tokenized behind it on the caller's stream, at a
        width known without asking the device: ``tokenizer.max_sequence_length + 2``, with the compaction dropping the
        PAD.  ``collate``'s exact width would need a host wait for the counts in the middle of the look-ahead, and the
        other host-known width, the byte-length bound, is about twice as wide and takes the statistics kernel off its
        <= 256 path; the statistics do not depend on the padded width.  ``collate`` never cuts a row, so i2l_tokenize's
        status word travels with the statistics, and a batch in which a row WAS cut (a formula of more than
        max_sequence_length tokens) is run again with ``collate``'s width when its statistics are collected.

        ``return_strings``: as in ``evaluate_batch`` ("pred_text").  ``return_statistics``: every result also carries
        "statistics", a host copy of its (B, 9) int32 statistics rows; ``metrics.metrics_from_packed`` of the rows of all
        batches, concatenated, gives the means over all pairs of a split (not means of batch means).  ``well_formed``: the
        bracket-constrained decode (step-batched kernels) in the place of the grouped one, the schedule otherwise the same.
        ``errors``: as in ``evaluate_batch``; the alignment launch sits behind the statistics on the decode's stream."""
        self._single_model("evaluate_stream")
        return self._evaluate_stream(batches, max_length, lookahead, return_strings, return_statistics, well_formed, errors)

    def _evaluate_stream(self, batches, max_length, lookahead, return_strings, return_statistics, well_formed, errors=None):
        from collections import deque
        pending = deque()
        constraint = self._constraint(well_formed)
        lookahead = max(1, min(int(lookahead), 2))           # the landing buffers / decoder slots rotate over 4 / 3
        for images, targets in batches:
            pending.append(self._evaluate_launch(images, targets, max_length, side_upload=True, coresident=True,
                                                 return_strings=return_strings, constraint=constraint, errors=errors))
            pending[-1]["return_statistics"] = return_statistics
            if len(pending) > lookahead:
                yield self._evaluate_finish(pending.popleft())
        while pending:
            yield self._evaluate_finish(pending.popleft())

    def _evaluate_launch(self, images, targets, max_length: Optional[int], side_upload: bool = False,
                         rows_per_workgroup: int = 0, coresident: bool = False, return_strings: bool = False,
                         constraint=None, errors=None):
        """Enqueues the whole chain of one batch and the copy of its statistics to pinned memory; no host wait.
        ``coresident``: two streams -- everything up to the decoder's prepare on the first, the decode and what follows on the
        second (see evaluate_stream); otherwise the whole chain on the current stream."""
        from . import metrics as M
        import contextlib
        L = _lib.lib()
        tk = self.tokenizer
        raw = images
        # host-side preparation and everything that touches the CALLER's stream first (targets, the small constant tensors)
        T = int(max_length if max_length is not None else tk.max_sequence_length)
        tok_status = None
        if isinstance(targets, (list, tuple)) and targets and all(isinstance(t, str) for t in targets):
            from .tokenizer import tokenize_table
            ttable = tokenize_table(tk, self.device)
            if ttable is None:
                raise ValueError("img2latex_amd: string targets need a tokenizer with a device vocabulary table "
                                 "(tokenize_image); encode them with the tokenizer's own encode and pass the id tensor")
            if side_upload:                                  # evaluate_stream: no host wait (see its docstring)
                text, row_off = ttable.upload(targets)
                tgt, _, _, tok_status = ttable.launch(text, row_off, int(tk.max_sequence_length) + 2, True)
            else:
                tgt = ttable.collate(targets)
        else:
            tgt = targets.to(self.device, dtype=torch.int32).contiguous()
        if tgt.dim() != 2:
            raise RuntimeError(f"targets must be (B, L) token ids, got {tuple(tgt.shape)}")
        special = getattr(tk, "special_tokens", DEFAULT_SPECIAL_TOKENS)
        drop = sorted({tk.token_to_id[t] for t in special.values()}) if hasattr(tk, "token_to_id") else \
            sorted({tk.pad_token_id, tk.start_token_id, tk.end_token_id})
        if len(drop) > 8:
            raise NotImplementedError("img2latex_amd: at most 8 special token ids")
        dev = tgt.device
        key = (tuple(drop), tk.pad_token_id, dev)
        if getattr(self, "_drop_key", None) != key:
            self._drop = torch.tensor(drop, dtype=torch.int32, device=dev)
            self._pad = torch.tensor([tk.pad_token_id], dtype=torch.int32, device=dev)
            self._drop_key = key
        cur = torch.cuda.current_stream(self.device)
        if coresident:
            st = self.__dict__.setdefault("_ev_streams", {})
            if "enc" not in st:
                st["enc"] = torch.cuda.Stream(self.device)
                st["dec"] = torch.cuda.Stream(self.device, priority=-1)
                # (r04, measured and dropped: id compaction + statistics on a third stream, so that the decode stream goes from
                # decode(i) straight into decode(i + 1) -- three kernels sharing the CUs: 1.25 -> 1.63 ms per batch)
                st["stat"] = st["dec"]
                st["resident"], st["n"] = torch.zeros(1, dtype=torch.int32, device=self.device), 0
            s_enc, s_dec, s_stat = st["enc"], st["dec"], st["stat"]
            s_enc.wait_stream(cur)                           # the caller's tensors, tgt, the constants
            on_enc = lambda: torch.cuda.stream(s_enc)
            on_dec = lambda: torch.cuda.stream(s_dec)
            on_stat = lambda: torch.cuda.stream(s_stat)
        else:
            on_enc = on_dec = on_stat = contextlib.nullcontext
        with on_enc():
            if coresident and st["n"] > 0:                   # not before the previous batch's decode owns its compute units
                _lib.check(L.i2l_stream_wait_value32(st["resident"].data_ptr(), st["n"], 20000.0, _lib.stream_ptr()),
                           "stream_wait_value32")
            if not isinstance(images, torch.Tensor):
                from ..data import preprocess_batch
                enc_mod = self.model.encoder
                if side_upload and getattr(self, "_up_stream", None) is None:
                    self._up_stream = torch.cuda.Stream(self.device)
                with torch.cuda.device(self.device):
                    images = preprocess_batch(list(images), (enc_mod.img_height, enc_mod.img_width), enc_mod.channels, True,
                                              upload_stream=self._up_stream if side_upload else None)
            x = self._as_batch(images)
        B = x.shape[0]
        if tgt.shape[0] != B:
            raise RuntimeError(f"targets must be ({B}, L) token ids, got {tuple(tgt.shape)}")
        W = max(T, tgt.shape[1])
        prepared = None
        with on_enc(), torch.cuda.device(dev), torch.no_grad():
            t_ids = torch.zeros((B, W), dtype=torch.int32, device=dev)
            t_len = torch.empty((B,), dtype=torch.int32, device=dev)
            _lib.check(L.i2l_compact_ids(tgt.data_ptr(), B, tgt.shape[1], tgt.stride(0), -1, self._pad.data_ptr(), 1,
                                         t_ids.data_ptr(), W, t_len.data_ptr(), _lib.stream_ptr()), "compact_ids")
            enc = self.model.encoder(x)
            if coresident:
                w_, keep_, enc_c = self.model.decoder.prepare(enc, slot=("eval", id(self), st["n"] % 3))
                st["n"] += 1
                prepared = (w_, keep_, enc_c, self.model.decoder._ws)
                enc_done = torch.cuda.Event()
                enc_done.record(s_enc)
        with on_dec(), torch.cuda.device(dev):
            if coresident:
                s_dec.wait_event(enc_done)
                for t_ in (x, tgt, t_ids, t_len, enc):
                    t_.record_stream(s_dec)                  # allocated on the first stream, read on the second
            with torch.no_grad():
                ids, _ = self.model.greedy_ids(enc, tk.start_token_id, tk.end_token_id, T, stop=_lib.STOP_STICKY,
                                               select=_lib.SELECT_SOFTMAX, rows_per_workgroup=rows_per_workgroup,
                                               flags=(_lib.FLAG_DECODE_GROUP16 if coresident else 0) | self.decode_flags,
                                               prepared=prepared,
                                               resident=(st["resident"], st["n"]) if coresident else None,
                                               constraint=constraint)
            if coresident:
                decoded = torch.cuda.Event()
                decoded.record(s_dec)
        with on_stat(), torch.cuda.device(dev):
            if coresident:
                s_stat.wait_event(decoded)
                for t_ in (ids, t_ids, t_len) + (() if tok_status is None else (tok_status,)):
                    t_.record_stream(s_stat)
            p_ids = torch.zeros((B, W), dtype=torch.int32, device=dev)
            p_len = torch.empty((B,), dtype=torch.int32, device=dev)
            with torch.no_grad():
                _lib.check(L.i2l_compact_ids(ids.data_ptr(), B, T, ids.stride(0), int(tk.end_token_id),
                                             self._drop.data_ptr(), len(drop), p_ids.data_ptr(), W, p_len.data_ptr(),
                                             _lib.stream_ptr()), "compact_ids")
                packed = M.device_sequence_statistics(p_ids, p_len, t_ids, t_len, 4, tk.pad_token_id, _max_len=W, defer=True)
                if errors is not None:
                    errors.update(p_ids, p_len, t_ids, t_len)
            # statistics + the first id of every row (-3 = the grouped decode timed out) in ONE device->host copy
            packed = torch.cat([packed, ids[:, :1]] + ([] if tok_status is None else [tok_status.expand(B)[:, None]]), dim=1)
            # pinned landing buffers are reused (registering pinned memory costs ~1 ms): a ring of 4, more than the
            # two batches evaluate_stream ever has in flight
            ring = self.__dict__.setdefault("_host_ring", {"bufs": [None] * 4, "next": 0})
            slot = ring["next"]
            ring["next"] = (slot + 1) % 4
            if ring["bufs"][slot] is None or ring["bufs"][slot].numel() < packed.numel():
                ring["bufs"][slot] = torch.empty((packed.numel(),), dtype=torch.int32).pin_memory()
            host = ring["bufs"][slot][:packed.numel()].view(packed.shape)
            host.copy_(packed, non_blocking=True)
            text = None
            table = detokenize_table(tk, dev) if return_strings else None
            if table is not None:
                t_bytes, t_off = table.launch(ids, int(tk.end_token_id), width=T)
                land = ring.setdefault("text", [None] * 4)           # the strings' landing buffers rotate with the statistics'
                if land[slot] is None or land[slot][0].numel() < t_bytes.numel() or land[slot][1].numel() < t_off.numel():
                    land[slot] = (torch.empty((t_bytes.numel(),), dtype=torch.uint8).pin_memory(),
                                  torch.empty((t_off.numel(),), dtype=torch.int32).pin_memory())
                text = (land[slot][0][:t_bytes.numel()], land[slot][1][:t_off.numel()])
                text[0].copy_(t_bytes, non_blocking=True)
                text[1].copy_(t_off, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        return dict(host=host, done=done, keep=(packed, x, tgt), p_ids=p_ids, p_len=p_len, raw=(raw, targets, max_length),
                    rows_per_workgroup=rows_per_workgroup, return_strings=return_strings, text=text, constraint=constraint,
                    errors=errors, aligned=(p_ids, p_len, t_ids, t_len))

    def _evaluate_finish(self, h) -> Dict:
        from . import metrics as M
        h["done"].synchronize()
        host = h["host"]
        if _lib.ids_timed_out(host[:, 9:10]) and h["rows_per_workgroup"] == 0:
            # the timeout fallback of Seq2SeqModel.greedy_ids_host: the row-per-workgroup kernel needs no partner
            raw, targets, max_length = h["raw"]
            if h["errors"] is not None:
                h["errors"].retract(*h["aligned"])           # this run's rows are not the batch's
            again = self._evaluate_launch(raw, targets, max_length, rows_per_workgroup=1, return_strings=h["return_strings"],
                                          constraint=h["constraint"], errors=h["errors"])
            again["return_statistics"] = h.get("return_statistics", False)
            return self._evaluate_finish(again)
        _lib.check_ids(host[:, 9:10])
        if host.shape[1] > 10 and int(host[0, 10]) != 0:
            # string targets at the stream's fixed width and a row was cut: once more with collate's width
            raw, targets, max_length = h["raw"]
            if h["errors"] is not None:
                h["errors"].retract(*h["aligned"])
            again = self._evaluate_launch(raw, targets, max_length, rows_per_workgroup=h["rows_per_workgroup"],
                                          return_strings=h["return_strings"], constraint=h["constraint"], errors=h["errors"])
            again["return_statistics"] = h.get("return_statistics", False)
            return self._evaluate_finish(again)
        out = M.metrics_from_packed(host)
        if h["errors"] is not None:
            h["errors"].add_distances(host[:, 0])
        out["pred_ids"], out["pred_len"] = h["p_ids"], h["p_len"]
        if h.get("return_statistics"):
            out["statistics"] = host[:, :9].clone()                  # the landing buffer is reused
        if h["text"] is not None:
            out["pred_text"] = DetokenizeTable.strings(*h["text"])
        elif h["return_strings"]:
            rows, lens = h["p_ids"].cpu().tolist(), h["p_len"].cpu().tolist()
            out["pred_text"] = [self.tokenizer.decode(r[:n]) for r, n in zip(rows, lens)]
        return out

    def predict_batch(self, images, beam_size: int = 0, max_length: int = 141, temperature: float = 1.0,
                      top_k: int = 0, top_p: float = 0.0, batch_size: int = 16, seed: Optional[int] = None,
                      well_formed=None) -> List[str]:
        """predictor.py:205-394: every image through ``_prepare_image`` (:242), stacked, the batched greedy loop.  As in
        the reference beam_size is clamped to 0 (:231-235)."""
        if isinstance(images, torch.Tensor):
            images = [images] if images.dim() <= 3 else list(images)
        results: List[str] = []
        start, end = self.tokenizer.start_token_id, self.tokenizer.end_token_id
        table = detokenize_table(self.tokenizer, self.device)               # None: the tokenizer keeps its host decode
        constraint = self._constraint(well_formed)
        for i in range(0, len(images), batch_size):
            x = torch.stack([self._prepare_image(im) for im in images[i:i + batch_size]])
            if x.dim() == 5 and x.shape[1] == 1:                            # :254-257
                x = x.squeeze(1)
            if table is not None:
                results.extend(self._batch_strings(table, x, max_length, temperature, top_k, top_p,
                                                   None if seed is None else seed + i, constraint))
                continue
            for seq in self.predict_batch_ids(x, max_length, temperature, top_k, top_p,
                                              None if seed is None else seed + i,
                                              well_formed=False if constraint is None else constraint):
                if seq and seq[0] == start:                                 # :384-388
                    seq = seq[1:]
                if seq and seq[-1] == end:
                    seq = seq[:-1]
                results.append(self.tokenizer.decode(seq))
        return results

    def predict(self, image, beam_size: int = 0, max_length: int = 141, temperature: float = 1.0, top_k: int = 0,
                top_p: float = 0.0, well_formed=None) -> str:
        """predictor.py:139-203: one image (path / PIL / ndarray / tensor) through ``_prepare_image`` and
        Seq2SeqModel.inference (greedy; beam clamped to 0)."""
        x = self._prepare_image(image).to(self.device)
        start, end = self.tokenizer.start_token_id, self.tokenizer.end_token_id
        table = detokenize_table(self.tokenizer, self.device)
        constraint = self._constraint(well_formed)
        if table is not None and x.dim() == 4 and x.shape[0] == 1:
            # one image: _greedy_search's loop (logits arg max, no sticky stop; top_k / top_p ignored as there), the row
            # cut before its first END and decoded on the device
            with torch.no_grad():
                return self._greedy_strings(table, self.model.encoder(x), max_length, temperature, constraint=constraint)[0]
        with torch.no_grad():
            seq = self.model.inference(image=x, start_token_id=start, end_token_id=end, max_length=max_length,
                                       beam_size=0, temperature=temperature, top_k=top_k, top_p=top_p,
                                       constraint=constraint)
        if seq and isinstance(seq[0], list):
            seq = seq[0]
        if seq and seq[0] == start:
            seq = seq[1:]
        if seq and seq[-1] == end:
            seq = seq[:-1]
        return self.tokenizer.decode(seq)

    def predict_batch_nbest(self, images, beam_size: int = 5, nbest: Optional[int] = None, max_length: int = 141,
                            length_penalty: float = 0.0, batch_size: int = 16,
                            well_formed=None) -> List[List[Tuple[str, float, float]]]:
        """Per image the (latex, score, key) of its ``nbest`` (default ``beam_size``) best beam-search hypotheses in rank
        order (Seq2SeqModel.beam_search_nbest: key = score / length ** length_penalty), every image through
        ``_prepare_image`` as in ``predict_batch``, the ids through the tokenizer's own ``decode``.  ``well_formed``: the
        well-formed search, every hypothesis nesting its groups and ending on END (None: the predictor's own setting)."""
        self._single_model("predict_batch_nbest")
        constraint = self._constraint(well_formed)
        if constraint is not None and constraint.kind != _lib.CONSTRAIN_BRACKETS:
            raise RuntimeError("img2latex_amd: the argument rules exist for the greedy and sampling decode only; the N-best "
                               "beam search takes well_formed=True")
        if isinstance(images, torch.Tensor):
            images = [images] if images.dim() <= 3 else list(images)
        start, end = self.tokenizer.start_token_id, self.tokenizer.end_token_id
        results: List[List[Tuple[str, float, float]]] = []
        for i in range(0, len(images), batch_size):
            x = torch.stack([self._prepare_image(im) for im in images[i:i + batch_size]])
            if x.dim() == 5 and x.shape[1] == 1:
                x = x.squeeze(1)
            with torch.no_grad():
                rows = self.model.beam_search_nbest(self.model.encoder(x.to(self.device)), start, end, max_length,
                                                    beam_size, nbest=nbest, length_penalty=length_penalty,
                                                    constraint=constraint)
            results.extend([(self.tokenizer.decode(h.tokens), h.score, h.key) for h in hyps] for hyps in rows)
        return results

    def predict_nbest(self, image, beam_size: int = 5, nbest: Optional[int] = None, max_length: int = 141,
                      length_penalty: float = 0.0, well_formed=None) -> List[Tuple[str, float, float]]:
        """``predict_batch_nbest`` for one image (path / PIL / ndarray / tensor)."""
        self._single_model("predict_nbest")
        return self.predict_batch_nbest([image], beam_size, nbest, max_length, length_penalty, well_formed=well_formed)[0]

    def predict_batch_samples(self, images, samples: int = 8, rank: str = "consensus", max_length: int = 141,
                              temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, seed: int = 0,
                              well_formed=None, length_penalty: float = 0.0,
                              batch_size: int = 16) -> List[List[Tuple[str, float, float]]]:
        """Per image the (latex, score, key) of ``samples`` (1 .. 16) top-k / top-p draws, best first
        (Seq2SeqModel.sample_nbest: ``rank="consensus"`` puts the draw with the smallest summed edit distance to the
        others first and ``key`` is that sum; ``rank="logprob"`` orders by ``key = score / length ** length_penalty``).
        Every image goes through ``_prepare_image`` as in ``predict_batch``; batch i draws with ``seed + i``.  The strings
        come from the device detokenizer where the tokenizer has a device image, else from its own ``decode``.
        ``well_formed``: True keeps every draw's groups nested, "arguments" also gives every command its arguments, and
        both end every draw on END (None: the predictor's own setting)."""
        self._single_model("predict_batch_samples")
        constraint = self._constraint(well_formed)
        if isinstance(images, torch.Tensor):
            images = [images] if images.dim() <= 3 else list(images)
        start, end = self.tokenizer.start_token_id, self.tokenizer.end_token_id
        table = detokenize_table(self.tokenizer, self.device)
        results: List[List[Tuple[str, float, float]]] = []
        for i in range(0, len(images), batch_size):
            x = torch.stack([self._prepare_image(im) for im in images[i:i + batch_size]])
            if x.dim() == 5 and x.shape[1] == 1:
                x = x.squeeze(1)
            with torch.no_grad():
                out = self.model.sample_multi_device(self.model.encoder(x.to(self.device)), start, end, max_length, samples,
                                                     temperature, top_k, top_p, seed + i, rank, length_penalty,
                                                     constraint=constraint)
            n, per = out["order"].shape
            order, score, key = out["order"].cpu().tolist(), out["score"].cpu().tolist(), out["key"].cpu().tolist()
            if table is not None:
                text, _ = table.decode_now(out["ids"].view(n * per, -1), end)
            else:
                lens = (out["len"] - out["finished"]).cpu().view(-1).tolist()
                text = [self.tokenizer.decode(row[:m]) for row, m in zip(out["ids"].view(n * per, -1).cpu().tolist(), lens)]
            results.extend([(text[j * per + s], score[j][s], key[j][s]) for s in order[j]] for j in range(n))
        return results

    def predict_samples(self, image, samples: int = 8, rank: str = "consensus", max_length: int = 141,
                        temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, seed: int = 0, well_formed=None,
                        length_penalty: float = 0.0) -> List[Tuple[str, float, float]]:
        """``predict_batch_samples`` for one image (path / PIL / ndarray / tensor)."""
        self._single_model("predict_samples")
        return self.predict_batch_samples([image], samples, rank, max_length, temperature, top_k, top_p, seed,
                                          well_formed=well_formed, length_penalty=length_penalty)[0]
