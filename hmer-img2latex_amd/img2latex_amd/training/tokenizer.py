"""Formula strings -> token ids on the device: LaTeXTokenizer.encode / encode_batch (reference
img2latex/data/tokenizer.py:143-164,196-232) and the data set's ``START formula END`` rule (data/dataset.py:333-335, its
collator :59-66) through i2l_tokenize.  The other half of ``DetokenizeTable`` (training/predictor.py): strings in at the
boundary, strings out, the ids never on the host in between."""
from __future__ import annotations

import weakref
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

STATUS_TRUNCATED, STATUS_BAD_OFFSETS, STATUS_BAD_TABLE = 1, 2, 4     # i2l_tokenize's *status bits


def pack_texts(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """``(bytes uint8, offsets int32 (len(texts) + 1))``: the texts in UTF-8 back to back, text r at
    ``bytes[offsets[r]:offsets[r + 1]]``.  One join + one encode for the batch; the per-text byte lengths are the
    character counts when the batch is ASCII and are only taken text by text when it is not.  A string that has no UTF-8
    form (a lone surrogate) raises UnicodeEncodeError: i2l_tokenize is promised well-formed UTF-8."""
    texts = list(texts)
    blob = "".join(texts).encode("utf-8")
    lens = np.fromiter(map(len, texts), dtype=np.int64, count=len(texts))
    if int(lens.sum()) != len(blob):
        lens = np.fromiter((len(t.encode("utf-8")) for t in texts), dtype=np.int64, count=len(texts))
    if len(blob) > 0x7fffffff:
        raise ValueError("img2latex_amd: more than 2^31 - 1 bytes of text in one batch")
    off = np.zeros(len(texts) + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    return np.frombuffer(blob, dtype=np.uint8), off


def upload_packed(data: np.ndarray, off: np.ndarray, device):
    """``pack_texts``' result in ONE host -> device copy on the current stream, the offsets in front of the bytes:
    ``(text uint8, row_off int32)`` device views of it."""
    head = off.size * 4
    both = np.empty(head + max(data.size, 1), dtype=np.uint8)
    both[:head] = off.view(np.uint8)
    both[head:head + data.size] = data
    dev = torch.from_numpy(both).to(device)
    return dev[head:head + data.size], dev[:head].view(torch.int32)


def tokenize_image(tokenizer) -> Optional[np.ndarray]:
    """The vocabulary as i2l_tokenize probes it: the self-contained hash table image the library's host function
    i2l_tokenize_table_build makes from ``token_to_id`` (every key in UTF-8 with its id), as a uint8 array.  Works on
    anything with ``token_to_id`` and the four special ids (TokenTable, the reference's LaTeXTokenizer).  None -- the caller
    keeps its host ``encode`` -- for a tokenizer without them, with a key that is no ``str`` or has no UTF-8 form, or
    with an id outside int32."""
    try:
        items = list(tokenizer.token_to_id.items())
        for name in ("pad_token_id", "start_token_id", "end_token_id", "unk_token_id"):
            int(getattr(tokenizer, name))
        keys = [k.encode("utf-8") for k, _ in items]
        ids = np.array([int(v) for _, v in items], dtype=np.int64)
    except (AttributeError, KeyError, TypeError, ValueError, UnicodeEncodeError):
        return None
    if ids.size and (ids.min() < -2 ** 31 or ids.max() > 2 ** 31 - 1):
        return None
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    L = _lib.lib()
    size = L.i2l_tokenize_table_bytes(len(keys), int(off[-1]))
    if size == 0:
        return None
    blob = np.frombuffer(b"".join(keys), dtype=np.uint8) if off[-1] else np.zeros(1, np.uint8)
    off32, ids32 = off.astype(np.int32), np.ascontiguousarray(ids.astype(np.int32))
    image = np.empty(size, dtype=np.uint8)
    _lib.check(L.i2l_tokenize_table_build(blob.ctypes.data, off32.ctypes.data, ids32.ctypes.data if ids32.size else None,
                                          len(keys), image.ctypes.data, image.size), "tokenize_table_build")
    return image


class TokenizeTable:
    """``tokenize_image`` of one tokenizer on one device, and the calls that use it.  ``launch`` enqueues i2l_tokenize on
    the current stream and returns device tensors; ``encode_batch`` and ``collate`` take Python strings."""

    def __init__(self, tokenizer, device):
        image = tokenize_image(tokenizer)
        if image is None:
            raise ValueError("img2latex_amd: this tokenizer has no device vocabulary table (see tokenize_image)")
        self.device = torch.device(device)
        self.image_host, self._image = image, None                   # uploaded by the first launch
        self.pad_id, self.start_id = int(tokenizer.pad_token_id), int(tokenizer.start_token_id)
        self.end_id, self.unk_id = int(tokenizer.end_token_id), int(tokenizer.unk_token_id)
        self.max_sequence_length = getattr(tokenizer, "max_sequence_length", None)

    @property
    def image(self) -> torch.Tensor:
        if self._image is None:
            self._image = torch.from_numpy(self.image_host).to(self.device)
        return self._image

    def upload(self, texts: Sequence[str], packed=None):
        """``pack_texts`` (or its result, ``packed``) + ONE host -> device copy on the current stream, the offsets in front
        of the bytes: ``(text uint8, row_off int32)`` device views of it."""
        return upload_packed(*(pack_texts(texts) if packed is None else packed), self.device)

    def launch(self, text: torch.Tensor, row_off: torch.Tensor, width: int, add_special: bool = False,
               out: Optional[torch.Tensor] = None):
        """text (uint8) and row_off (int32, rows + 1) on the device -> ``(ids (rows, width) int32, out_len (rows),
        out_count (rows), status (1))`` on the current stream, no host wait.  ``out``: a (rows, >= width) int32 matrix to
        write into (columns behind ``width`` stay as they are); ``ids`` is then a view of it."""
        rows, width = row_off.numel() - 1, int(width)
        if out is None:
            out = torch.empty((rows, max(width, 1)), dtype=torch.int32, device=self.device)
        meta = torch.empty((2 * rows + 1,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().i2l_tokenize(
                text.data_ptr() if text.numel() else None, text.numel(), row_off.data_ptr(), rows, self.image.data_ptr(),
                self.image.numel(), self.unk_id, self.pad_id, self.start_id, self.end_id, int(bool(add_special)), width,
                out.data_ptr(), out.stride(0), meta.data_ptr(), meta.data_ptr() + 4 * rows, meta.data_ptr() + 8 * rows,
                _lib.stream_ptr()), "tokenize")
        if rows == 0:
            meta.zero_()
        return out[:, :width], meta[:rows], meta[rows:2 * rows], meta[2 * rows:]

    def encode_batch(self, texts: Sequence[str], add_special_tokens: bool = False, padding: bool = True,
                     truncation: bool = True) -> torch.Tensor:
        """``LaTeXTokenizer.encode_batch`` (tokenizer.py:196-232) at ``tokenizer.max_sequence_length``: every text split
        as ``str.split()`` splits it, looked up (unknown -> UNK), with START / END around it when asked, cut to the
        maximum length and padded with PAD.  Returns a (len(texts), max_sequence_length) **int32 tensor on the device** --
        the project's id type; the reference returns int64 on the CPU.  ``padding=False`` or ``truncation=False`` give
        ragged rows in the reference too (its ``torch.tensor`` then fails unless all rows happen to agree), so both are
        refused here; ``collate`` is the untruncated rule."""
        if not padding or not truncation:
            raise ValueError("img2latex_amd: encode_batch returns one rectangular tensor: padding=False / truncation=False "
                             "have no such result (the reference's has none either); use collate() for untruncated rows")
        if self.max_sequence_length is None or int(self.max_sequence_length) <= 0:
            raise ValueError("img2latex_amd: encode_batch needs the tokenizer's max_sequence_length")
        text, off = self.upload(texts)
        return self.launch(text, off, int(self.max_sequence_length), add_special_tokens)[0]

    def collate(self, formulas: Sequence[str]) -> torch.Tensor:
        """The data set's rule (dataset.py:333-335 + Im2LatexCollator :59-66): row i is ``START formula_i END``, never
        cut, padded with PAD to the longest row of the batch; (B, longest) int32 on the device.  The launch is sized from
        the byte lengths (a row of b bytes has at most (b + 1) // 2 tokens: they need a separator between them), and ONE
        small device -> host read of the largest count gives the width."""
        formulas = list(formulas)
        if not formulas:
            return torch.empty((0, 0), dtype=torch.int32, device=self.device)
        data, off = pack_texts(formulas)
        bound = (int(np.diff(off).max()) + 1) // 2 + 2
        text, row_off = self.upload(formulas, (data, off))
        ids, _, count, _ = self.launch(text, row_off, bound, True)
        return ids[:, :int(count.max())].contiguous()


_TABLES: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def tokenize_table(tokenizer, device) -> Optional[TokenizeTable]:
    """The TokenizeTable of (tokenizer, device), built once (the cache dies with the tokenizer; a tokenizer edited
    afterwards needs a new table: build a TokenizeTable directly).  None when ``tokenize_image`` gives none."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    try:
        per_tok = _TABLES.setdefault(tokenizer, {})
    except TypeError:                                                # not hashable / not weakly referenceable: no cache
        per_tok = {}
    if device not in per_tok:
        try:
            per_tok[device] = TokenizeTable(tokenizer, device)
        except ValueError:
            per_tok[device] = None
    return per_tok[device]
