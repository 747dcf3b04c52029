"""Seq2SeqModel with the reference's surface (img2latex/model/seq2seq.py:17-298).

``forward`` / ``inference`` / ``_greedy_search`` / ``_beam_search`` keep the reference's
argument meaning, defaults, return types and post-processing; the encoder and the
whole decode loop run as HIP kernels (one persistent launch per search, one
device->host copy of the ids at the end instead of a sync per step).
"""
from __future__ import annotations

import ctypes
import math
import warnings
from collections import namedtuple
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from .cnn_encoder import CNNEncoder
from .lstm_decoder import LSTMDecoder

# one row of beam_search_nbest: tokens (START stripped, cut at END), the raw sum of log-probabilities, the ranking key
# score / norm[length] and whether the beam ended in END
BeamHypothesis = namedtuple("BeamHypothesis", ["tokens", "score", "key", "finished"])
# one row of sample_nbest: tokens (cut at END), the sum of the log-probabilities of its tokens (END included) under the
# constraint-renormalised model, the ranking key, the summed edit distance to the image's other samples, whether it
# ended in END, and which draw it was
SampleHypothesis = namedtuple("SampleHypothesis", ["tokens", "score", "key", "risk", "finished", "sample"])
RANKS = {"consensus": _lib.RANK_CONSENSUS, "logprob": _lib.RANK_LOGPROB}


def length_norm_table(max_length: int, length_penalty: float = 0.0, length_norm: Optional[Sequence[float]] = None):
    """The float64 table of ``max_length + 1`` divisors beam_search_nbest ranks by (index: tokens after START, END
    included), or None for all ones.  ``length_penalty = a``: ``norm[n] = float(n) ** a`` for n >= 1, ``norm[0] = 1``.
    ``length_norm``: the caller's own table, validated here -- ValueError for a wrong length, a non-finite or
    non-positive value, or a non-zero ``length_penalty`` beside it."""
    if length_norm is not None:
        if length_penalty != 0.0:
            raise ValueError("img2latex_amd: pass length_norm or a non-zero length_penalty, not both")
        table = [float(v) for v in length_norm]
        if len(table) != max_length + 1:
            raise ValueError(f"img2latex_amd: length_norm needs max_length + 1 = {max_length + 1} values, got {len(table)}")
        if not all(math.isfinite(v) and v > 0.0 for v in table):
            raise ValueError("img2latex_amd: every length_norm value must be finite and > 0")
        return table
    if not math.isfinite(length_penalty):
        raise ValueError("img2latex_amd: length_penalty must be finite")
    if length_penalty == 0.0:
        return None
    table = [1.0] + [float(n) ** float(length_penalty) for n in range(1, max_length + 1)]
    if not all(math.isfinite(v) and v > 0.0 for v in table):
        raise ValueError(f"img2latex_amd: length_penalty {length_penalty} leaves a table value that is not finite and > 0")
    return table


class Seq2SeqModel(nn.Module):
    def __init__(self, model_type: str = "cnn_lstm", vocab_size: int = None,
                 encoder_params: Dict = None, decoder_params: Dict = None):
        super().__init__()
        encoder_params = {} if encoder_params is None else encoder_params
        decoder_params = {} if decoder_params is None else decoder_params
        vocab_size = 100 if vocab_size is None else vocab_size              # seq2seq.py:50-51
        embedding_dim = encoder_params.get("embedding_dim", 256)           # :54
        if model_type == "cnn_lstm":                                        # defaults of :58-67
            self.encoder = CNNEncoder(
                img_height=encoder_params.get("img_height", 50), img_width=encoder_params.get("img_width", 200),
                channels=encoder_params.get("channels", 1),
                conv_filters=encoder_params.get("conv_filters", [32, 64, 128]),
                kernel_size=encoder_params.get("kernel_size", 3), pool_size=encoder_params.get("pool_size", 2),
                padding=encoder_params.get("padding", "same"), embedding_dim=embedding_dim)
        elif model_type == "resnet_lstm":
            from .resnet_encoder import ResNetEncoder                       # defaults of :69-76
            self.encoder = ResNetEncoder(
                img_height=encoder_params.get("img_height", 224), img_width=encoder_params.get("img_width", 224),
                channels=encoder_params.get("channels", 3), model_name=encoder_params.get("model_name", "resnet50"),
                embedding_dim=embedding_dim, freeze_backbone=encoder_params.get("freeze_backbone", True))
        else:
            raise ValueError(f"Invalid model type: {model_type}. Expected 'cnn_lstm' or 'resnet_lstm'.")
        self.decoder = LSTMDecoder(                                         # defaults of :83-91
            vocab_size=vocab_size, embedding_dim=embedding_dim, hidden_dim=decoder_params.get("hidden_dim", 256),
            max_seq_length=decoder_params.get("max_seq_length", 150), lstm_layers=decoder_params.get("lstm_layers", 1),
            dropout=decoder_params.get("dropout", 0.1), attention=decoder_params.get("attention", False))
        self.model_type = model_type
        self.vocab_size = vocab_size

    # ---------------------------------------------------------------- training-mode forward
    def forward(self, images: torch.Tensor, target_sequences: torch.Tensor) -> torch.Tensor:
        """decoder(encoder(images), target_sequences[:, :-1]) -> (B,T,V)   (seq2seq.py:98-122)."""
        return self.decoder(self.encoder(images), target_sequences[:, :-1])

    # ---------------------------------------------------------------- inference
    def inference(self, image: torch.Tensor, start_token_id: int, end_token_id: int, max_length: int = None,
                  temperature: float = None, top_k: int = None, top_p: float = None, beam_size: int = None,
                  constraint=None):
        """seq2seq.py:124-190: List[int] for one image, List[List[int]] for a batch.  (A ResNet encoder runs the eval
        trunk its ``eval_precision`` selects; nothing here depends on which.)  ``constraint`` = a BracketTable or an
        ArgumentTable: the greedy search is the constrained one (LSTMDecoder.run_steps); beam search has no constrained
        form."""
        max_length = 150 if max_length is None else max_length
        temperature = 1.0 if temperature is None else temperature
        top_k = 0 if top_k is None else top_k
        top_p = 0.0 if top_p is None else top_p
        beam_size = 0 if beam_size is None else beam_size
        encoder_output = self.encoder(image)
        if encoder_output.dim() == 1:
            encoder_output = encoder_output.unsqueeze(0)
        if beam_size > 0:
            if constraint is not None:
                raise RuntimeError("img2latex_amd: inference(beam_size > 0) runs the grouped beam kernels, which carry no "
                                   "bracket constraint; use beam_search_nbest(..., constraint=table), nbest=1 for the "
                                   "single best, or beam_size=0")
            return self._beam_search(encoder_output, start_token_id, end_token_id, max_length, beam_size)
        return self._greedy_search(encoder_output, start_token_id, end_token_id, max_length, temperature, top_k, top_p,
                                   constraint=constraint)

    def greedy_ids(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int, max_length: int,
                   temperature: float = 1.0, stop: int = _lib.STOP_NONE, select: int = _lib.SELECT_LOGITS,
                   want_logits: bool = False, rows_per_workgroup: int = 0, flags: int = 0, prepared=None, resident=None,
                   constraint=None):
        """Device-side greedy loop; returns (ids (B,T) int32 on device, logits or None).  ``flags``:
        _lib.FLAG_DECODE_GROUP8 / _GROUP16 select the 8-member (vector ALUs) / 16-member (matrix cores) grouped kernels (the
        ones that share a CU with a conv workgroup);
        ``prepared`` / ``resident`` / ``constraint``: see LSTMDecoder.run_steps."""
        B = encoder_output.shape[0]
        key = (B, int(start_token_id), encoder_output.device)
        if getattr(self, "_tok0_key", None) != key:               # the START column: built once per batch shape
            self._tok0 = torch.full((B,), int(start_token_id), dtype=torch.int32, device=encoder_output.device)
            self._tok0_key = key
        tok0 = self._tok0
        ids, logits, _ = self.decoder.run_steps(encoder_output, max_length, tok0, temperature=temperature,
                                                select=select, stop=stop, end_id=end_token_id,
                                                want_logits=want_logits, rows_per_workgroup=rows_per_workgroup,
                                                flags=flags, prepared=prepared, resident=resident,
                                                constraint=constraint)
        return ids, logits

    def greedy_ids_host(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int, max_length: int,
                        temperature: float = 1.0, stop: int = _lib.STOP_NONE, select: int = _lib.SELECT_LOGITS,
                        flags: int = 0, constraint=None) -> torch.Tensor:
        """greedy_ids + the ONE device->host copy of the search, with the timeout fallback both callers
        (_greedy_search and Predictor.predict_batch_ids) share: the grouped kernel needs its 4 members resident
        together; on a GPU shared with other work (fewer than 32 free CUs) a bounded wait can expire (ids -3) ->
        run the row-per-workgroup HIP kernel, which needs no partner."""
        ids, _ = self.greedy_ids(encoder_output, start_token_id, end_token_id, max_length, temperature, stop=stop,
                                 select=select, flags=flags, constraint=constraint)
        ids = ids.cpu()
        if _lib.ids_timed_out(ids):
            warnings.warn("img2latex_amd: grouped decode timed out (GPU oversubscribed?); "
                          "re-running on the row-per-workgroup kernel", RuntimeWarning)
            ids, _ = self.greedy_ids(encoder_output, start_token_id, end_token_id, max_length, temperature, stop=stop,
                                     select=select, rows_per_workgroup=1, flags=flags, constraint=constraint)
            ids = _lib.check_ids(ids.cpu())
        return ids

    def _greedy_search(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int,
                       max_length: int, temperature: float, top_k: int, top_p: float, constraint=None):
        """seq2seq.py:192-232.  top_k / top_p are accepted and ignored, as in the reference.
        The loop stops when ALL rows emit END in the same step (:220); the kernel runs the
        rows independently, so that step is located in the ids afterwards."""
        B = encoder_output.shape[0]
        ids = self.greedy_ids_host(encoder_output, start_token_id, end_token_id, max_length, temperature,
                                   constraint=constraint).numpy()
        # host post-processing in numpy: one thread, no dispatch (torch would fan a 38 k-element compare out to every
        # host core: measured 10 ms per batch on the 16-core GPU box against 1.4 ms for the whole device path)
        all_end = (ids == end_token_id).all(axis=0)
        steps = int(all_end.argmax()) + 1 if bool(all_end.any()) else max_length
        full = np.empty((B, steps + 1), dtype=np.int64)
        full[:, 0] = start_token_id
        full[:, 1:] = ids[:, :steps]
        sequences = full.tolist()
        seq = sequences[0] if B == 1 else sequences
        if B == 1:                                                # :224-231
            if seq and seq[0] == start_token_id:
                seq = seq[1:]
            if end_token_id in seq:
                seq = seq[: seq.index(end_token_id)]
        return seq

    def _beam_search(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int,
                     max_length: int, beam_size: int):
        """seq2seq.py:234-298: batch size 1 only; a batch falls back to greedy (:244-247)."""
        if encoder_output.size(0) != 1:
            return self._greedy_search(encoder_output, start_token_id, end_token_id, max_length, 1.0, 0, 0.0)
        return self.beam_search_batch(encoder_output, start_token_id, end_token_id, max_length, beam_size)[0]

    def beam_search_batch(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int,
                          max_length: int, beam_size: int, return_scores: bool = False, flags: int = 0):
        """N independent batch-1 beam searches in one launch (BASELINE config 3): element j
        equals ``inference(image[j:j+1], beam_size=k)`` of the reference.  ``flags``: _lib.FLAG_NO_GROUP selects
        the one-workgroup-per-image kernel (the automatic fallback when the grouped kernel times out);
        _lib.FLAG_BEAM_BATCHED (here or in ``decoder.kernel_flags``) the step-batched matrix-core search
        (i2l_beam_decode_batched: the images x beam slots as rows of one batched step; nothing in it can time out)."""
        if beam_size > _lib.MAX_BEAM:
            raise NotImplementedError(f"img2latex_amd: beam_size <= {_lib.MAX_BEAM} (got {beam_size})")
        dec = self.decoder
        w, keep, enc = dec.prepare(encoder_output)
        n, dev = enc.shape[0], enc.device
        L = _lib.lib()
        if (int(flags) | int(dec.kernel_flags)) & _lib.FLAG_BEAM_BATCHED:
            # its scratch lives for this call only, on this stream
            nbytes = L.i2l_beam_batched_scratch_bytes(n, beam_size, dec.vocab_size, dec.hidden_dim, dec.lstm_layers,
                                                      max_length)
            if nbytes == 0:
                raise RuntimeError("img2latex_amd: dimensions not supported by the step-batched beam search")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            seq = torch.empty((n, max_length + 1), dtype=torch.int32, device=dev)
            ln = torch.empty((n,), dtype=torch.int32, device=dev)
            score = torch.empty((n,), dtype=torch.float64, device=dev)
            _lib.check(L.i2l_beam_decode_batched(ctypes.byref(w), dec._ws.data_ptr(), n, beam_size, max_length,
                                                 int(start_token_id), int(end_token_id), scratch.data_ptr(), nbytes,
                                                 seq.data_ptr(), ln.data_ptr(), score.data_ptr(),
                                                 int(flags) | int(dec.kernel_flags), _lib.stream_ptr()),
                       "beam_decode_batched")
            seq_h, lens = seq.cpu(), ln.cpu().tolist()
            del keep, scratch
            out = [row[:ln_j] for row, ln_j in zip(seq_h.tolist(), lens)]
            if return_scores:
                return out, score.cpu().tolist()
            return out
        nbytes = L.i2l_beam_workspace_bytes(n, beam_size, dec.hidden_dim, dec.lstm_layers, max_length)
        bws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        seq = torch.empty((n, max_length + 1), dtype=torch.int32, device=dev)
        ln = torch.empty((n,), dtype=torch.int32, device=dev)
        score = torch.empty((n,), dtype=torch.float64, device=dev)
        def launch(fl):
            _lib.check(L.i2l_beam_decode(ctypes.byref(w), dec._ws.data_ptr(), n, beam_size, max_length,
                                         int(start_token_id), int(end_token_id), bws.data_ptr(), nbytes,
                                         seq.data_ptr(), ln.data_ptr(), score.data_ptr(), int(fl), _lib.stream_ptr()),
                       "beam_decode")
        launch(flags | int(dec.kernel_flags))
        seq_h, ln_h = seq.cpu(), ln.cpu()
        if min(ln_h.tolist()) <= -3:
            # the grouped kernel needs its four workgroups resident together; on a GPU shared with other work a
            # poll can time out (len -3): run the one-workgroup-per-image kernel instead
            warnings.warn("img2latex_amd: grouped beam search timed out, re-running with one workgroup per image")
            launch(flags | int(dec.kernel_flags) | _lib.FLAG_NO_GROUP)
            seq_h, ln_h = seq.cpu(), ln.cpu()
        del keep
        lens = ln_h.tolist()                                   # one conversion each, then plain list slices
        out = [row[:ln_j] for row, ln_j in zip(seq_h.tolist(), lens)]
        if return_scores:
            return out, score.cpu().tolist()
        return out

    def beam_search_nbest(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int, max_length: int,
                          beam_size: int, nbest: Optional[int] = None, length_penalty: float = 0.0,
                          length_norm: Optional[Sequence[float]] = None, constraint=None) -> List[List[BeamHypothesis]]:
        """Per image the ``nbest`` (default ``beam_size``) best hypotheses of the beam search above, ranked by
        ``score / norm[n]``, n = tokens after START with END (``length_norm_table``): the completed beams in rank order,
        then, when the search ran out of steps, its final beams.  With ``nbest = 1`` and no normalisation, row 0 is
        ``beam_search_batch``'s result under _lib.FLAG_BEAM_BATCHED.  Always the step-batched search
        (i2l_beam_decode_nbest); dimensions it refuses raise RuntimeError.

        ``constraint``: a BracketTable (training/constraint.py) selects the well-formed search
        (i2l_beam_decode_nbest_constrained): a beam extends only by tokens its bracket state allows, with the log-probs
        renormalised over them, so every hypothesis nests its groups, ends on END (``finished`` is always True) and its
        score is its log-probability under the constrained model.  ``nbest=1`` gives the single best one.  An
        ArgumentTable is refused: the beam entry reads bracket class bytes and would misread its bytes."""
        if constraint is not None and constraint.kind != _lib.CONSTRAIN_BRACKETS:
            raise RuntimeError("img2latex_amd: the argument rules exist for the greedy and sampling decode only; the N-best "
                               "beam search takes a BracketTable (well_formed=True)")
        nbest = int(beam_size if nbest is None else nbest)
        table = length_norm_table(int(max_length), float(length_penalty), length_norm)
        dec = self.decoder
        w, keep, enc = dec.prepare(encoder_output)
        n, dev = enc.shape[0], enc.device
        L = _lib.lib()
        cls = None
        if constraint is not None:
            cls = dec._constraint_table(constraint, int(end_token_id), dev)
        size_query = L.i2l_beam_nbest_scratch_bytes if cls is None else L.i2l_beam_nbest_constrained_scratch_bytes
        nbytes = size_query(n, int(beam_size), nbest, dec.vocab_size, dec.hidden_dim, dec.lstm_layers, int(max_length))
        if nbytes == 0:
            raise RuntimeError(f"img2latex_amd: dimensions not supported by the n-best beam search (beam_size <= "
                               f"{_lib.MAX_BEAM}, nbest <= {_lib.MAX_NBEST}, vocabulary <= 2048)")
        norm = None if table is None else torch.tensor(table, dtype=torch.float64, device=dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # lives for this call only, on this stream
        seq = torch.empty((n, nbest, max_length + 1), dtype=torch.int32, device=dev)
        ln = torch.empty((n, nbest), dtype=torch.int32, device=dev)
        score = torch.empty((n, nbest), dtype=torch.float64, device=dev)
        key = torch.empty((n, nbest), dtype=torch.float64, device=dev)
        fin = torch.empty((n, nbest), dtype=torch.int32, device=dev)
        count = torch.empty((n,), dtype=torch.int32, device=dev)
        args = (ctypes.byref(w), dec._ws.data_ptr(), n, int(beam_size), nbest, int(max_length), int(start_token_id),
                int(end_token_id), _lib.ptr(norm), scratch.data_ptr(), nbytes, seq.data_ptr(), ln.data_ptr(), score.data_ptr(),
                key.data_ptr(), fin.data_ptr(), count.data_ptr(), 0)
        if cls is None:
            _lib.check(L.i2l_beam_decode_nbest(*args, _lib.stream_ptr()), "beam_decode_nbest")
        else:
            _lib.check(L.i2l_beam_decode_nbest_constrained(*args, cls.data_ptr(), _lib.stream_ptr()),
                       "beam_decode_nbest_constrained")
        seq_h, ln_h, sc_h = seq.cpu().tolist(), ln.cpu().tolist(), score.cpu().tolist()
        key_h, fin_h, cnt_h = key.cpu().tolist(), fin.cpu().tolist(), count.cpu().tolist()
        del keep, scratch, norm, cls
        return [[BeamHypothesis(seq_h[j][r][:ln_h[j][r]], sc_h[j][r], key_h[j][r], bool(fin_h[j][r]))
                 for r in range(cnt_h[j])] for j in range(n)]

    def sample_nbest(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int, max_length: int,
                     samples: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, seed: int = 0,
                     rank: str = "consensus", length_penalty: float = 0.0,
                     length_norm: Optional[Sequence[float]] = None, constraint=None) -> List[List[SampleHypothesis]]:
        """Per image ``samples`` (1 .. 16) top-k / top-p draws in ONE step-batched loop (i2l_sample_decode_multi: the
        draws of an image share its encoder row), each with its sequence log-probability, ranked on the device, best
        first.  ``rank="consensus"``: the minimum-Bayes-risk order -- ascending ``risk``, the summed Levenshtein distance
        to the image's other draws, then descending score; ``key`` is the risk.  ``rank="logprob"``: descending ``key =
        score / norm[n]`` with beam_search_nbest's table (``length_norm_table``).  Duplicates are kept: every image gets
        ``samples`` hypotheses.  ``constraint``: a BracketTable or an ArgumentTable -- every draw then keeps its rules
        and ends on END within ``max_length``; the score is the log-probability under the constrained model."""
        out = self.sample_multi_device(encoder_output, start_token_id, end_token_id, max_length, samples, temperature,
                                       top_k, top_p, seed, rank, length_penalty, length_norm, constraint)
        n = out["ids"].shape[0]
        ids, ln, fin, risk, score, key, order = (out[k] for k in ("ids", "len", "finished", "risk", "score", "key", "order"))
        ids_h, ln_h, fin_h, risk_h = ids.cpu().tolist(), ln.cpu().tolist(), fin.cpu().tolist(), risk.cpu().tolist()
        sc_h, key_h, ord_h = score.cpu().tolist(), key.cpu().tolist(), order.cpu().tolist()
        return [[SampleHypothesis(ids_h[j][s][:ln_h[j][s] - fin_h[j][s]], sc_h[j][s], key_h[j][s], risk_h[j][s],
                                  bool(fin_h[j][s]), s) for s in ord_h[j]] for j in range(n)]

    def sample_multi_device(self, encoder_output: torch.Tensor, start_token_id: int, end_token_id: int, max_length: int,
                            samples: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 0.0, seed: int = 0,
                            rank: str = "consensus", length_penalty: float = 0.0,
                            length_norm: Optional[Sequence[float]] = None, constraint=None) -> Dict[str, torch.Tensor]:
        """``sample_nbest``'s one call (i2l_sample_decode_multi) with its outputs left on the device, in SAMPLE order:
        "ids" (images, samples, max_length) int32, -1 behind END; "len", "finished", "risk" int32 and "score", "key"
        float64, (images, samples); "order" (images, samples) int32, the sample indices best first."""
        if rank not in RANKS:
            raise ValueError(f"img2latex_amd: unknown rank {rank!r}; expected one of {sorted(RANKS)}")
        samples, max_length = int(samples), int(max_length)
        if not 1 <= samples <= _lib.MAX_NBEST:
            raise ValueError(f"img2latex_amd: samples must be 1 .. {_lib.MAX_NBEST}, got {samples}")
        table = length_norm_table(max_length, float(length_penalty), length_norm)
        dec = self.decoder
        w, keep, enc = dec.prepare(encoder_output)
        n, dev = enc.shape[0], enc.device
        L = _lib.lib()
        kind, cls = _lib.CONSTRAIN_NONE, None
        if constraint is not None:
            kind, cls = constraint.kind, dec._constraint_table(constraint, int(end_token_id), dev)
        nbytes = L.i2l_sample_multi_scratch_bytes(n, samples, dec.vocab_size, dec.hidden_dim, dec.lstm_layers, max_length, kind)
        if nbytes == 0:
            raise RuntimeError(f"img2latex_amd: dimensions not supported by the consensus decode (samples <= "
                               f"{_lib.MAX_NBEST}, max_length <= {_lib.MAX_RANK_STEPS}, vocabulary <= 2048)")
        norm = None if table is None else torch.tensor(table, dtype=torch.float64, device=dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)      # lives for this call only, on this stream
        tok0 = torch.full((n,), int(start_token_id), dtype=torch.int32, device=dev)
        ids = torch.empty((n, samples, max_length), dtype=torch.int32, device=dev)
        ln, fin, risk, order = (torch.empty((n, samples), dtype=torch.int32, device=dev) for _ in range(4))
        score, key = (torch.empty((n, samples), dtype=torch.float64, device=dev) for _ in range(2))
        _lib.check(L.i2l_sample_decode_multi(ctypes.byref(w), dec._ws.data_ptr(), n, samples, max_length, tok0.data_ptr(),
                                             float(temperature), int(top_k), float(top_p), int(seed), int(end_token_id),
                                             kind, _lib.ptr(cls), RANKS[rank], _lib.ptr(norm), scratch.data_ptr(), nbytes,
                                             ids.data_ptr(), ln.data_ptr(), fin.data_ptr(), score.data_ptr(),
                                             risk.data_ptr(), key.data_ptr(), order.data_ptr(), 0, _lib.stream_ptr()),
                   "sample_decode_multi")
        del keep, scratch, norm, cls, tok0
        return {"ids": ids, "len": ln, "finished": fin, "risk": risk, "score": score, "key": key, "order": order}
