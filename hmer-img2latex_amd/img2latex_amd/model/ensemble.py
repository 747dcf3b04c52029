"""Ensemble decode (this package: the reference decodes with one model): several decoders of ONE vocabulary choose every
token together.  Each member runs its own step kernels on its own state along the shared tokens, one launch per step
combines their rows (csrc/ensemble_rules.inc.h) and the selection kernels pick from the combined row
(i2l_ensemble_decode, csrc/decode_ensemble.inc.h).

``EnsembleDecoder`` has ``LSTMDecoder``'s ``run_steps`` / ``sample_steps``; ``EnsembleModel`` answers what ``Predictor``'s
one-batch paths ask of a model -- ``encoder``, ``greedy_ids``, ``greedy_ids_host``, ``decoder.sample_steps``,
``inference`` -- so the predictor keeps one copy of its loops.  Beam search over an ensemble does not exist: refused.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch
import torch.nn as nn

from .. import _lib
from .lstm_decoder import LSTMDecoder
from .seq2seq_model import Seq2SeqModel

COMBINE = {"logprob": _lib.ENSEMBLE_LOGPROB, "prob": _lib.ENSEMBLE_PROB}


def combine_rule(combine) -> int:
    """"logprob" / "prob" (or the I2L_ENSEMBLE_* value) -> the C ABI's rule id; anything else raises ValueError."""
    if combine in COMBINE:
        return COMBINE[combine]
    if combine in COMBINE.values() and not isinstance(combine, bool):
        return int(combine)
    raise ValueError(f"img2latex_amd: unknown ensemble rule {combine!r}; expected 'logprob' or 'prob'")


def member_weights(weights, n: int):
    """``n`` finite weights > 0 as floats (None: equal ones); the library normalises them to sum 1."""
    if weights is None:
        return [1.0 / n] * n
    weights = [float(w) for w in weights]
    if len(weights) != n:
        raise ValueError(f"img2latex_amd: {len(weights)} ensemble weights for {n} members")
    if not all(math.isfinite(w) and w > 0 for w in weights):
        raise ValueError(f"img2latex_amd: ensemble weights must be finite and > 0, got {weights}")
    return weights


class EncoderOutputs(tuple):
    """The members' encoder outputs, one (B, E_m) tensor each, with the two attributes the decode loops read off a
    single model's encoder output: ``shape`` (of member 0: only the row count is shared) and ``device``."""

    @property
    def shape(self):
        return self[0].shape

    @property
    def device(self):
        return self[0].device


class EnsembleDecoder(nn.Module):
    """``run_steps`` / ``sample_steps`` with ``LSTMDecoder``'s signatures over ``decoders`` (1 .. 8 LSTMDecoders of one
    vocabulary; embedding, hidden size, layers and attention may differ).  ``encoder_output`` is a sequence, one tensor
    per member; ``hidden`` and the returned state are one (h, c) pair per member.  ``want_logits`` returns the COMBINED
    rows.  Every call is step-batched (i2l_ensemble_decode) whatever the flags say; with one member it is that member's
    ``run_steps(flags=FLAG_DECODE_BATCHED)`` / ``sample_steps`` bit for bit."""

    def __init__(self, decoders: Sequence[LSTMDecoder], weights=None, combine="logprob"):
        super().__init__()
        decoders = list(decoders)
        if not 1 <= len(decoders) <= _lib.MAX_ENSEMBLE:
            raise ValueError(f"img2latex_amd: an ensemble has 1 .. {_lib.MAX_ENSEMBLE} members, got {len(decoders)}")
        vocabs = [d.vocab_size for d in decoders]
        if len(set(vocabs)) != 1:
            raise ValueError(f"img2latex_amd: the members of an ensemble share one vocabulary, got sizes {vocabs}")
        self.members = nn.ModuleList(decoders)
        self.weights = member_weights(weights, len(decoders))
        self.combine = combine_rule(combine)
        self.vocab_size = vocabs[0]
        self.kernel_flags = 0

    def _call(self, encoder_output, steps, tok0, forced, hidden, temperature, select, top_k, top_p, seed, stop, end_id,
              want_ids, want_dist, want_state, flags, constraint, reuse_weight_images=True):
        n = len(self.members)
        encs = list(encoder_output)
        if len(encs) != n:
            raise RuntimeError(f"img2latex_amd: {len(encs)} encoder outputs for {n} ensemble members")
        if hidden is not None and len(hidden) != n:
            raise RuntimeError(f"img2latex_amd: {len(hidden)} hidden states for {n} ensemble members")
        rows = encs[0].shape[0]
        if any(e.shape[0] != rows for e in encs):
            raise RuntimeError("img2latex_amd: the members' encoder outputs differ in their row count")
        if constraint is not None and forced is not None:
            raise RuntimeError("img2latex_amd: a constrained decode takes no forced tokens")
        # every refusal of a member's own arguments comes before anything is launched
        states = [d._hidden(None if hidden is None else hidden[m], rows) for m, d in enumerate(self.members)]
        L = _lib.lib()
        records = (_lib.EnsembleMember * n)()
        keep = []
        for m, (d, enc) in enumerate(zip(self.members, encs)):
            w, k, enc = d.prepare(enc, reuse_weight_images)
            h = c = None
            if want_state:
                h = torch.empty((d.lstm_layers, rows, d.hidden_dim), dtype=torch.float32, device=enc.device)
                c = torch.empty_like(h)
            keep.append((w, k, enc, d._ws, h, c))
            records[m] = _lib.EnsembleMember(ctypes.pointer(w), d._ws.data_ptr(), _lib.ptr(states[m][0]),
                                             _lib.ptr(states[m][1]), _lib.ptr(h), _lib.ptr(c), self.weights[m])
        dev = encs[0].device
        tok0 = _lib.require_gpu(tok0, "tok0", torch.int32)
        if forced is not None:
            forced = _lib.require_gpu(forced, "forced", torch.int32)
            if forced.shape != (rows, steps):
                raise RuntimeError(f"forced tokens must be ({rows},{steps}), got {tuple(forced.shape)}")
        ids = torch.empty((rows, steps), dtype=torch.int32, device=dev) if want_ids else None
        dist = torch.empty((rows, steps, self.vocab_size), dtype=torch.float32, device=dev) if want_dist else None
        nbytes = L.i2l_ensemble_scratch_bytes(records, n, rows)
        if nbytes == 0:
            raise RuntimeError("img2latex_amd: decoder dimensions not supported by the step-batched decode")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cls = state = None
        kind = _lib.CONSTRAIN_NONE
        if constraint is not None:
            cls = self.members[0]._constraint_table(constraint, end_id, dev)
            state = torch.empty(constraint.state_bytes(rows), dtype=torch.uint8, device=dev)   # zeroed by the call
            kind = constraint.kind
        _lib.check(L.i2l_ensemble_decode(
            records, n, self.combine, rows, int(steps), tok0.data_ptr(), _lib.ptr(forced), float(temperature), int(select),
            int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stop), int(end_id), _lib.ptr(cls), kind,
            _lib.ptr(state), 0 if state is None else state.numel(), _lib.ptr(ids), _lib.ptr(dist), scratch.data_ptr(), nbytes,
            int(flags) | int(self.kernel_flags), _lib.stream_ptr()), "ensemble_decode")
        _lib.mark("decode")
        out_state = [(k[4], k[5]) for k in keep] if want_state else None
        del keep, scratch, state, records
        return ids, dist, out_state

    def run_steps(self, encoder_output, steps: int, tok0: torch.Tensor, forced: Optional[torch.Tensor] = None,
                  hidden=None, temperature: float = 1.0, select: int = _lib.SELECT_LOGITS, stop: int = _lib.STOP_NONE,
                  end_id: int = -1, want_ids: bool = True, want_logits: bool = False, want_state: bool = False,
                  reuse_weight_images: bool = True, rows_per_workgroup: int = 0, flags: int = 0, prepared=None,
                  resident=None, constraint=None):
        """``LSTMDecoder.run_steps`` for the ensemble: (ids, combined logits, [(h, c) per member]).  ``rows_per_workgroup``
        is accepted and ignored (the row kernel has no ensemble form); ``prepared`` / ``resident`` belong to the grouped
        pipeline, which stays single-model: refused."""
        if prepared is not None or resident is not None:
            raise RuntimeError("img2latex_amd: the ensemble decode takes no prepared workspace and no residency signal "
                               "(the look-ahead pipeline is single-model)")
        if select not in (_lib.SELECT_LOGITS, _lib.SELECT_SOFTMAX):
            raise RuntimeError("img2latex_amd: run_steps selects by arg max; sample_steps samples")
        return self._call(encoder_output, steps, tok0, forced, hidden, temperature, select, 0, 0.0, 0, stop, end_id,
                          want_ids, want_logits, want_state, flags, constraint, reuse_weight_images)

    def sample_steps(self, encoder_output, steps: int, tok0: torch.Tensor, temperature: float, top_k: int, top_p: float,
                     seed: int, stop: int = _lib.STOP_STICKY, end_id: int = -1, hidden=None, want_probs: bool = False,
                     flags: int = 0, want_state: bool = False, constraint=None):
        """``LSTMDecoder.sample_steps`` for the ensemble: (ids, probs or None), with ``want_state`` a third item, the
        members' (h, c) pairs."""
        ids, probs, state = self._call(encoder_output, steps, tok0, None, hidden, temperature, _lib.SELECT_SAMPLE, top_k,
                                       top_p, seed, stop, end_id, True, want_probs, want_state, flags, constraint)
        return (ids, probs, state) if want_state else (ids, probs)


class EnsembleEncoder(nn.Module):
    """The members' encoders as one callable: ``encoder(x)`` -> ``EncoderOutputs``.  The input geometry is the members'
    common one (``Predictor.from_checkpoints`` checks it)."""

    def __init__(self, encoders):
        super().__init__()
        self.members = nn.ModuleList(encoders)
        first = self.members[0]
        self.img_height, self.img_width, self.channels = first.img_height, first.img_width, first.channels

    def forward(self, x: torch.Tensor) -> EncoderOutputs:
        outs = []
        for enc in self.members:
            e = enc(x)
            outs.append(e.unsqueeze(0) if e.dim() == 1 else e)
        return EncoderOutputs(outs)


def _no_beam(what: str):
    raise RuntimeError(f"img2latex_amd: {what} over an ensemble does not exist (beam / N-best search is single-model); "
                       "use beam_size=0")


class EnsembleModel(nn.Module):
    """``models``: 1 .. 8 Seq2SeqModels of one vocabulary and one input geometry.  ``encoder(x)`` returns the members'
    encoder outputs; ``greedy_ids``, ``greedy_ids_host`` and the greedy ``inference`` are Seq2SeqModel's own loops over
    the ``EnsembleDecoder``.  ``inference(beam_size > 0)``, ``beam_search_batch`` and ``beam_search_nbest`` raise
    RuntimeError before anything is launched."""

    def __init__(self, models: Sequence[Seq2SeqModel], weights=None, combine="logprob"):
        super().__init__()
        models = list(models)
        self.models = nn.ModuleList(models)
        self.decoder = EnsembleDecoder([m.decoder for m in models], weights, combine)
        self.encoder = EnsembleEncoder([m.encoder for m in models])
        self.model_type = models[0].model_type
        self.vocab_size = self.decoder.vocab_size

    greedy_ids = Seq2SeqModel.greedy_ids
    greedy_ids_host = Seq2SeqModel.greedy_ids_host
    _greedy_search = Seq2SeqModel._greedy_search

    def inference(self, image: torch.Tensor, start_token_id: int, end_token_id: int, max_length: int = None,
                  temperature: float = None, top_k: int = None, top_p: float = None, beam_size: int = None,
                  constraint=None):
        """``Seq2SeqModel.inference`` with ``beam_size=0``: the greedy search of the ensemble."""
        if beam_size is not None and beam_size > 0:
            _no_beam(f"inference(beam_size={beam_size})")
        return self._greedy_search(self.encoder(image), start_token_id, end_token_id,
                                   150 if max_length is None else max_length, 1.0 if temperature is None else temperature,
                                   0 if top_k is None else top_k, 0.0 if top_p is None else top_p, constraint=constraint)

    def beam_search_batch(self, *args, **kwargs):
        _no_beam("beam_search_batch")

    def beam_search_nbest(self, *args, **kwargs):
        _no_beam("beam_search_nbest")

    def sample_nbest(self, *args, **kwargs):
        raise RuntimeError("img2latex_amd: sample_nbest over an ensemble does not exist (the consensus decode is "
                           "single-model)")
