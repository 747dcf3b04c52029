"""Evaluation metrics with the reference's names and results (img2latex/training/metrics.py), computed on the
device: the id sequences and the (B,T,V) logits stay in HBM, the kernels return the INTEGER statistics
(Levenshtein table corner, clipped n-gram matches, accuracy counts) and the few float64 operations per pair
that turn them into scores are written here exactly as the reference writes them.

``calculate_metrics`` / ``masked_accuracy`` / ``token_list_accuracy`` are drop-ins for the calls at
cli.py:495, trainer.py:391,526 and metrics.py:591-621.  No CPU fallback: inputs are uploaded if they are lists.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple, Union

import torch

from .. import _lib

Seqs = Union[Sequence[Sequence[int]], torch.Tensor]


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("img2latex_amd: the metrics kernels need the ROCm device; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _pack(seqs: Sequence[Sequence[int]], dev: torch.device, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Ragged id lists -> (padded (n, width) int32, lengths (n) int32) on the device."""
    import numpy as np
    n = len(seqs)
    ids = np.zeros((n, max(width, 1)), dtype=np.int32)
    lens = np.empty((n,), dtype=np.int32)
    for i, s in enumerate(seqs):
        if isinstance(s, torch.Tensor):
            s = s.tolist()
        lens[i] = len(s)
        if len(s):
            ids[i, : len(s)] = s
    return torch.from_numpy(ids).to(dev), torch.from_numpy(lens).to(dev)


def sequence_statistics(predictions: Sequence[Sequence[int]], targets: Sequence[Sequence[int]], n: int = 4,
                        pad_token_id: int = 0) -> Dict[str, torch.Tensor]:
    """One launch for the whole batch.  Returns host int tensors: lev (P), match (P,4), tla (P,2), gen_len, true_len."""
    assert len(predictions) == len(targets), "Predictions and targets must have the same length"
    pairs = len(predictions)
    if pairs == 0:
        z = torch.zeros((0,), dtype=torch.int32)
        return dict(lev=z, match=torch.zeros((0, 4), dtype=torch.int32), tla=torch.zeros((0, 2), dtype=torch.int32),
                    gen_len=z, true_len=z)
    dev = _device()
    width = max([len(s) for s in predictions] + [len(s) for s in targets] + [1])
    p_ids, p_len = _pack(predictions, dev, width)
    t_ids, t_len = _pack(targets, dev, width)
    return device_sequence_statistics(p_ids, p_len, t_ids, t_len, n, pad_token_id, _max_len=width)


def device_sequence_statistics(p_ids: torch.Tensor, p_len: torch.Tensor, t_ids: torch.Tensor, t_len: torch.Tensor,
                               n: int = 4, pad_token_id: int = 0, _max_len: int = None, defer: bool = False):
    """Same for id matrices that already live on the device ((P, W) int32 + lengths), e.g. the decode kernel's output.
    ``defer=True`` returns the statistics as ONE device tensor (P, 9) int32 = [lev | match x4 | tla x2 | gen_len |
    true_len] without touching the host (``unpack_statistics`` splits its host copy), so a caller can overlap the next
    batch's host work with this one's kernels."""
    for name, t in (("pred ids", p_ids), ("pred lengths", p_len), ("target ids", t_ids), ("target lengths", t_len)):
        _lib.require_gpu(t, name, torch.int32)
    pairs = p_ids.shape[0]
    if _max_len is None:                                             # one sync; the list entry point knows it already
        pm, tm = int(p_len.max()), int(t_len.max())
        if pm > p_ids.shape[1] or tm > t_ids.shape[1]:
            raise RuntimeError("sequence length exceeds the id matrix width")
        max_len = max(pm, tm, 0)
    else:
        max_len = int(_max_len)
    if p_ids.shape[1] < max_len or t_ids.shape[1] < max_len:        # the kernel indexes rows up to max_len
        pad = lambda m: torch.nn.functional.pad(m, (0, max_len - m.shape[1]))
        p_ids, t_ids = pad(p_ids).contiguous(), pad(t_ids).contiguous()
    dev = p_ids.device
    lev = torch.empty((pairs,), dtype=torch.int32, device=dev)
    match = torch.empty((pairs, 4), dtype=torch.int32, device=dev)
    tla = torch.empty((pairs, 2), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().i2l_sequence_metrics(
        p_ids.data_ptr(), p_len.data_ptr(), p_ids.stride(0), t_ids.data_ptr(), t_len.data_ptr(), t_ids.stride(0), pairs,
        max_len, int(n), int(pad_token_id), lev.data_ptr(), match.data_ptr(), tla.data_ptr(), _lib.stream_ptr()),
        "sequence_metrics")
    packed = torch.cat([lev[:, None], match, tla, p_len[:, None], t_len[:, None]], dim=1)
    return packed if defer else unpack_statistics(packed.cpu())


def unpack_statistics(packed_host: torch.Tensor) -> Dict[str, torch.Tensor]:
    """(P, 9) int32 host tensor of device_sequence_statistics(defer=True) -> the dict of the other entry points."""
    return dict(lev=packed_host[:, 0], match=packed_host[:, 1:5], tla=packed_host[:, 5:7], gen_len=packed_host[:, 7],
                true_len=packed_host[:, 8])


def _lev_similarity(raw_distance: int, rows: int, cols: int) -> float:
    """metrics.py:85-94."""
    max_length = max(rows, cols)
    if max_length == 0:
        return 1.0
    return 1.0 - (raw_distance / max_length)


def _bleu_from_counts(match: Sequence[int], gen_len: int, true_len: int, n: int) -> float:
    """BLEU-n from the kernel's clipped n-gram match counts (i2l_sequence_metrics).  Bit-identical to the
    reference's score (metrics.py:113-181) because the float64 operations run in the same order: each
    precision is ONE division match / (gen_len - g + 1); their logs are added left to right starting from
    0.0; one division by n; one exp; the brevity factor exp(1 - true_len / gen_len) multiplies from the left."""
    if min(gen_len, true_len) == 0:
        return 0.0
    log_sum = 0.0
    for g in range(1, n + 1):
        hits = int(match[g - 1]) if min(gen_len, true_len) >= g else 0
        if hits == 0:                       # a zero precision zeroes the geometric mean (also: too short for g-grams)
            return 0.0
        log_sum += math.log(hits / (gen_len - g + 1))
    score = math.exp(log_sum / n)
    if gen_len >= true_len:
        return score
    return math.exp(1.0 - true_len / gen_len) * score


def levenshtein_distance(sequence_one: List[int], sequence_two: List[int]) -> float:
    """Normalised Levenshtein similarity of one pair (metrics.py:49-94)."""
    st = sequence_statistics([sequence_one], [sequence_two])
    return _lev_similarity(int(st["lev"][0]), len(sequence_one), len(sequence_two))


def bleu_n_score(generated_sequence: List[int], true_sequence: List[int], n: int = None) -> float:
    """BLEU-n of one pair (metrics.py:97-181)."""
    n = 4 if n is None else n
    if n > 4:
        raise NotImplementedError("img2latex_amd: BLEU-n is built for n <= 4 (the reference calls it with 4)")
    st = sequence_statistics([generated_sequence], [true_sequence], n)
    return _bleu_from_counts(st["match"][0].tolist(), len(generated_sequence), len(true_sequence), n)


def calculate_metrics(predictions: List[List[int]], targets: List[List[int]]) -> Dict[str, float]:
    """metrics.py:184-223: mean BLEU-4 and mean Levenshtein similarity of a batch, one kernel launch."""
    assert len(predictions) == len(targets), "Predictions and targets must have the same length"
    num_sequences = len(predictions)
    return metrics_from_statistics(sequence_statistics(predictions, targets, 4))


def metrics_from_packed(packed_host: torch.Tensor) -> Dict[str, float]:
    """The float64 tail of calculate_metrics on the (P, >= 9) int32 host rows of device_sequence_statistics(defer=True), by
    the library's host helper (i2l_scores_from_statistics: the formulas below, operation by operation, without the
    interpreter: 0.5 ms -> 5 us per 256 pairs; ``metrics_from_statistics`` is the Python statement of the same thing)."""
    import ctypes
    if packed_host.dtype != torch.int32 or packed_host.dim() != 2 or packed_host.shape[1] < 9 or packed_host.stride(1) != 1:
        raise TypeError("packed statistics must be a (P, >= 9) int32 host tensor with contiguous rows")
    b, l = ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().i2l_scores_from_statistics(packed_host.data_ptr(), packed_host.shape[0], packed_host.stride(0), 4,
                                                     ctypes.byref(b), ctypes.byref(l)), "scores_from_statistics")
    return {"bleu": b.value, "levenshtein": l.value, "batch_size": int(packed_host.shape[0])}


def metrics_from_statistics(st: Dict[str, torch.Tensor]) -> Dict[str, float]:
    """The float64 tail of calculate_metrics on the kernel's integer statistics (host tensors)."""
    match, lev = st["match"].tolist(), st["lev"].tolist()
    gl, tl = st["gen_len"].tolist(), st["true_len"].tolist()
    num_sequences = len(lev)
    bleu_scores = [_bleu_from_counts(match[i], gl[i], tl[i], 4) for i in range(num_sequences)]
    mean_bleu = sum(bleu_scores) / num_sequences
    lev_similarities = [_lev_similarity(lev[i], gl[i], tl[i]) for i in range(num_sequences)]
    mean_lev = sum(lev_similarities) / num_sequences
    return {"bleu": mean_bleu, "levenshtein": mean_lev, "batch_size": num_sequences}


def token_list_accuracy(predictions: List[List[int]], targets: List[List[int]], pad_token_id: int) -> Tuple[int, int]:
    """metrics.py:241-277: (correct, non-pad) token counts over the common prefix length of every pair."""
    if len(predictions) == 0:
        return 0, 0
    k = min(len(predictions), len(targets))                     # zip() semantics
    st = sequence_statistics(predictions[:k], targets[:k], 1, pad_token_id)
    tla = st["tla"].to(torch.int64).sum(dim=0)
    return int(tla[0]), int(tla[1])


def masked_accuracy(logits: torch.Tensor, targets: torch.Tensor, pad_token_id: int) -> Tuple[int, int]:
    """metrics.py:226-238 without moving the (B,T,V) logits to the host: (correct, total) over non-pad targets."""
    logits = _lib.require_gpu(logits.detach(), "logits").contiguous()
    targets = targets.detach()
    if not targets.is_cuda:
        targets = targets.to(logits.device)
    targets = targets.to(torch.int64).contiguous()
    V = logits.shape[-1]
    rows = logits.numel() // V
    if targets.numel() != rows:
        raise RuntimeError(f"targets must have {rows} elements, got {targets.numel()}")
    out = torch.empty((2,), dtype=torch.int64, device=logits.device)
    _lib.check(_lib.lib().i2l_masked_accuracy(logits.data_ptr(), targets.data_ptr(), rows, V, int(pad_token_id),
                                              out.data_ptr(), _lib.stream_ptr()), "masked_accuracy")
    c, t = out.cpu().tolist()
    return int(c), int(t)


# ------------------------------------------------------------------------------------------------ error analysis
# Which tokens the model gets wrong: the edit script of every (target, prediction) pair and the token confusion matrix of
# a split, on the device (csrc/edit_align_rules.inc.h states the rules; i2l_edit_alignment / i2l_confusion_margins /
# i2l_confusion_top).  The reference answers the question offline, per character string (analysis/errors.py).
OP_MATCH, OP_SUBSTITUTION, OP_DELETION, OP_INSERTION = 0, 1, 2, 3
KIND_SUBSTITUTIONS, KIND_DELETIONS, KIND_INSERTIONS, KIND_MATCHES = 1, 2, 4, 8     # I2L_CONFUSION_*
MAX_ALIGN_WIDTH, MAX_ALIGN_VOCAB, MAX_TOP = 1024, 2048, 1024
DEFAULT_DISTANCE_RANGES = [[0, 0], [1, 1], [2, 3], [4, "inf"]]                     # analysis/errors.py's defaults


def device_edit_alignment(p_ids: torch.Tensor, p_len: torch.Tensor, t_ids: torch.Tensor, t_len: torch.Tensor,
                          vocab_size: int, confusion: torch.Tensor = None, want_ops: bool = True,
                          want_script: bool = False) -> Dict[str, torch.Tensor]:
    """ONE launch over id matrices that live on the device ((P, W) int32 + lengths (P) int32, as
    ``device_sequence_statistics`` takes them); nothing is copied to the host.  Returns device tensors: "ops" (P, 4) int32
    = matches, substitutions, deletions, insertions (``want_ops``); "script" (P, Wp + Wt) uint8 and "script_len" (P) int32
    (``want_script``: 0 match, 1 substitution, 2 deletion, 3 insertion, forward order, the bytes behind script_len
    unwritten).  ``confusion``: a (V + 1, V + 1) int32 device tensor that the pairs' operations are ADDED to."""
    for name, t in (("pred ids", p_ids), ("pred lengths", p_len), ("target ids", t_ids), ("target lengths", t_len)):
        _lib.require_gpu(t, name, torch.int32)
    V = int(vocab_size)
    if p_ids.dim() != 2 or t_ids.dim() != 2 or p_ids.shape[0] != t_ids.shape[0] or p_len.numel() != p_ids.shape[0] or \
            t_len.numel() != t_ids.shape[0]:
        raise RuntimeError("id matrices must be (P, W) with P lengths each")
    if p_ids.stride(1) != 1 or t_ids.stride(1) != 1 or not p_len.is_contiguous() or not t_len.is_contiguous():
        raise RuntimeError("id rows and lengths must be contiguous")
    if confusion is not None:
        _lib.require_gpu(confusion, "confusion", torch.int32)
        if tuple(confusion.shape) != (V + 1, V + 1) or not confusion.is_contiguous():
            raise RuntimeError(f"confusion must be a contiguous ({V + 1}, {V + 1}) int32 tensor")
    if not (want_ops or want_script or confusion is not None):
        raise ValueError("nothing asked for: want_ops, want_script or a confusion matrix")
    pairs, dev = p_ids.shape[0], p_ids.device
    out: Dict[str, torch.Tensor] = {}
    if pairs == 0:
        if want_ops:
            out["ops"] = torch.zeros((0, 4), dtype=torch.int32, device=dev)
        if want_script:
            out["script"] = torch.zeros((0, p_ids.shape[1] + t_ids.shape[1]), dtype=torch.uint8, device=dev)
            out["script_len"] = torch.zeros((0,), dtype=torch.int32, device=dev)
        return out
    # a zero-width matrix holds nothing to read: one column of filler keeps the strides positive
    if p_ids.shape[1] == 0:
        p_ids = torch.zeros((pairs, 1), dtype=torch.int32, device=dev)
    if t_ids.shape[1] == 0:
        t_ids = torch.zeros((pairs, 1), dtype=torch.int32, device=dev)
    wp, wt = p_ids.shape[1], t_ids.shape[1]
    if p_ids.stride(0) != wp:
        p_ids = p_ids.contiguous()
    if t_ids.stride(0) != wt:
        t_ids = t_ids.contiguous()
    L = _lib.lib()
    need = L.i2l_edit_alignment_scratch_bytes(pairs, wp, wt)
    scratch = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
    if want_ops:
        out["ops"] = torch.empty((pairs, 4), dtype=torch.int32, device=dev)
    if want_script:
        out["script"] = torch.empty((pairs, wp + wt), dtype=torch.uint8, device=dev)
        out["script_len"] = torch.empty((pairs,), dtype=torch.int32, device=dev)
    _lib.check(L.i2l_edit_alignment(p_ids.data_ptr(), p_len.data_ptr(), wp, t_ids.data_ptr(), t_len.data_ptr(), wt, pairs, V,
                                    _lib.ptr(scratch), need, _lib.ptr(out.get("ops")), _lib.ptr(out.get("script")),
                                    _lib.ptr(out.get("script_len")), _lib.ptr(confusion), _lib.stream_ptr()),
               "edit_alignment")
    return out


def edit_alignment(predictions: Sequence[Sequence[int]], targets: Sequence[Sequence[int]], vocab_size: int,
                   confusion: torch.Tensor = None, want_ops: bool = True, want_script: bool = False):
    """``device_edit_alignment`` for ragged id lists (uploaded, as ``sequence_statistics`` uploads them).  Returns host
    values: "ops" (P, 4) int32 tensor; "script": a list of P lists of operation codes; "confusion": the device tensor the
    operations were added to (a fresh zeroed one when none was given)."""
    assert len(predictions) == len(targets), "Predictions and targets must have the same length"
    dev = _device()
    V = int(vocab_size)
    if confusion is None:
        confusion = torch.zeros((V + 1, V + 1), dtype=torch.int32, device=dev)
    out = {"confusion": confusion}
    if len(predictions) == 0:
        if want_ops:
            out["ops"] = torch.zeros((0, 4), dtype=torch.int32)
        if want_script:
            out["script"] = []
        return out
    width = max([len(s) for s in predictions] + [len(s) for s in targets] + [1])
    p_ids, p_len = _pack(predictions, dev, width)
    t_ids, t_len = _pack(targets, dev, width)
    if int(p_len.max()) > p_ids.shape[1] or int(t_len.max()) > t_ids.shape[1]:
        raise RuntimeError("sequence length exceeds the id matrix width")
    res = device_edit_alignment(p_ids, p_len, t_ids, t_len, V, confusion, want_ops, want_script)
    if want_ops:
        out["ops"] = res["ops"].cpu()
    if want_script:
        rows, lens = res["script"].cpu(), res["script_len"].cpu().tolist()
        out["script"] = [rows[i, :n].tolist() for i, n in enumerate(lens)]
    return out


def confusion_margins(confusion: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(row_total (V + 1), col_total (V + 1), diag (V)) int32 device tensors of a (V + 1, V + 1) confusion matrix."""
    _lib.require_gpu(confusion, "confusion", torch.int32)
    V = confusion.shape[0] - 1
    if confusion.dim() != 2 or confusion.shape[1] != V + 1 or V < 1 or not confusion.is_contiguous():
        raise RuntimeError("confusion must be a contiguous (V + 1, V + 1) int32 tensor")
    dev = confusion.device
    row, col = (torch.empty((V + 1,), dtype=torch.int32, device=dev) for _ in range(2))
    diag = torch.empty((V,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().i2l_confusion_margins(confusion.data_ptr(), V, row.data_ptr(), col.data_ptr(), diag.data_ptr(),
                                                _lib.stream_ptr()), "confusion_margins")
    return row, col, diag


def confusion_top(confusion: torch.Tensor, kinds: int, n: int) -> List[Tuple[int, int, int]]:
    """The up to ``n`` largest non-zero cells of the selected kinds (an OR of KIND_*) as host (row, col, count) tuples:
    count descending, then row, then column ascending.  One small copy of the listed cells."""
    _lib.require_gpu(confusion, "confusion", torch.int32)
    V = confusion.shape[0] - 1
    if confusion.dim() != 2 or confusion.shape[1] != V + 1 or V < 1 or not confusion.is_contiguous():
        raise RuntimeError("confusion must be a contiguous (V + 1, V + 1) int32 tensor")
    L, dev, n = _lib.lib(), confusion.device, int(n)
    need = L.i2l_confusion_top_scratch_bytes(V)
    scratch = torch.empty((max(need, 1),), dtype=torch.uint8, device=dev)
    out = torch.empty((3 * max(n, 1) + 1,), dtype=torch.int32, device=dev)       # rows | cols | counts | listed
    m = max(n, 1)
    _lib.check(L.i2l_confusion_top(confusion.data_ptr(), V, int(kinds), n, scratch.data_ptr(), need, out[:m].data_ptr(),
                                   out[m:2 * m].data_ptr(), out[2 * m:3 * m].data_ptr(), out[3 * m:].data_ptr(),
                                   _lib.stream_ptr()), "confusion_top")
    host = out.cpu()
    listed = int(host[3 * m])
    counts = host[2 * m:2 * m + listed].to(torch.int64) & 0xFFFFFFFF
    return list(zip(host[:listed].tolist(), host[m:m + listed].tolist(), counts.tolist()))


def distance_buckets(distances: Sequence[int], ranges=None) -> List[Dict]:
    """Counts of the pairs' edit distances per closed range [lo, hi] ("inf": no upper edge), analysis/errors.py's buckets
    on TOKEN distances."""
    ranges = DEFAULT_DISTANCE_RANGES if ranges is None else ranges
    total = len(distances)
    out = []
    for lo, hi in ranges:
        unbounded = isinstance(hi, str) or hi == float("inf")
        count = sum(1 for d in distances if d >= lo and (unbounded or d <= hi))
        out.append({"range": [int(lo), "inf" if unbounded else int(hi)], "count": count,
                    "fraction": count / total if total else 0.0})
    return out


class ErrorAnalysis:
    """The confusion matrix of a split and the report on it.

    ``update`` only enqueues i2l_edit_alignment on the current stream (``Predictor.evaluate_batch / evaluate_stream`` call it
    behind i2l_sequence_metrics when given ``errors=``); ``add_distances`` takes the per-pair edit distances that the packed
    statistics bring to the host anyway; ``report`` runs i2l_confusion_margins and i2l_confusion_top and copies their
    results -- the only device-to-host copies of the analysis.  Everything counted comes from those three entries: the
    host divides and packs."""

    def __init__(self, vocab_size: int, device=None):
        self.vocab_size = int(vocab_size)
        if not 1 <= self.vocab_size <= MAX_ALIGN_VOCAB:
            raise NotImplementedError(f"img2latex_amd: the error analysis is built for vocabularies of 1 .. {MAX_ALIGN_VOCAB} tokens")
        dev = _device() if device is None else torch.device(device)
        self.confusion = torch.zeros((self.vocab_size + 1, self.vocab_size + 1), dtype=torch.int32, device=dev)
        self.distances: List[int] = []

    def update(self, p_ids: torch.Tensor, p_len: torch.Tensor, t_ids: torch.Tensor, t_len: torch.Tensor) -> None:
        device_edit_alignment(p_ids, p_len, t_ids, t_len, self.vocab_size, self.confusion, want_ops=False)

    def retract(self, p_ids: torch.Tensor, p_len: torch.Tensor, t_ids: torch.Tensor, t_len: torch.Tensor) -> None:
        """Takes a batch out again that ``update`` had added (the evaluate chain's rare second run of a batch).  The
        subtraction is no atomic, so it waits for the updates in flight on other streams, and they for it."""
        once = torch.zeros_like(self.confusion)
        device_edit_alignment(p_ids, p_len, t_ids, t_len, self.vocab_size, once, want_ops=False)
        torch.cuda.synchronize(self.confusion.device)
        self.confusion -= once
        torch.cuda.synchronize(self.confusion.device)

    def add_distances(self, lev) -> None:
        self.distances.extend(int(d) for d in (lev.tolist() if hasattr(lev, "tolist") else lev))

    @staticmethod
    def ranges_from_config(config) -> Union[List, None]:
        """A checkpoint config's ``analysis.error_distance_ranges``, or None."""
        got = ((config or {}).get("analysis") or {}).get("error_distance_ranges")
        return [list(r) for r in got] if got else None

    def report(self, tokenizer=None, top: int = 20, ranges=None) -> Dict:
        V = self.vocab_size
        top = max(1, min(int(top), MAX_TOP))
        row_d, col_d, diag_d = confusion_margins(self.confusion)
        subs = confusion_top(self.confusion, KIND_SUBSTITUTIONS, top)
        dels = confusion_top(self.confusion, KIND_DELETIONS, top)
        ins = confusion_top(self.confusion, KIND_INSERTIONS, top)
        unsigned = lambda t: (t.cpu().to(torch.int64) & 0xFFFFFFFF).tolist()
        row, col, diag = unsigned(row_d), unsigned(col_d), unsigned(diag_d)
        return build_report(V, row, col, diag, subs, dels, ins, self.distances, tokenizer, ranges)


def build_report(V: int, row: Sequence[int], col: Sequence[int], diag: Sequence[int], subs, dels, ins, distances,
                 tokenizer=None, ranges=None) -> Dict:
    """The report dict from the device entries' results on the host: margins (row (V + 1), col (V + 1), diag (V)) and the
    three top lists of (row, col, count).  Sums of the margins, divisions, packing."""
    id_to_token = getattr(tokenizer, "id_to_token", None) if tokenizer is not None else None

    def name(i):
        if id_to_token is None:
            return int(i)
        return id_to_token.get(int(i), str(int(i))) if hasattr(id_to_token, "get") else id_to_token[int(i)]

    matches, deletions, insertions = sum(diag), col[V], row[V]
    substitutions = sum(row[:V]) - matches - deletions
    per_token = []
    for v in range(V):
        if row[v] or col[v]:
            per_token.append({"token": name(v), "id": v, "target_count": row[v], "predicted_count": col[v], "matches": diag[v],
                              "recall": diag[v] / row[v] if row[v] else None,
                              "precision": diag[v] / col[v] if col[v] else None})
    return {
        "level": "token",
        "vocab_size": V,
        "pairs": len(distances),
        "edit_distance_total": sum(distances),
        "distance_buckets": distance_buckets(distances, ranges),
        "operations": {"match": matches, "substitution": substitutions, "deletion": deletions, "insertion": insertions},
        "top_substitutions": [{"target": name(a), "predicted": name(b), "count": c} for a, b, c in subs],
        "top_deletions": [{"target": name(a), "count": c} for a, _, c in dels],
        "top_insertions": [{"predicted": name(b), "count": c} for _, b, c in ins],
        "per_token": per_token,
    }


def report_markdown(report: Dict) -> str:
    """error_analysis_report.md: the report dict as the sections of the reference's error report (analysis/errors.py),
    with TOKEN-level distances where the reference's are character-level."""
    lines = ["# Error analysis", "",
             f"{report['pairs']} (target, prediction) pairs, vocabulary of {report['vocab_size']} tokens.  Edit distances and "
             "operations are counted in tokens (the reference's offline report counts characters).  The `evaluate` command "
             "aligns the pairs its BLEU and Levenshtein figures are computed on, built as the reference builds them: the "
             "prediction without special tokens, the target without padding but with its START and END tokens, which "
             "therefore show up as two deletions per pair.", "",
             "## Edit-distance buckets", "", "| token edit distance | pairs | fraction |", "|---|---|---|"]
    for b in report["distance_buckets"]:
        lo, hi = b["range"]
        label = f"{lo}" if lo == hi else (f"{lo}+" if hi == "inf" else f"{lo}-{hi}")
        lines.append(f"| {label} | {b['count']} | {b['fraction']:.4f} |")
    lines += ["", "## Operation totals", "", "| operation | count |", "|---|---|"]
    lines += [f"| {k} | {v} |" for k, v in report["operations"].items()]
    cell = lambda t: "`" + str(t).replace("|", "\\|") + "`"
    lines += ["", "## Top substitutions", "", "| target | predicted | count |", "|---|---|---|"]
    lines += [f"| {cell(e['target'])} | {cell(e['predicted'])} | {e['count']} |" for e in report["top_substitutions"]]
    lines += ["", "## Top deleted tokens", "", "| target | count |", "|---|---|"]
    lines += [f"| {cell(e['target'])} | {e['count']} |" for e in report["top_deletions"]]
    lines += ["", "## Top inserted tokens", "", "| predicted | count |", "|---|---|"]
    lines += [f"| {cell(e['predicted'])} | {e['count']} |" for e in report["top_insertions"]]
    worst = sorted((t for t in report["per_token"] if t["recall"] is not None), key=lambda t: (t["recall"], -t["target_count"]))
    lines += ["", "## Lowest per-token recall", "", "| token | in targets | matches | recall | precision |", "|---|---|---|---|---|"]
    for t in worst[:len(report["top_substitutions"]) or 20]:
        prec = "-" if t["precision"] is None else f"{t['precision']:.4f}"
        lines.append(f"| {cell(t['token'])} | {t['target_count']} | {t['matches']} | {t['recall']:.4f} | {prec} |")
    return "\n".join(lines) + "\n"
