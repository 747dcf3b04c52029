"""The consensus decode's rules (csrc/sample_rank_rules.inc.h) restated in plain Python, and the float64 sequence score.

cut       a sample's sequence is its tokens before the first ``end_id`` (all ``steps`` without one); ``len`` counts the
          tokens after START with END: sequence length + 1 if it ended, else ``steps``; ``finished`` iff it holds END.
distance  the textbook Levenshtein table between two cut sequences (``levenshtein``; ``distance`` is the same table
          a row at a time in numpy, held to it by test_sample_rank_host.py).
risk      the sum of a sample's distances to every sample of its image (itself included: 0).
order     "consensus": ascending risk, then descending score, then ascending index; key = float(risk).
          "logprob":   descending key = score / norm[len] (norm None: the score itself), then ascending index.
"""
import functools

import numpy as np

CONSENSUS, LOGPROB = 0, 1


def cut(row, end_id):
    row = [int(v) for v in row]
    if end_id in row:
        n = row.index(end_id)
        return row[:n], n + 1, 1
    return row, len(row), 0


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
        prev = cur
    return prev[len(b)]


@functools.lru_cache(maxsize=None)
def _distance(a, b):
    """``levenshtein`` of two tuples, a whole table row per numpy operation: row[j] = min(up + 1, diagonal + cost) first,
    then the left neighbour's ``row[j - 1] + 1`` as a running minimum of row[j] - j.  Remembered, and asked for with
    a <= b only: the distance is symmetric."""
    if len(a) < 8 or len(b) < 8:
        return levenshtein(a, b)
    bb, idx = np.array(b), np.arange(len(b) + 1)
    prev = idx.copy()
    for i in range(1, len(a) + 1):
        cur = np.empty(len(b) + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (bb != a[i - 1]))
        prev = np.minimum.accumulate(cur - idx) + idx
    return int(prev[-1])


def distance(a, b):
    a, b = tuple(a), tuple(b)
    return _distance(a, b) if a <= b else _distance(b, a)


def rank_image(ids, end_id, score, rank, norm=None):
    """ids (samples, steps) ints, score (samples,) float64 -> dict of len, finished, risk (int lists), key (float64
    array), order (sample indices best first), dist (samples x samples)."""
    S = len(ids)
    cuts = [cut(r, end_id) for r in ids]
    dist = [[distance(cuts[i][0], cuts[j][0]) for j in range(S)] for i in range(S)]
    risk = [sum(r) for r in dist]
    score = np.asarray(score, dtype=np.float64)
    if rank == CONSENSUS:
        key = np.array([float(r) for r in risk], dtype=np.float64)

        def before(i, j):
            if risk[i] != risk[j]:
                return risk[i] < risk[j]
            if score[i] != score[j]:
                return score[i] > score[j]
            return i < j
    else:
        key = np.array([score[s] / np.float64(norm[cuts[s][1]]) if norm is not None else score[s] for s in range(S)],
                       dtype=np.float64)

        def before(i, j):
            if key[i] != key[j]:
                return key[i] > key[j]
            return i < j
    order = sorted(range(S), key=functools.cmp_to_key(lambda i, j: -1 if before(i, j) else 1))
    return dict(len=[c[1] for c in cuts], finished=[c[2] for c in cuts], risk=risk, key=key, order=order, dist=dist)


def rank_images(ids, end_id, score, rank, norm=None):
    """ids (images, samples, steps), score (images, samples) -> the per-image dicts stacked into arrays."""
    rows = [rank_image(ids[i], end_id, score[i], rank, norm) for i in range(len(ids))]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def sequence_scores(logits, ids, end_id, allowed=None):
    """The float64 log-probability of each row's tokens up to and including END: logits (rows, steps, V) of a
    teacher-forced replay of ``ids`` (rows, steps); allowed (rows, steps, V) bool or None: the columns the row's
    constraint allowed at each step (a forbidden column enters the softmax as -inf)."""
    x = np.asarray(logits, dtype=np.float64)
    if allowed is not None:
        x = np.where(allowed, x, -np.inf)
    m = x.max(axis=-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(x - m).sum(axis=-1))
    out = np.zeros(x.shape[0], dtype=np.float64)
    for r in range(x.shape[0]):
        for t in range(x.shape[1]):
            tok = int(ids[r][t])
            if tok < 0:
                break
            out[r] += x[r, t, tok] - lse[r, t]
            if tok == end_id:
                break
    return out
