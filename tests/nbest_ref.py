"""The N-best, length-normalised ending of the beam search, restated on top of the oracle's decode step.

The search loop is img2latex_oracle.beam_search's (seq2seq.py:249-284), line for line: candidates from every live beam,
fp32 log-probs accumulated in Python floats, the stable descending sort by raw score keeping k, ended beams moving to
``completed`` on the next iteration in slot order, both ``break``s.  Only the ending differs:

    n(b)    tokens after START, END included
    key(b)  score(b) / norm[n(b)]            norm: max_length + 1 positive floats, None = all ones
    rows    ``completed`` sorted by key, descending and stable, cut to N; if the loop ran out of steps (neither
            ``break`` fired) and rows are left, the final beams follow, sorted by key, descending and stable in slot
            order.  Such a row is finished iff its last token is END; rows from ``completed`` always are.

With N = 1 and norm None, row 0 is ``max(completed)`` (first on ties) else ``beams[0]``: the oracle's result.
The search runs in the dtype of ``sd`` / ``enc``; ``search`` and ``rank`` are separate so that one search serves every
(N, norm) a test ranks it by."""
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

import img2latex_oracle as O


class Row(NamedTuple):
    tokens: List[int]
    score: float
    key: float
    finished: bool


def _strip(tokens, start_id, end_id):
    seq = tokens
    if seq and seq[0] == start_id:                                              # seq2seq.py:291-297
        seq = seq[1:]
    if end_id in seq:
        seq = seq[: seq.index(end_id)]
    return list(seq)


def _rel_gaps(keys):
    return [(a - b) / max(1.0, abs(a), abs(b)) for a, b in zip(keys[:-1], keys[1:])]


class Search(NamedTuple):
    """What the loop leaves: ``completed`` in retirement order and the final ``beams`` in slot order, each entry a
    (tokens with START, score) pair; whether neither ``break`` fired; the smallest candidate gap of any step."""
    completed: list
    beams: list
    ran_out: bool
    gap: float


def search(sd, cfg: Dict, enc: torch.Tensor, start_id: int, end_id: int, max_length: int, beam_size: int) -> Search:
    """The loop of img2latex_oracle.beam_search for ONE image (``enc`` has one row), every completed beam kept."""
    assert enc.shape[0] == 1
    beams = [dict(tokens=[start_id], hidden=None, score=0.0)]
    completed = []
    gap = float("inf")
    ran_out = True
    for _ in range(max_length):
        cands = []
        for bm in beams:
            last = bm["tokens"][-1]
            if last == end_id:
                completed.append(bm)
                continue
            out, hid = O.decode_step(sd, cfg, enc, torch.tensor([[last]], dtype=torch.long, device=enc.device), bm["hidden"])
            logp = torch.log_softmax(out.squeeze(1), dim=-1).squeeze(0)
            tv, ti = torch.topk(logp, beam_size)
            for lp, ix in zip(tv.tolist(), ti.tolist()):
                cands.append(dict(tokens=bm["tokens"] + [ix], hidden=hid, score=bm["score"] + lp))
        if not cands:
            ran_out = False
            break
        cands = sorted(cands, key=lambda b: b["score"], reverse=True)
        sc = [c["score"] for c in cands[:beam_size + 1]]
        gap = min([gap] + [a - b for a, b in zip(sc[:-1], sc[1:])])
        beams = cands[:beam_size]
        if all(b["tokens"][-1] == end_id for b in beams):
            completed.extend(beams)
            ran_out = False
            break
    pair = lambda b: (list(b["tokens"]), b["score"])                            # noqa: E731
    return Search([pair(b) for b in completed], [pair(b) for b in beams], ran_out, gap)


def rank(s: Search, start_id: int, end_id: int, max_length: int, nbest: int, norm: Optional[Sequence[float]] = None,
         stats: Optional[Dict] = None) -> List[Row]:
    """The ending: the rows of the image, ``len()`` of the result being its count.  ``stats`` receives "gap" (as
    img2latex_oracle.beam_search), "key_gap" (the smallest difference between neighbouring keys among the first N + 1
    ranked entries, relative to max(1, |key|); inf without neighbours), "completed" and "leftover" (how many entries of
    either kind were ranked) and "ran_out"."""
    if norm is not None:
        assert len(norm) == max_length + 1
    key_of = lambda b: b[1] / (1.0 if norm is None else float(norm[len(b[0]) - 1]))   # noqa: E731
    ranked = sorted(s.completed, key=key_of, reverse=True)                      # sorted() is stable
    left = sorted(s.beams, key=key_of, reverse=True) if s.ran_out else []
    rows = [Row(_strip(t, start_id, end_id), sc, key_of((t, sc)), True) for t, sc in ranked[:nbest]]
    for t, sc in left[:max(0, nbest - len(rows))]:
        rows.append(Row(_strip(t, start_id, end_id), sc, key_of((t, sc)), t[-1] == end_id))
    if stats is not None:
        kc = [key_of(b) for b in ranked][:nbest + 1]
        kl = [key_of(b) for b in left][:max(0, nbest + 1 - len(ranked))]
        stats.update(gap=s.gap, key_gap=min([float("inf")] + _rel_gaps(kc) + _rel_gaps(kl)), completed=len(ranked),
                     leftover=len(left), ran_out=s.ran_out)
    return rows


def beam_search_nbest(sd, cfg: Dict, enc: torch.Tensor, start_id: int, end_id: int, max_length: int, beam_size: int,
                      nbest: int, norm: Optional[Sequence[float]] = None, stats: Optional[Dict] = None) -> List[Row]:
    """``search`` then ``rank``: the rows of ONE image."""
    return rank(search(sd, cfg, enc, start_id, end_id, max_length, beam_size), start_id, end_id, max_length, nbest, norm,
                stats)
