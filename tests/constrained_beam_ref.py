"""The well-formed N-best beam search, restated: the loop of nbest_ref.search -- candidates from every live beam, scores
accumulated in Python floats, the stable descending sort by raw score keeping k, ended beams moving to ``completed`` on
the next iteration in slot order, both ``break``s -- with the bracket constraint inside (csrc/beam_bracket_rules.inc.h):

    state       every beam carries a BracketState; a new beam has a copy of its parent's, advanced by its token
    mask        a live beam at step t may extend by the columns ``table.allowed(state, end, max_length - t - 1)``; the
                others are set to -inf BEFORE log_softmax, so the log-probs are renormalised over the allowed columns
    candidates  the top ``min(k, #allowed)`` allowed columns of that row, descending, the lower index first on ties
                (``BracketTable.candidates``); a beam without one gets ``(end, 0.0)``

The model is a hook: ``row_logp(t, tokens, hidden) -> (row, hidden)`` returns the 1-D row of logits (``softmax=True``) or
of log-probs that are taken as they are (``softmax=False``) of a beam whose tokens, START included, are ``tokens``.  The
GPU test plugs in img2latex_oracle.decode_step, the host test a table.  ``table=None`` is the all-allowing policy: the
loop of nbest_ref.search itself.  The ending is nbest_ref.rank, unchanged."""
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

import img2latex_oracle as O
from img2latex_amd.training.constraint import BracketState
from nbest_ref import Search, rank  # noqa: F401  (the ending, for the callers)


def oracle_rows(sd, cfg: Dict, enc: torch.Tensor) -> Callable:
    """The hook of the oracle's decoder for ONE image: the logits of the step after ``tokens[-1]``."""
    assert enc.shape[0] == 1

    def row_logp(t, tokens, hidden):
        out, hid = O.decode_step(sd, cfg, enc, torch.tensor([[tokens[-1]]], dtype=torch.long, device=enc.device), hidden)
        return out.squeeze(1).squeeze(0), hid
    return row_logp


def search(row_logp: Callable, table, start_id: int, end_id: int, max_length: int, beam_size: int, softmax: bool = True,
           trace: Optional[List[dict]] = None) -> Search:
    """One image.  ``trace`` receives per step the new beams' tokens, parent slots, scores and states, and the candidate
    count of every slot the step found (0: not live)."""
    beams = [dict(tokens=[start_id], hidden=None, score=0.0, state=BracketState())]
    completed = []
    gap = float("inf")
    ran_out = True
    for t in range(max_length):
        cands, counts = [], []
        for slot, bm in enumerate(beams):
            if bm["tokens"][-1] == end_id:
                completed.append(bm)
                counts.append(0)
                continue
            row, hid = row_logp(t, bm["tokens"], bm["hidden"])
            if table is None:
                logp = torch.log_softmax(row, dim=-1) if softmax else row
                tv, ti = torch.sort(logp, descending=True, stable=True)
                picks = list(zip(ti[:beam_size].tolist(), tv[:beam_size].tolist()))
            else:
                rem = max_length - t - 1
                mask = torch.from_numpy(table.allowed(bm["state"], end_id, rem).astype(bool)).to(row.device)
                x = row.masked_fill(~mask, float("-inf"))
                logp = torch.log_softmax(x, dim=-1) if softmax else x
                picks = table.candidates(bm["state"], logp.cpu().numpy(), end_id, rem, beam_size)
            counts.append(len(picks))
            for ix, lp in picks:
                cands.append(dict(tokens=bm["tokens"] + [ix], hidden=hid, score=bm["score"] + lp, parent=slot))
        if not cands:
            ran_out = False
            break
        cands = sorted(cands, key=lambda b: b["score"], reverse=True)
        sc = [c["score"] for c in cands[:beam_size + 1]]
        gap = min([gap] + [a - b for a, b in zip(sc[:-1], sc[1:])])
        new = cands[:beam_size]
        for b in new:
            b["state"] = beams[b["parent"]]["state"].copy()
            if table is not None:
                table.advance(b["state"], b["tokens"][-1], end_id)
        beams = new
        if trace is not None:
            trace.append(dict(tokens=[b["tokens"][-1] for b in beams], parents=[b["parent"] for b in beams],
                              scores=[b["score"] for b in beams], states=[b["state"].copy() for b in beams], counts=counts))
        if all(b["tokens"][-1] == end_id for b in beams):
            completed.extend(beams)
            ran_out = False
            break
    pair = lambda b: (list(b["tokens"]), b["score"])                            # noqa: E731
    return Search([pair(b) for b in completed], [pair(b) for b in beams], ran_out, gap)


def allowed_gap(row_logp: Callable, table, start_id: int, end_id: int, max_length: int) -> float:
    """The smallest difference between the two largest allowed logits at any step of the constrained GREEDY path
    (beam 1): below it the fp32 arg max may leave the float64 one."""
    state, tokens, hidden, gap = BracketState(), [start_id], None, float("inf")
    for t in range(max_length):
        row, hidden = row_logp(t, tokens, hidden)
        x = row.detach().cpu().numpy().astype(np.float64)
        mask = table.allowed(state, end_id, max_length - t - 1).astype(bool)
        top = np.sort(x[mask])[::-1]
        if top.size > 1:
            gap = min(gap, float(top[0] - top[1]))
        pick = int(np.flatnonzero(mask)[np.argmax(x[mask])]) if top.size else end_id
        table.advance(state, pick, end_id)
        tokens = tokens + [pick]
        if pick == end_id:
            break
    return gap
