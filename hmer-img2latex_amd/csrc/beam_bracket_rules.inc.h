// The well-formed beam search: the bracket rules (bracket_rules.inc.h) inside the beam rules (beam_rules.inc.h), stated
// once.  Every hypothesis the search ever ranks is a prefix the bracket rules allow, so every hypothesis it returns
// nests and ends on END.  Shared by the step-batched kernels (beam_batched.inc.h under ConstrainRule,
// beam_constrained.inc.h) and a stand-alone host program (beam_constrained_host_main.cpp) that a host test compares with
// the Python restatement (training/constraint.py, tests/constrained_beam_ref.py) step by step.
//
// Plain C++, no HIP.  Every function is called by ONE thread.  What is new beside the two rule sets:
//
//   Policy       a live slot at step t of `steps`, with bracket state st, may extend by column v iff
//                br_allowed(st, v == end_id, cls[v], rem = steps - t - 1)                          (bb_may_extend)
//   Candidates   the slot's candidates are its top min(K, #allowed) allowed columns, descending by log-prob, the lower
//                index first on ties; beam_rank gets the count and never reads past it              (bb_candidates)
//   Log-probs    the log-softmax over the ALLOWED columns only: a forbidden column enters the softmax as -inf, the
//                constrained sampler's convention.  Scores are log-probabilities under the constrained model; a forced
//                closer or a forced END costs 0.  (The device's phase (c) renormalises; bb_candidates takes a row of
//                log-probs as it is.)
//   Fallback     no column allowed, or a selection round finds none (every allowed value left is -inf or NaN): the list
//                stops there, and an EMPTY list becomes the single candidate (end_id, 0.0f) -- as constraint_fallback, defined
//                but not well formed.  Only a malformed table, or a row without a finite allowed logit.  (bb_close_list)
//   Inheritance  new slot q has br_advance(copy of parent npar[q]'s state, ntok[q] == end_id, cls[ntok[q]]); the parents
//                are read from a copy taken before any slot is overwritten                            (bb_inherit)
//
// What follows, for a table as BracketTable builds them (every open kind has its closer) and finite logits:
//   - every live slot has at least one candidate: the closer of its innermost group (depth > 0) or END (depth 0) is
//     always allowed, because depth + 1 <= steps - t holds at t = 0 and every allowed pick keeps it;
//   - at step steps - 1 that bound leaves depth 0 and rem 0, so the ONLY candidate of every live slot is END;
//   - so all new beams of that step end, and the all-ended `break` of beam_step_end fires at the last step at the latest;
//   - so a constrained search never runs out of steps: every returned row comes from `completed`, has finished = 1 and
//     is well formed.
#pragma once
#include "beam_rules.inc.h"
#include "bracket_rules.inc.h"

BR_HD bool bb_may_extend(const BracketState& st, int v, int end_id, const uint8_t* cls, int steps, int t) {
    return br_allowed(st, v == end_id, cls[v], steps - t - 1);
}

// The end of a slot's list of n entries: an empty one becomes the fallback.  Returns the slot's candidate count, >= 1.
BR_HD int bb_close_list(int n, int end_id, float* topv, int* topi) {
    if (n > 0) return n;
    topv[0] = 0.0f;
    topi[0] = end_id;
    return 1;
}

// The candidates of one live slot from a row lp[0, V) of log-probs taken as they are: K rounds of strict > over the
// allowed columns not yet taken.  Writes topv / topi[0, count) and returns the count.
BR_HD int bb_candidates(const BracketState& st, const float* lp, const uint8_t* cls, int V, int K, int end_id, int steps,
                        int t, float* topv, int* topi) {
    int n = 0;
    for (; n < K; ++n) {
        float bv = -INFINITY;
        int bi = -1;
        for (int v = 0; v < V; ++v) {
            if (!bb_may_extend(st, v, end_id, cls, steps, t) || !(lp[v] > bv)) continue;
            bool taken = false;
            for (int j = 0; j < n; ++j) taken = taken || topi[j] == v;
            if (!taken) { bv = lp[v]; bi = v; }
        }
        if (bi < 0) break;
        topv[n] = bv;
        topi[n] = bi;
    }
    return bb_close_list(n, end_id, topv, topi);
}

// The state of a new slot: its parent's, from the copy `parents` of the step's states, advanced by its token.
BR_HD BracketState bb_inherit(const BracketState* parents, int par, int tok, int end_id, const uint8_t* cls) {
    BracketState s = parents[par];
    br_advance(s, tok == end_id, cls[tok]);
    return s;
}
