// The serial rules of the beam search (reference seq2seq.py:249-297), stated once: what retires into `completed`, how
// the K x K candidates of a step are ranked, how a step ends, how a result is read back from the histories.  These are
// the decisions whose tie behaviour is pinned to the reference token for token: first on ties, strict >, stable order.
// Shared by beam_kernel<K> (decode.hip), the step-batched kernels (beam_batched.inc.h, beam_nbest.inc.h), the
// well-formed search's rules (beam_bracket_rules.inc.h) and two stand-alone host programs (beam_rules_host_main.cpp,
// beam_constrained_host_main.cpp) that host tests feed with exact score ties.
//
// Plain C++, no HIP: BEAM_HD is `__host__ __device__` under hipcc and empty elsewhere.  Every function is called by ONE
// thread; the arrays it gets are the caller's (LDS, registers or global memory on the device, vectors on the host).
//
// Slots: an image has K slots, the beams of a step are the slots 0 .. nb - 1 in rank order.  Histories: row t of
// tokhist / parhist ([T][K]) holds the token chosen for slot q at step t and the slot of step t - 1 it extends.
//
// Where a retiring beam goes is a "completed" sink with one member, put(im, score, t, q) -- (t, q) the history row and
// slot of the beam's last token, t = -1 the empty sequence:
//   BeamBest   keeps max(completed), first on ties (:286-290), in the image's record
//   BeamList   keeps the N best by key = score / norm[tokens after START], END included, in a sorted list
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BEAM_HD __host__ __device__ inline
#else
#define BEAM_HD inline
#endif

struct BeamImage {       // per image: `completed` reduced to its best entry, the beam count, the end of the search
    double best_c;
    int has_c, best_t, best_q;   // (with BeamList the entries are in the list and has_c counts them)
    int nb;              // beams in the slots 0 .. nb - 1
    int t_last;          // last history row written
    int done;            // one of the loop's two `break`s fired
};

struct NbestEntry {
    double key, score;
    int t, q;            // history row and slot of the last token; t = -1: the empty sequence (START == END)
};

BEAM_HD double nb_key(const double* norm, double score, int n) { return norm ? score / norm[n] : score; }

// A new entry goes in front of the first entry whose key is STRICTLY smaller; the last entry drops on overflow.  Beams
// retire in step order, then slot order, so this streaming insertion is the stable descending sort of the whole
// `completed` list cut to N.
BEAM_HD void nb_insert(NbestEntry* list, int& cnt, int N, double key, double score, int t, int q) {
    int pos = cnt;
    while (pos > 0 && list[pos - 1].key < key) --pos;
    if (pos >= N) return;
    const int last = cnt < N ? cnt : N - 1;
    for (int i = last; i > pos; --i) list[i] = list[i - 1];
    NbestEntry& e = list[pos];
    e.key = key; e.score = score; e.t = t; e.q = q;
    if (cnt < N) ++cnt;
}

struct BeamBest {
    BEAM_HD void put(BeamImage& im, double score, int t, int q) const {
        if (!im.has_c || score > im.best_c) { im.has_c = 1; im.best_c = score; im.best_t = t; im.best_q = q; }
    }
};

struct BeamList {
    NbestEntry* list;    // [N] of this image, the first im.has_c in use, keys non-increasing
    int N;
    const double* norm;  // [T + 1] length divisors, or null = all ones
    BEAM_HD void put(BeamImage& im, double score, int t, int q) const {
        int cnt = im.has_c;
        nb_insert(list, cnt, N, nb_key(norm, score, t + 1), score, t, q);
        im.has_c = cnt;
    }
};

// (a) of step t: beams whose last token is END retire into `completed`, in slot order (:258-260); the live flags of
// all K slots; returns the live count (0: `if not candidates: break`, :276-277).
template <class Sink>
BEAM_HD int beam_retire(BeamImage& im, const Sink& completed, const int* last, const double* score, int* live, int K,
                        int end_id, int t) {
    int nl = 0;
    for (int q = 0; q < K; ++q) {
        int lv = 0;
        if (q < im.nb) {
            if (last[q] == end_id) completed.put(im, score[q], t - 1, q);
            else { lv = 1; ++nl; }
        }
        live[q] = lv;
    }
    return nl;
}

// The start of a search: the one beam [START] with score 0.0 in slot 0, then (a) of step 0 -- START == END retires it
// at once as the empty sequence and ends the search.
template <class Sink>
BEAM_HD void beam_start(BeamImage& im, const Sink& completed, double* score, int* last, int* live, int K, int start_id,
                        int end_id) {
    for (int q = 0; q < K; ++q) { score[q] = 0.0; last[q] = start_id; }
    im = BeamImage{};
    im.nb = 1; im.best_t = -1; im.t_last = -1;
    if (beam_retire(im, completed, last, score, live, K, end_id, 0) == 0) im.done = 1;
}

// (d) of a step: the candidates of the live slots in (slot, rank) order, fp64 score + logp, the stable descending
// selection of K by K rounds of strict > (:268-280).  topv / topi: [K][K], the top K log-probs of each live slot's row,
// descending, and their tokens.  Writes the new beams' parent slots, tokens and scores, the step's two history rows
// and zeroes in the slots nnew .. K - 1; returns nnew.  K * K <= 64.
// ncand: [K], how many of its K entries live slot s really has, 0 .. K (the bracket-constrained search,
// beam_bracket_rules.inc.h: a slot may extend by fewer than K columns); entries j >= ncand[s] are never read and
// nnew = min(K, sum over the live slots of ncand[s]).  Null: K for every slot, the unconstrained search.
BEAM_HD int beam_rank(const int* live, const double* score, const float* topv, const int* topi, int K, const int* ncand,
                      int* npar, int* ntok, double* nscore, int32_t* tokrow, int32_t* parrow) {
    int nlive = 0, counted = 0;
    for (int q = 0; q < K; ++q) {
        nlive += live[q];
        if (ncand && live[q]) counted += ncand[q];
    }
    const int total = ncand ? counted : nlive * K;       // a null count folds to the arithmetic of the unconstrained search
    const int nnew = total < K ? total : K;
    unsigned long long used = 0ull;                      // candidate flags; an entry a slot does not have counts as used,
    if (ncand)                                           // so the rounds below keep their constant bounds
        for (int s0 = 0; s0 < K; ++s0) {
            if (!live[s0]) continue;
            for (int j = ncand[s0]; j < K; ++j) used |= 1ull << (s0 * K + j);
        }
    for (int q = 0; q < nnew; ++q) {
        double bs = 0.0;
        int bc = -1;
        for (int s0 = 0; s0 < K; ++s0) {
            if (!live[s0]) continue;
            for (int j = 0; j < K; ++j) {
                const int c = s0 * K + j;
                if ((used >> c) & 1ull) continue;
                const double sc = score[s0] + (double)topv[c];
                if (bc < 0 || sc > bs) { bs = sc; bc = c; }
            }
        }
        used |= 1ull << bc;
        npar[q] = bc / K;
        ntok[q] = topi[bc];
        nscore[q] = bs;
        tokrow[q] = topi[bc];
        parrow[q] = bc / K;
    }
    for (int q = nnew; q < K; ++q) { npar[q] = 0; ntok[q] = 0; nscore[q] = 0.0; }
    return nnew;
}

// (f), the ending of step t: the slots take the new scores and last tokens; all nnew beams ended --
// completed.extend(beams); break (:282-284); else (a) of step t + 1 when there is one.  Sets im.done.
template <class Sink>
BEAM_HD void beam_step_end(BeamImage& im, const Sink& completed, int nnew, const int* ntok, const double* nscore,
                           double* score, int* last, int* live, int K, int end_id, int t, int T) {
    bool all_end = true;
    for (int q = 0; q < K; ++q) {
        score[q] = nscore[q];
        last[q] = ntok[q];
        if (q < nnew && ntok[q] != end_id) all_end = false;
    }
    im.nb = nnew;
    im.t_last = t;
    if (all_end) {
        for (int q = 0; q < nnew; ++q) completed.put(im, nscore[q], t, q);
        im.done = 1;
    } else if (t + 1 < T) {
        if (beam_retire(im, completed, ntok, nscore, live, K, end_id, t + 1) == 0) im.done = 1;
    }
}

// Result: the beam whose last token is slot q of history row t, walked back to step 0 into out[0 .. T]: START is not
// in the histories, the sequence is cut at the first END and padded with -1 (:291-297).  Returns its length.
BEAM_HD int beam_backtrack(const int32_t* tokhist, const int32_t* parhist, int K, int t, int q, int end_id, int T,
                           int32_t* out) {
    const int n = t + 1;                                 // tokens after START
    for (int pos = t; pos >= 0; --pos) {
        out[pos] = tokhist[(size_t)pos * K + q];
        q = parhist[(size_t)pos * K + q];
    }
    int len = n;
    for (int i = 0; i < n; ++i)
        if (out[i] == end_id) { len = i; break; }
    for (int i = len; i < T + 1; ++i) out[i] = -1;
    return len;
}

// The result with BeamBest: max(completed) else beams[0] (:286-290).  score: the slots' scores after the last step.
BEAM_HD int beam_best_result(const BeamImage& im, const double* score, const int32_t* tokhist, const int32_t* parhist,
                             int K, int end_id, int T, int32_t* out, double* score_out) {
    *score_out = im.has_c ? im.best_c : score[0];
    return beam_backtrack(tokhist, parhist, K, im.has_c ? im.best_t : im.t_last, im.has_c ? im.best_q : 0, end_id, T, out);
}

// The result with BeamList, row by row.  The list's entries come first.  An image that was still searching after the
// last step (neither `break` fired) fills further rows from its final slots in slot order -- all of them have n = T, and
// x / norm[T] is monotone in x, so slot order (raw score, descending, stable) is their stable key order.  Such a row is
// finished when its last token is END: the reference never retires a beam that ends at the very last step.
BEAM_HD int beam_list_count(const BeamImage& im, int N) {
    const int all = im.has_c + (im.done ? 0 : im.nb);
    return all < N ? all : N;
}

struct NbestRow {
    double score, key;   // -inf in a row past the count
    int len, finished;   // -1, 0 there, and out all -1
};

// score / last: the slots' scores and last tokens after the last step
BEAM_HD NbestRow beam_list_row(const BeamImage& im, const BeamList& l, int row, const double* score, const int* last,
                               const int32_t* tokhist, const int32_t* parhist, int K, int end_id, int T, int32_t* out) {
    NbestRow r{-INFINITY, -INFINITY, -1, 0};
    int t, q;
    if (row < im.has_c) {
        const NbestEntry e = l.list[row];
        t = e.t; q = e.q; r.score = e.score; r.key = e.key; r.finished = 1;
    } else if (row < beam_list_count(im, l.N)) {
        t = im.t_last; q = row - im.has_c;
        r.score = score[q]; r.key = nb_key(l.norm, r.score, t + 1); r.finished = last[q] == end_id;
    } else {
        for (int i = 0; i < T + 1; ++i) out[i] = -1;
        return r;
    }
    r.len = beam_backtrack(tokhist, parhist, K, t, q, end_id, T, out);
    return r;
}
