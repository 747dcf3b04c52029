// The rules of the consensus decode (i2l_sample_decode_multi, i2l_sample_rank), stated once: how a sample's token row
// is cut, what the distance of two samples is, what a sample's risk and key are, and in which order the samples of an
// image are reported.  Shared by sample_rank.inc.h (the device kernels) and a stand-alone host program
// (sample_rank_host_main.cpp) that a host test compares with the Python restatement (tests/sample_rank_ref.py).
//
// Plain C++, no HIP: BR_HD is `__host__ __device__` under hipcc and empty elsewhere.  Every function is called by ONE
// thread; the arrays it gets are the caller's.
//
//   cut       a sample's sequence is its tokens before the first end_id, all `steps` of them if it has none.  len is
//             the number of tokens after START, END included: the sequence length + 1 if the sample ended, else steps
//             (the N-best search's n of norm[n]).  finished is 1 iff the sample holds END.
//   distance  d(i, j): the Levenshtein distance of the cut sequences of samples i and j of one image, an integer.
//   risk      risk[i] = sum over j of d(i, j), int32; uniform weights -- the samples are draws from the model.
//   order     I2L_RANK_CONSENSUS: ascending risk, then descending score, then ascending sample index; key = (double)risk.
//             I2L_RANK_LOGPROB:   descending key = score / norm[len] (norm null: all ones; ONE IEEE division), then
//                                 ascending sample index.
//             Duplicates are kept: the count is always the number of samples, and equal samples pull the consensus
//             toward the mode.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BR_HD __host__ __device__ inline
#else
#define BR_HD inline
#endif

#define SR_RANK_CONSENSUS 0      // I2L_RANK_CONSENSUS
#define SR_RANK_LOGPROB 1        // I2L_RANK_LOGPROB
#define SR_MAX_SAMPLES 16        // I2L_MAX_NBEST
#define SR_MAX_STEPS 1024

struct SrCut {
    int n;           // tokens of the sequence
    int len;         // tokens after START, END included
    int finished;
};

// The cut from the place of the first end_id in the row (steps: there is none).
BR_HD SrCut sr_cut_at(int first_end, int steps) {
    const bool ended = first_end < steps;
    return SrCut{ended ? first_end : steps, ended ? first_end + 1 : steps, ended ? 1 : 0};
}

// index of the first end_id in ids[0, steps), or steps
BR_HD int sr_first_end(const int32_t* ids, int steps, int end_id) {
    int t = 0;
    while (t < steps && ids[t] != end_id) ++t;
    return t;
}

BR_HD SrCut sr_cut(const int32_t* ids, int steps, int end_id) { return sr_cut_at(sr_first_end(ids, steps, end_id), steps); }

// The Levenshtein distance of a[0, na) and b[0, nb) by the textbook table, one row at a time; row: nb + 1 ints of the
// caller.  The device takes Myers' bit-vector algorithm instead (sample_rank.inc.h): both are exact, so they agree.
BR_HD int sr_distance(const int32_t* a, int na, const int32_t* b, int nb, int* row) {
    for (int j = 0; j <= nb; ++j) row[j] = j;
    for (int i = 1; i <= na; ++i) {
        int diag = row[0];
        row[0] = i;
        for (int j = 1; j <= nb; ++j) {
            const int up = row[j], left = row[j - 1];
            int v = diag + (a[i - 1] == b[j - 1] ? 0 : 1);
            if (up + 1 < v) v = up + 1;
            if (left + 1 < v) v = left + 1;
            row[j] = v;
            diag = up;
        }
    }
    return row[nb];
}

BR_HD double sr_key(int rank, int risk, double score, int len, const double* norm) {
    if (rank == SR_RANK_CONSENSUS) return (double)risk;
    return norm ? score / norm[len] : score;
}

// is sample i reported before sample j (i != j)
BR_HD bool sr_before(int rank, int risk_i, double score_i, double key_i, int i, int risk_j, double score_j, double key_j,
                     int j) {
    if (rank == SR_RANK_CONSENSUS) {
        if (risk_i != risk_j) return risk_i < risk_j;
        if (score_i > score_j) return true;
        if (score_j > score_i) return false;
        return i < j;
    }
    if (key_i > key_j) return true;
    if (key_j > key_i) return false;
    return i < j;
}

// order[0, n): the sample indices best first -- a selection sort, so the result is a permutation whatever the scores hold
BR_HD void sr_order(int rank, int n, const int* risk, const double* score, const double* key, int32_t* order) {
    for (int i = 0; i < n; ++i) order[i] = i;
    for (int p = 0; p + 1 < n; ++p) {
        int b = p;
        for (int q = p + 1; q < n; ++q) {
            const int i = order[q], j = order[b];
            if (sr_before(rank, risk[i], score[i], key[i], i, risk[j], score[j], key[j], j)) b = q;
        }
        const int32_t best = order[b];
        for (int q = b; q > p; --q) order[q] = order[q - 1];      // stable: the others keep their places
        order[p] = best;
    }
}
