// The combination rule of the ensemble decode, stated once: how the logit rows of M decoders that read the same tokens
// become ONE row, "the ensemble's logits", which the selection kernels then treat exactly as they treat one model's.
// Shared by ensemble_combine_kernel (decode_ensemble.inc.h) and a stand-alone host program
// (ensemble_rules_host_main.cpp) that a host test compares with a numpy float64 restatement.
//
// Plain C++, no HIP: BR_HD is `__host__ __device__` under hipcc and empty elsewhere.
//
// Members m = 0 .. M-1, 1 <= M <= ENS_MAX (8), raw logit rows x_m[0, V) and weights w_m > 0 normalised to sum 1
// (ens_normalise: the caller's weights divided by their float64 sum; log w_m beside them).
//
//   lp_m[v] = x_m[v] - lse_m,   lse_m = max + log(sum exp(x_m - max)) over [0, V)      the member's log-probabilities
//   ENS_LOGPROB (the default)   y[v] = sum_m w_m lp_m[v]            a weighted geometric mean; the row is left unnormalised
//   ENS_PROB                    y[v] = log(sum_m w_m exp(lp_m[v]))  an arithmetic mean, evaluated as a log-sum-exp over
//                                                                  the members of log w_m + lp_m[v]
//
// The temperature is NOT applied here: y goes to the selection as one model's logits do, and the division by the
// temperature, I2L_SELECT_LOGITS / _SOFTMAX, the top-k / top-p sampling, the constraint masks, logits_out and probs_out
// all happen there, to y.
//
// lse_m is accumulated ONLINE, one pass: (mx, s) with s = sum exp(x - mx) over what has been seen, rescaled when the
// maximum moves (ens_accumulate); partial pairs of different lanes are brought to a common maximum (ens_rescale) and
// their sums added.  A row costs one exp per element and is read once for lse and once for y.  lse_m is never formed:
// the member keeps (max, log sum) and ens_logprob subtracts them one after the other.
//
// Corners:
//   a column is -inf in one member     lp_m[v] = -inf.  LOGPROB: y[v] = -inf (w_m > 0: one member's veto is final).
//                                      PROB: that member adds nothing and the other members decide; y[v] = -inf only when
//                                      every member has -inf there.  Never NaN: the log-sum-exp over members is taken
//                                      around the largest term, and "every term -inf" is answered before any subtraction.
//   every column of a member is -inf   its max is -inf and the member's row is all -inf (ens_logprob answers -inf for a
//                                      -inf logit without subtracting).  LOGPROB: y is all -inf and the selection's own
//                                      fallback applies (column 0, or the constraint's first allowed column).  PROB: the
//                                      member drops out, the others are NOT renormalised (its weight is lost mass).
//   M == 1                             there is no combination at all: the loop skips the combine launch and the
//                                      selection reads the member's own logits, so the call is the single-model entry
//                                      bit for bit.  (The rule itself with M == 1 gives y = lp_0, the normalised row; the
//                                      host program evaluates that, the decode never does.)
// A logit of +inf or NaN is outside the rule (no decoder with finite weights produces one).
#pragma once
#include <math.h>

#include "bracket_rules.inc.h"      // BR_HD

constexpr int ENS_MAX = 8;
constexpr int ENS_LOGPROB = 0, ENS_PROB = 1;

// one more logit into the running (max, sum exp(x - max)); starts from (-INFINITY, 0)
BR_HD void ens_accumulate(float& mx, float& s, float x) {
    if (x > mx) {
        s = s * expf(mx - x) + 1.f;      // mx == -inf: s is 0 and expf(-inf) is 0
        mx = x;
    } else if (x > -INFINITY) {
        s += expf(x - mx);
    }
}

// a partial sum taken around mx, restated around new_mx >= mx
BR_HD float ens_rescale(float mx, float s, float new_mx) { return mx > -INFINITY ? s * expf(mx - new_mx) : 0.f; }

// lp = x - lse with lse = mx + log(s), evaluated as (x - mx) - log(s): x - mx is exact or nearly so where it matters
// (near the maximum), while mx + log(s) rounded to fp32 first would cost half an ulp of |mx| -- 5e-4 at logits of -1e4
BR_HD float ens_logprob(float x, float mx, float log_s) { return x > -INFINITY ? (x - mx) - log_s : -INFINITY; }

// y[v] from the members' lp_m[v]; w and logw are ens_normalise's
template <int M>
BR_HD float ens_combine(const float* lp, const float* w, const float* logw, int rule) {
    if (rule == ENS_LOGPROB) {
        float y = 0.f;
#pragma unroll
        for (int m = 0; m < M; ++m) y += w[m] * lp[m];
        return y;
    }
    float a[M], top = -INFINITY;
#pragma unroll
    for (int m = 0; m < M; ++m) { a[m] = logw[m] + lp[m]; top = fmaxf(top, a[m]); }
    if (!(top > -INFINITY)) return -INFINITY;
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) s += expf(a[m] - top);
    return top + logf(s);
}

// host only: the caller's weights (each finite and > 0, checked by the caller) to sum 1, and their logs
inline void ens_normalise(const float* weight, int M, float* w, float* logw) {
    double sum = 0.0;
    for (int m = 0; m < M; ++m) sum += (double)weight[m];
    for (int m = 0; m < M; ++m) {
        const double q = (double)weight[m] / sum;
        w[m] = (float)q;
        logw[m] = (float)log(q);
    }
}

inline bool ens_weight_ok(float weight) { return weight > 0.f && weight <= 3.402823466e+38f; }   // NaN and inf fail
