// The distillation loss, stated once: how one row of the student's logits, the rows of M teachers that read the same
// tokens, and the data set's token become a loss and the gradient of that loss by the student's logits.  Shared by
// ce_distill_rows_kernel (train_distill.inc.h) and a stand-alone host program (distill_rules_host_main.cpp) that a host
// test compares with a numpy float64 restatement.  (This package: the reference trains on the data set's tokens alone.)
//
// Plain C++, no HIP: BR_HD is `__host__ __device__` under hipcc and empty elsewhere.
//
// Per row with target t != pad: student logits x[0, V), teacher rows z_m[0, V) with weights w_m (ens_normalise),
// combination rule, temperature tau > 0, hard weight alpha in [0, 1], label smoothing eps.
//
//   hard     = (1 - eps) (lse(x) - x[t]) + eps (lse(x) - mean_v x[v])       ce_rows_kernel's row loss, t clamped into
//                                                                           [0, V) as there
//   y[v]     = ens_combine over lp_m[v] = ens_logprob(z_m[v])               ensemble_rules.inc.h, unchanged: the
//                                                                           ensemble's row as the decode selects from it.
//                                                                           M == 1: no combination, y = z_0
//   q        = softmax(y / tau),  p = softmax(x / tau)                      the temperature is applied to y, not to the
//                                                                           members, as in the decode
//   soft     = tau^2 sum_v q[v] (log q[v] - log p[v])                       a term with q[v] == 0 is 0
//   loss     = alpha hard + (1 - alpha) soft
//   dlogits[v] = alpha (softmax(x)[v] - (1 - eps) [v == t] - eps / V) + (1 - alpha) tau (p[v] - q[v])
//
// dlogits is the gradient of the SUM over rows; the 1 / count of the mean is applied by i2l_grad_clip_adam_step.
//
// Every statistic is taken around its row's maximum: (max, sum exp((x - max) / tau)) accumulated online (dr_accumulate,
// ens_accumulate's scheme with a scale), partial pairs brought to a common maximum (dr_rescale).  A softmax is
// exp((x - max) / tau) / sum, never exp(x / tau - lse): lse rounded to fp32 costs half an ulp of |lse|, 5e-4 at logits of
// 1e4 (ce_rows_kernel and ens_logprob say the same).  log q - log p is ((y - ymax) / tau - log sq) - ((x - xmax) / tau -
// log sp): no logarithm of a quotient that may have underflowed, and exactly 0 in every column when y == x.
//
// Corners:
//   pad row (t == pad)        contributes exactly 0 to every sum and has exactly zero dlogits.  It is SELECTED, not
//                             multiplied: the kernel reads neither the student's nor the teachers' row, so whatever the
//                             teachers hold at pad positions (NaN included) reaches no output.
//   teacher logits            must be finite at kept rows.  -inf, +inf or NaN there is outside the rule.
//   NaN in the student's row  the row's sums and its dlogits are NaN (dr_accumulate lets a NaN into the sum, unlike
//                             ens_accumulate, which passes over what is not a number); the batch's sums are then NaN
//                             and i2l_grad_clip_adam_step skips the update.  +-inf in the student's row is outside
//                             the rule.
//   tau == 1, alpha == 1      no special case: alpha == 1 gives ce_rows_kernel's loss and gradient through the same
//                             expressions (0 * soft: soft is finite for finite teachers).
#pragma once
#include <math.h>
#include <stdint.h>

#include "ensemble_rules.inc.h"     // ens_accumulate, ens_rescale, ens_logprob, ens_combine, ens_normalise; BR_HD

struct DistillCoef {
    float tau, inv_tau, alpha, eps, base;     // base = eps / V
};

// host only: inv_tau and base are rounded once, here, for the kernel and the host program alike
inline DistillCoef dr_coef(float tau, float alpha, float eps, int V) {
    return DistillCoef{tau, 1.f / tau, alpha, eps, eps / (float)V};
}

// what a row's columns share once passes 1 and 2 are done
struct DistillRow {
    float xmx, s1, sp, log_sp;      // the student: max, sum exp(x - max), sum exp((x - max) / tau) and its log
    float ymx, sq, log_sq;          // the ensemble's row: max of y, sum exp((y - max) / tau) and its log
};

// one more value into the running (max, sum exp((x - max) scale)); starts from (-INFINITY, 0).  -inf is passed over
// (the columns beyond V); a NaN is NOT: it fails both comparisons' "greater" and lands in the sum.
BR_HD void dr_accumulate(float& mx, float& s, float x, float scale) {
    if (x > mx) {
        s = s * expf((mx - x) * scale) + 1.f;      // mx == -inf: s is 0 and expf(-inf) is 0
        mx = x;
    } else if (x != -INFINITY) {
        s += expf((x - mx) * scale);
    }
}

// a partial sum taken around mx, restated around new_mx >= mx; 0 for a partial sum that has seen nothing, NaN stays NaN
BR_HD float dr_rescale(float mx, float s, float new_mx, float scale) {
    return s == 0.f ? 0.f : s * expf((mx - new_mx) * scale);
}

// y[v] from the members' z_m[v]: ens_logprob and ens_combine, or z_0 itself for one teacher
template <int M>
BR_HD float dr_teacher(const float* z, const float* top, const float* log_s, const float* w, const float* logw, int rule) {
    if (M == 1) return z[0];
    float lp[M];
#pragma unroll
    for (int m = 0; m < M; ++m) lp[m] = ens_logprob(z[m], top[m], log_s[m]);
    return ens_combine<M>(lp, w, logw, rule);
}

// the row's hard loss: ce_rows_kernel's expressions, xt = x[clamped target], sx = sum_v x[v]
BR_HD float dr_hard(float xmx, float s1, float sx, float xt, int V, float eps) {
    const float lse = xmx + logf(s1);
    return (1.f - eps) * (lse - xt) + eps * (lse - sx / (float)V);
}

// column v: returns dlogits[v]; kl = q (log q - log p), the column's share of soft / tau^2
BR_HD float dr_column(float x, float y, bool is_target, const DistillRow& r, const DistillCoef& k, float& kl) {
    const float ax = (x - r.xmx) * k.inv_tau, ay = (y - r.ymx) * k.inv_tau;
    const float p = expf(ax) / r.sp, q = expf(ay) / r.sq;
    kl = q > 0.f ? q * ((ay - r.log_sq) - (ax - r.log_sp)) : 0.f;
    const float g = expf(x - r.xmx) / r.s1 - k.base - (is_target ? 1.f - k.eps : 0.f);
    return k.alpha * g + (1.f - k.alpha) * (k.tau * (p - q));
}

BR_HD float dr_soft(float kl_sum, float tau) { return tau * tau * kl_sum; }

BR_HD float dr_loss(float hard, float soft, float alpha) { return alpha * hard + (1.f - alpha) * soft; }

BR_HD int dr_clamp_target(int t, int V) { return t < 0 ? 0 : (t > V - 1 ? V - 1 : t); }

// host only: what the entry accepts besides pointers and sizes
inline bool dr_args_ok(int n, int combine, float temperature, float alpha) {
    return n >= 1 && n <= ENS_MAX && (combine == ENS_LOGPROB || combine == ENS_PROB) && temperature > 0.f &&
           temperature <= 3.402823466e+38f && alpha >= 0.f && alpha <= 1.f;      // NaN fails every comparison
}
