// The rules of minimum-risk fine-tuning (i2l_risk_rows), stated once: how a draw and the gold formula are cut, what a
// draw's reward and advantage are, which coefficient and smoothing a sequence of the assembled batch carries, and what the
// assembled rows hold.  Shared by train_risk.hip (the device kernel) and a stand-alone host program
// (risk_rules_host_main.cpp) that a host test compares with the Python restatement (tests/risk_ref.py).
//
// Plain C++, no HIP: BR_HD is `__host__ __device__` under hipcc and empty elsewhere.  Every function is called by ONE
// thread; the arrays it gets are the caller's.
//
// One image has a gold row formulas[0, steps + 1) = [START, tokens ..., END, PAD ...] and `samples` draws of `steps` ids
// each, as i2l_sample_decode_multi leaves them (-1 behind END).
//
//   cut        draw: its ids before the first end_id, all `steps` of them if it has none (sample_rank_rules' sr_cut).
//              gold: formulas[1, steps + 1) before the first end_id OR pad_id.
//   distance   d: the Levenshtein distance of the two cut sequences, an integer.  A pad_id that the model itself sampled
//              before its END is a token like any other here: it counts in the distance and in the length.
//   reward     r = 1 - d / max(len_draw, len_gold), 1 when both are empty: training/metrics.py's _lev_similarity, the
//              figure `evaluate` reports.  ONE double division and one subtraction; rounded to fp32 once where stored.
//   advantage  leave-one-out: A[n] = r[n] - (sum over m != n of r[m], in index order) / (samples - 1), in double from the
//              double rewards, rounded once.  All draws equal: every advantage is 0 up to the rounding of that double sum
//              (exactly 0 for two draws, below samples x 2^-50 otherwise).
//   sequences  image-major, samples + 1 per image, steps + 1 tokens each:
//              gold    formulas' row as it stands          coefficient alpha, smoothing label_smoothing, part 0
//              draw n  [START, the draw through its END, PAD ...]
//                                                           coefficient (float)((1 - (double)alpha) A[n]) from the DOUBLE
//                                                           advantage, smoothing 0, part 1
//              Everything behind a draw's first END is PAD (the decode's -1 among it).  A sampled PAD before END stays in
//              the row, where the loss masks it exactly as it masks a gold PAD (target == pad_id), although it counted in
//              the distance.
#pragma once
#include "sample_rank_rules.inc.h"

#define RK_MAX_SAMPLES SR_MAX_SAMPLES   // I2L_MAX_NBEST
#define RK_MAX_STEPS SR_MAX_STEPS       // I2L_MAX_RANK_STEPS
#define RK_PART_GOLD 0
#define RK_PART_DRAW 1

// what i2l_risk_rows accepts besides its pointers: 0 ok, 1 a bad argument, 2 an unsupported dimension
BR_HD int rk_check(int images, int samples, int steps, float alpha, float label_smoothing) {
    if (images <= 0 || samples <= 0 || steps <= 0) return 1;
    if (!(alpha >= 0.f && alpha <= 1.f)) return 1;
    if (!(label_smoothing >= 0.f && label_smoothing < 1.f)) return 1;
    if (samples < 2 || samples > RK_MAX_SAMPLES || steps > RK_MAX_STEPS) return 2;
    return 0;
}

// number of gold tokens: index of the first end_id or pad_id in gold[0, steps), or steps; gold = formulas + 1
BR_HD int rk_gold_len(const int32_t* gold, int steps, int end_id, int pad_id) {
    int t = 0;
    while (t < steps && gold[t] != end_id && gold[t] != pad_id) ++t;
    return t;
}

BR_HD double rk_reward(int d, int len_draw, int len_gold) {
    const int longest = len_draw > len_gold ? len_draw : len_gold;
    if (longest == 0) return 1.0;
    return 1.0 - (double)d / (double)longest;
}

BR_HD double rk_advantage(const double* reward, int n, int samples) {
    double others = 0.0;
    for (int m = 0; m < samples; ++m)
        if (m != n) others += reward[m];
    return reward[n] - others / (double)(samples - 1);
}

BR_HD float rk_coef_gold(float alpha) { return alpha; }
BR_HD float rk_coef_draw(float alpha, double advantage) { return (float)((1.0 - (double)alpha) * advantage); }

// token t of a draw's assembled row, 0 <= t <= steps; first_end = sr_first_end(draw, steps, end_id)
BR_HD int32_t rk_draw_row_token(const int32_t* draw, int t, int first_end, int start_id, int pad_id) {
    if (t == 0) return start_id;
    return t - 1 <= first_end ? draw[t - 1] : pad_id;
}
