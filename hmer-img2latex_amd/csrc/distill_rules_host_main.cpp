// The distillation loss (distill_rules.inc.h) as a stand-alone host program, so that a host test can hold it to a float64
// restatement -- one to eight teachers, both rules, rows of 1 to 1025 columns, temperatures on both sides of 1, logits
// scaled by 30, a logit of +1e4, teacher equal to student -- under the host sanitizers (-fsanitize=address,undefined) in
// a process of its own.  It holds no rule: the row is walked with the functions the kernel calls, in fp32 and in the
// kernel's partition -- dr_accumulate / ens_accumulate over a lane's columns, the lanes' pairs joined as the kernel joins
// them, dr_teacher per column, then dr_column.
//
//   distill_rules_host_main CASES OUT
//
// CASES: "DSTL", int32 count, then per case int32 M, V, rule, target; float32 tau, alpha, eps; float32 weight[M];
//        float32 x[V]; float32 z[M][V].  The row is a kept one: the pad selection is the kernel's.
// OUT per case: float32 hard, soft, loss; float32 dlogits[V].
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "distill_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// The kernel's partition of a row: 64 lanes, lane l holds columns l, l + 64, ...; per-lane partial results meet in a
// butterfly (wave_sum / wave_max: every level adds lane l and lane l ^ off).  A serial fp32 sum over 1025 columns would
// carry an error that grows with V and say nothing about the kernel's.
constexpr int LANES = 64;

static float wave_sum(const float (&part)[LANES]) {
    float v[LANES], t[LANES];
    memcpy(v, part, sizeof v);
    for (int off = LANES / 2; off > 0; off >>= 1) {
        for (int l = 0; l < LANES; ++l) t[l] = v[l] + v[l ^ off];
        memcpy(v, t, sizeof v);
    }
    return v[0];
}

static float wave_max(const float (&part)[LANES]) {
    float top = part[0];
    for (int l = 1; l < LANES; ++l) top = fmaxf(top, part[l]);
    return top;
}

// (max, sum exp((value(v) - max) scale)) of a row through the lanes: dr_accumulate per lane, dr_rescale, wave_sum
template <class F>
static void lane_max_sum(int V, float scale, F value, float& top, float& sum) {
    float mx[LANES], s[LANES];
    for (int l = 0; l < LANES; ++l) {
        mx[l] = -INFINITY; s[l] = 0.f;
        for (int v = l; v < V; v += LANES) dr_accumulate(mx[l], s[l], value(v), scale);
    }
    top = wave_max(mx);
    for (int l = 0; l < LANES; ++l) s[l] = dr_rescale(mx[l], s[l], top, scale);
    sum = wave_sum(s);
}

template <int M>
static void distill_row(const std::vector<float>& x, const std::vector<float>& z, int V, int target, const float* w,
                        const float* logw, int rule, const DistillCoef& k, float* head, std::vector<float>& d) {
    float top[M], log_s[M], part[LANES];
    for (int m = 0; m < M; ++m) {
        float mx[LANES], s[LANES];
        for (int l = 0; l < LANES; ++l) {
            mx[l] = -INFINITY; s[l] = 0.f;
            for (int v = l; v < V; v += LANES) ens_accumulate(mx[l], s[l], z[(size_t)m * V + v]);
        }
        top[m] = wave_max(mx);
        for (int l = 0; l < LANES; ++l) s[l] = ens_rescale(mx[l], s[l], top[m]);
        log_s[m] = logf(wave_sum(s));
    }
    DistillRow r;
    float same_max;
    lane_max_sum(V, 1.f, [&](int v) { return x[(size_t)v]; }, r.xmx, r.s1);
    lane_max_sum(V, k.inv_tau, [&](int v) { return x[(size_t)v]; }, same_max, r.sp);
    r.log_sp = logf(r.sp);
    for (int l = 0; l < LANES; ++l) {
        part[l] = 0.f;
        for (int v = l; v < V; v += LANES) part[l] += x[(size_t)v];
    }
    const float sx = wave_sum(part);
    std::vector<float> y((size_t)V);
    for (int v = 0; v < V; ++v) {
        float zc[M];
        for (int m = 0; m < M; ++m) zc[m] = z[(size_t)m * V + v];
        y[(size_t)v] = dr_teacher<M>(zc, top, log_s, w, logw, rule);
    }
    lane_max_sum(V, k.inv_tau, [&](int v) { return y[(size_t)v]; }, r.ymx, r.sq);
    r.log_sq = logf(r.sq);
    const int tg = dr_clamp_target(target, V);
    for (int l = 0; l < LANES; ++l) {
        part[l] = 0.f;
        for (int v = l; v < V; v += LANES) {
            float kl;
            d[(size_t)v] = dr_column(x[(size_t)v], y[(size_t)v], v == tg, r, k, kl);
            part[l] += kl;
        }
    }
    head[0] = dr_hard(r.xmx, r.s1, sx, x[(size_t)tg], V, k.eps);
    head[1] = dr_soft(wave_sum(part), k.tau);
    head[2] = dr_loss(head[0], head[1], k.alpha);
}

template <int M>
static bool dispatch(int m, const std::vector<float>& x, const std::vector<float>& z, int V, int target, const float* w,
                     const float* logw, int rule, const DistillCoef& k, float* head, std::vector<float>& d) {
    if (m == M) { distill_row<M>(x, z, V, target, w, logw, rule, k, head, d); return true; }
    if constexpr (M < ENS_MAX) return dispatch<M + 1>(m, x, z, V, target, w, logw, rule, k, head, d);
    return false;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "DSTL", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t c = 0; c < count; ++c) {
        int32_t head[4];
        float coef[3];
        if (!get(in, head, sizeof head) || !get(in, coef, sizeof coef)) return 2;
        const int M = head[0], V = head[1], rule = head[2], target = head[3];
        if (V < 1 || V > 4096 || !dr_args_ok(M, rule, coef[0], coef[1])) return 2;
        std::vector<float> weight((size_t)M), w((size_t)M), logw((size_t)M), x((size_t)V), z((size_t)M * V), d((size_t)V);
        if (!get(in, weight.data(), weight.size() * sizeof(float)) || !get(in, x.data(), x.size() * sizeof(float)) ||
            !get(in, z.data(), z.size() * sizeof(float)))
            return 2;
        for (int m = 0; m < M; ++m)
            if (!ens_weight_ok(weight[(size_t)m])) return 2;
        ens_normalise(weight.data(), M, w.data(), logw.data());
        const DistillCoef k = dr_coef(coef[0], coef[1], coef[2], V);
        float res[3];
        if (!dispatch<1>(M, x, z, V, target, w.data(), logw.data(), rule, k, res, d)) return 2;
        fwrite(res, sizeof(float), 3, out);
        fwrite(d.data(), sizeof(float), d.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
