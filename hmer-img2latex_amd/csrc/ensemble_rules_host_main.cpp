// The ensemble's combination rule (ensemble_rules.inc.h) as a stand-alone host program, so that a host test can hold
// it to a float64 restatement -- rows with -inf columns, a member that is all -inf, logits around -1e4 and +80, one to
// eight members -- under the host sanitizers (-fsanitize=address,undefined) in a process of its own.  It holds no
// rule: per member one pass of ens_accumulate over the row, then ens_logprob and ens_combine per column, in fp32.
//
//   ensemble_rules_host_main CASES OUT
//
// CASES: "ENSR", int32 count, then per case int32 M, V, rule; float32 weight[M]; float32 x[M][V].
// OUT per case: float32 y[V].
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ensemble_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <int M>
static void combine_row(const std::vector<float>& x, int V, const float* w, const float* logw, int rule, std::vector<float>& y) {
    float mx[M], log_s[M];
    for (int m = 0; m < M; ++m) {
        float s = 0.f;
        mx[m] = -INFINITY;
        for (int v = 0; v < V; ++v) ens_accumulate(mx[m], s, x[(size_t)m * V + v]);
        log_s[m] = logf(s);
    }
    for (int v = 0; v < V; ++v) {
        float lp[M];
        for (int m = 0; m < M; ++m) lp[m] = ens_logprob(x[(size_t)m * V + v], mx[m], log_s[m]);
        y[(size_t)v] = ens_combine<M>(lp, w, logw, rule);
    }
}

template <int M>
static bool dispatch(int m, const std::vector<float>& x, int V, const float* w, const float* logw, int rule, std::vector<float>& y) {
    if (m == M) { combine_row<M>(x, V, w, logw, rule, y); return true; }
    if constexpr (M < ENS_MAX) return dispatch<M + 1>(m, x, V, w, logw, rule, y);
    return false;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "ENSR", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[3];
        if (!get(in, head, sizeof head)) return 2;
        const int M = head[0], V = head[1], rule = head[2];
        if (M < 1 || M > ENS_MAX || V < 1 || V > 4096 || (rule != ENS_LOGPROB && rule != ENS_PROB)) return 2;
        std::vector<float> weight((size_t)M), w((size_t)M), logw((size_t)M), x((size_t)M * V), y((size_t)V);
        if (!get(in, weight.data(), weight.size() * sizeof(float)) || !get(in, x.data(), x.size() * sizeof(float))) return 2;
        for (int m = 0; m < M; ++m)
            if (!ens_weight_ok(weight[(size_t)m])) return 2;
        ens_normalise(weight.data(), M, w.data(), logw.data());
        if (!dispatch<1>(M, x, V, w.data(), logw.data(), rule, y)) return 2;
        fwrite(y.data(), sizeof(float), y.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
