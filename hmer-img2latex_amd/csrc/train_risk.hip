// Minimum-risk fine-tuning (training/risk.py, TrainStep(risk=...)): the launches the objective adds to a training step.
//
//   i2l_risk_rows             risk_rows_kernel<W>: rewards, advantages and the assembled (images (samples + 1), steps + 1)
//                             token rows with their per-sequence coefficient, smoothing and part (risk_rules.inc.h)
//   i2l_ce_weighted_fwd_bwd   ce_rows_kernel<true> (ce_rows.inc.h) + ce_weighted_sum_kernel: the cross entropy whose
//                             sequences carry their own coefficient and smoothing
//   i2l_rows_repeat / _fold   the encoder rows repeated for the samples + 1 sequences of an image, and their gradient
//                             folded back
//
// No polls, no atomics, no cooperative launch; every output element is written; every sum is ordered.  Every refusal is
// host code in front of the first HIP call and leaves the outputs untouched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"
#include "risk_rules.inc.h"

namespace {

#include "ce_rows.inc.h"
#include "myers_wave.inc.h"

struct RiskParams {
    const int32_t* formulas;   // [images][steps + 1]
    const int32_t* draws;      // [images][samples][steps]
    int images, samples, steps, start_id, end_id, pad_id;
    float alpha, smoothing;
    int32_t* rows;             // [images][samples + 1][steps + 1]
    float *coef, *smooth;      // [images][samples + 1]
    int32_t* part;             // [images][samples + 1]
    int32_t *dist, *len;       // [images][samples]
    float *reward, *advantage; // [images][samples]
};

// grid images, blockDim.x == 64 * samples: one WAVE per draw; steps <= 64 * W.  The wave cuts its draw and the gold row
// with ballots (as sample_distance_kernel does), runs wave_edit_distance of draw against gold and writes its row; wave 0
// writes the gold row too.  After ONE barrier the first `samples` threads turn the rewards in LDS into advantages.
template <int W>
__global__ __launch_bounds__(64 * RK_MAX_SAMPLES) void risk_rows_kernel(RiskParams p) {
    typedef unsigned long long u64;
    __shared__ double reward[RK_MAX_SAMPLES];
    const int img = blockIdx.x, lane = threadIdx.x & 63, S = p.samples, T = p.steps;
    const int n = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int32_t* gold_row = p.formulas + (size_t)img * (T + 1);
    const int32_t* gold = gold_row + 1;
    const int32_t* draw = p.draws + ((size_t)img * S + n) * T;
    int pa[W], tb[W];
    int fa = T, fb = T;                                  // first END of the draw; first END or PAD of the gold tokens
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int at = 64 * w + lane;
        const bool in = at < T;
        pa[w] = in ? draw[at] : 0;
        tb[w] = in ? gold[at] : 0;
        const u64 ea = __ballot(in && pa[w] == p.end_id);
        const u64 eb = __ballot(in && (tb[w] == p.end_id || tb[w] == p.pad_id));
        if (ea && fa == T) fa = 64 * w + __builtin_ctzll(ea);
        if (eb && fb == T) fb = 64 * w + __builtin_ctzll(eb);
    }
    const int R = sr_cut_at(fa, T).n, C = fb;            // rk_gold_len(gold, T, end, pad) == fb
    const int d = wave_edit_distance<W>(pa, R, tb, C, lane);
    const size_t seq0 = (size_t)img * (S + 1);
    int32_t* row = p.rows + (seq0 + 1 + n) * (size_t)(T + 1);
    if (lane == 0) row[0] = p.start_id;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int at = 64 * w + lane;
        if (at < T) row[1 + at] = at <= fa ? pa[w] : p.pad_id;        // rk_draw_row_token
    }
    if (n == 0) {
        int32_t* out = p.rows + seq0 * (size_t)(T + 1);
        for (int t = lane; t <= T; t += 64) out[t] = gold_row[t];
    }
    if (lane == 0) {
        const size_t at = (size_t)img * S + n;
        const double r = rk_reward(d, R, C);
        reward[n] = r;
        p.dist[at] = d;
        p.len[at] = R;
        p.reward[at] = (float)r;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < S) {
        const double a = rk_advantage(reward, t, S);
        p.advantage[(size_t)img * S + t] = (float)a;
        p.coef[seq0 + 1 + t] = rk_coef_draw(p.alpha, a);
        p.smooth[seq0 + 1 + t] = 0.f;
        p.part[seq0 + 1 + t] = RK_PART_DRAW;
    }
    if (t == 64) {                                       // samples >= 2: the block has a second wave
        p.coef[seq0] = rk_coef_gold(p.alpha);
        p.smooth[seq0] = p.smoothing;
        p.part[seq0] = RK_PART_GOLD;
    }
}

template <int... Ws, class F>
bool risk_with_width(int width, F&& f) {
    return ((width == Ws && (f(std::integral_constant<int, Ws>{}), true)) || ...);
}

// out[0] = sum_i coef[i / steps] loss[i], out[1] = sum(keep); parts = [sum loss, sum keep] of part 0, then of part 1,
// unweighted.  One workgroup, fixed order -> deterministic; the stride and the tree are ordered_sum2_kernel's, so with
// every coefficient 1 out[] holds that kernel's bits.
__global__ __launch_bounds__(256) void ce_weighted_sum_kernel(const float* __restrict__ loss, const float* __restrict__ keep,
                                                              size_t n, int steps, const float* __restrict__ coef,
                                                              const int32_t* __restrict__ part, float* __restrict__ out,
                                                              float* __restrict__ parts) {
    __shared__ double red[6][256];
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (size_t i = threadIdx.x; i < n; i += 256) {
        const size_t seq = i / (size_t)steps;
        const float l = loss[i], k = keep[i];
        acc[0] += coef[seq] * l;
        acc[1] += k;
        const bool gold = part[seq] == RK_PART_GOLD;
        acc[2] += gold ? l : 0.f;
        acc[3] += gold ? k : 0.f;
        acc[4] += gold ? 0.f : l;
        acc[5] += gold ? 0.f : k;
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) red[c][threadIdx.x] = acc[c];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int c = 0; c < 6; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)red[0][0];
        out[1] = (float)red[1][0];
        if (parts) {
#pragma unroll
            for (int c = 0; c < 4; ++c) parts[c] = (float)red[2 + c][0];
        }
    }
}

// out[r * times + j][c] = in[r][c]: one thread per output element
__global__ __launch_bounds__(256) void rows_repeat_kernel(const float* __restrict__ in, size_t total, int width, int times,
                                                          float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t orow = i / (size_t)width, c = i - orow * (size_t)width;
    out[i] = in[(orow / (size_t)times) * (size_t)width + c];
}

// out[r][c] = sum_j in[r * times + j][c], an fp32 sum in the order j = 0 .. times - 1: one thread per output element
__global__ __launch_bounds__(256) void rows_fold_kernel(const float* __restrict__ in, size_t total, int width, int times,
                                                        float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t r = i / (size_t)width, c = i - r * (size_t)width;
    const float* x = in + r * (size_t)times * (size_t)width + c;
    float s = x[0];
    for (int j = 1; j < times; ++j) s += x[(size_t)j * (size_t)width];
    out[i] = s;
}

// rows * width elements, one thread each: the grid of both kernels, 0 when it does not fit a launch
unsigned rows_grid(int rows, int width, int times, size_t* total) {
    if (rows <= 0 || width <= 0 || times <= 0) return 0;
    const size_t n = (size_t)rows * (size_t)width;
    if (n * (size_t)times > ((size_t)1 << 38)) return 0;        // the wider of the two grids stays below 2^31 workgroups
    const size_t blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffu) return 0;
    *total = n;
    return (unsigned)blocks;
}

}  // namespace

extern "C" int i2l_risk_rows(const int32_t* formulas, const int32_t* draws, int images, int samples, int steps, int start_id,
                             int end_id, int pad_id, float alpha, float label_smoothing, int32_t* rows_out, float* coef_out,
                             float* smooth_out, int32_t* part_out, int32_t* dist_out, int32_t* len_out, float* reward_out,
                             float* advantage_out, i2l_stream_t stream) {
    if (!formulas || !draws || !rows_out || !coef_out || !smooth_out || !part_out || !dist_out || !len_out || !reward_out ||
        !advantage_out)
        return I2L_ERR_ARG;
    const int bad = rk_check(images, samples, steps, alpha, label_smoothing);
    if (bad) return bad == 1 ? I2L_ERR_ARG : I2L_ERR_UNSUPPORTED;
    RiskParams p{formulas, draws, images, samples, steps, start_id, end_id, pad_id, alpha, label_smoothing,
                 rows_out, coef_out, smooth_out, part_out, dist_out, len_out, reward_out, advantage_out};
    const int width = steps <= 256 ? i2l_cdiv(steps, 64) : steps <= 512 ? 8 : 16;
    hipStream_t s = i2l_s(stream);
    const bool took = risk_with_width<1, 2, 3, 4, 8, 16>(width, [&](auto w) {
        hipLaunchKernelGGL(risk_rows_kernel<w>, dim3(images), dim3(64 * samples), 0, s, p);
    });
    if (!took) return I2L_ERR_UNSUPPORTED;
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

extern "C" size_t i2l_ce_weighted_workspace_bytes(int rows) {
    return rows > 0 ? 2 * i2l_align((size_t)rows * sizeof(float)) : 0;
}

extern "C" int i2l_ce_weighted_fwd_bwd(const float* logits, const int32_t* targets, int seqs, int steps, int vocab, int pad_id,
                                       const float* seq_coef, const float* seq_smooth, const int32_t* seq_part,
                                       void* workspace, size_t workspace_bytes, float* dlogits_out,
                                       float* loss_sum_and_count_out, float* parts_out, i2l_stream_t stream) {
    if (!logits || !targets || !seq_coef || !seq_smooth || !seq_part || !loss_sum_and_count_out) return I2L_ERR_ARG;
    if (seqs <= 0 || steps <= 0 || vocab <= 0) return I2L_ERR_ARG;
    if ((size_t)seqs * (size_t)steps > 0x7fffffffu) return I2L_ERR_UNSUPPORTED;
    const int rows = seqs * steps;
    const size_t part = i2l_align((size_t)rows * sizeof(float));
    if (!workspace || workspace_bytes < 2 * part) return I2L_ERR_WORKSPACE;
    float* row_loss = static_cast<float*>(workspace);
    float* row_keep = reinterpret_cast<float*>(static_cast<char*>(workspace) + part);
    hipStream_t s = i2l_s(stream);
    hipLaunchKernelGGL(ce_rows_kernel<true>, dim3(rows), dim3(256), 0, s, logits, targets, dlogits_out, row_loss, row_keep,
                       vocab, pad_id, 0.f, CeSeq{seq_coef, seq_smooth, steps});
    I2L_CHECK_LAUNCH();
    hipLaunchKernelGGL(ce_weighted_sum_kernel, dim3(1), dim3(256), 0, s, (const float*)row_loss, (const float*)row_keep,
                       (size_t)rows, steps, seq_coef, seq_part, loss_sum_and_count_out, parts_out);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

extern "C" int i2l_rows_repeat(const float* in, int rows, int width, int times, float* out, i2l_stream_t stream) {
    if (!in || !out) return I2L_ERR_ARG;
    size_t total = 0;
    const unsigned grid = rows_grid(rows, width, times, &total);
    if (!grid) return I2L_ERR_ARG;
    total *= (size_t)times;
    hipLaunchKernelGGL(rows_repeat_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, i2l_s(stream), in, total, width,
                       times, out);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

extern "C" int i2l_rows_fold(const float* in, int rows, int width, int times, float* out, i2l_stream_t stream) {
    if (!in || !out) return I2L_ERR_ARG;
    size_t total = 0;
    const unsigned grid = rows_grid(rows, width, times, &total);
    if (!grid) return I2L_ERR_ARG;
    hipLaunchKernelGGL(rows_fold_kernel, dim3(grid), dim3(256), 0, i2l_s(stream), in, total, width, times, out);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
