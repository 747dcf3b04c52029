// Word-level distillation (included by train_decoder.hip inside its anonymous namespace): the student trains against
// the token distribution of 1 .. 8 teachers at every teacher-forced position.  distill_rules.inc.h states the loss;
// this file holds the kernel that evaluates it, the ordered sum of its three row vectors and the launch.
//
// ce_distill_rows_kernel<M>: ensemble_combine_kernel's shape, one wave per row and DR_NT / 64 rows per workgroup.  A
// lane holds a CHUNK of the row in registers -- DR_CHUNK lane-strided columns of the student and of every teacher -- and
// the (M + 1) x DR_CHUNK loads of a chunk are issued together.  The row needs three dependent reductions:
//   pass 1   the teachers' (max, sum exp) pairs; the student's max, sum exp(x - max), sum exp((x - max) / tau), sum x
//   pass 2   y[v] (dr_teacher) and the max and sum of y / tau              backwards over the chunks
//   pass 3   the loss terms and dlogits                                    forwards
// so that the last chunk of one pass is the first of the next and is still in registers: a row of V <= 64 * DR_CHUNK =
// 512 columns (the shipped vocabulary) is read ONCE and no (rows, V) intermediate exists; a longer row is re-read chunk
// by chunk, y recomputed, whatever its length.  A pad row returns before any load of a logit.
//
// Block size and chunk width, from the compiler's resource report for gfx950 (-Rpass-analysis=kernel-resource-usage):
// DR_CHUNK = 8 with 256 threads gives 64 VGPRs at M = 1 (8 waves per SIMD), 80 at M = 2 (6 waves), 98 at M = 4 (4 waves)
// and 160 at M = 8 (3 waves); no scratch, no spill and no LDS at any M.  The kernel streams (M + 1) rows in and one out
// per row, so what it needs is loads in flight, and a chunk already has 8 (M + 1) per lane: 3 waves of 72 loads at
// M = 8 are as many as 8 waves of 16 at M = 1 and more.  DR_CHUNK = 16 would keep V <= 1024 in registers but doubles
// the row registers (M = 8 would be past 256 and down to one or two waves) for vocabularies the project does not ship.
// 256 threads rather than 64: four rows per workgroup keep the grid at rows / 4 workgroups (2384 for 64 x 149 rows)
// instead of 9536 one-wave workgroups; nothing is shared between the waves, so there is no barrier and no LDS.
//
// distill_sum3_kernel is ordered_sum2_kernel's scheme with a third vector: one workgroup, thread i adds rows i, i + 256,
// ... in double, the 256 partial sums meet in an LDS tree -- a fixed order, so the three sums are deterministic.

#include "distill_rules.inc.h"

constexpr int DR_NT = 256;
constexpr int DR_CHUNK = 8;

struct DistillArgs {
    const float* x;              // (rows, V) student logits
    const int32_t* tgt;          // (rows)
    const float* z[ENS_MAX];     // teacher m's (rows, ld[m]) logits
    int ld[ENS_MAX];
    float w[ENS_MAX], logw[ENS_MAX];
    float* d;                    // (rows, V) or null
    float *row_hard, *row_soft, *row_keep;
    int rows, V, pad, rule;
    DistillCoef k;
};

// chunk `c`: xs[i] = x[512 c + 64 i + lane] and a[m][i] likewise, -inf beyond V (the accumulators pass over it)
template <int M>
__device__ __forceinline__ void dr_load_chunk(float (&xs)[DR_CHUNK], float (&a)[M][DR_CHUNK], const float* x,
                                              const float* const (&z)[M], int c, int V, int lane) {
#pragma unroll
    for (int i = 0; i < DR_CHUNK; ++i) {
        const int v = (c * DR_CHUNK + i) * 64 + lane;
        xs[i] = v < V ? x[v] : -INFINITY;
#pragma unroll
        for (int m = 0; m < M; ++m) a[m][i] = v < V ? z[m][v] : -INFINITY;
    }
}

template <int M>
__device__ __forceinline__ void dr_teacher_chunk(float (&y)[DR_CHUNK], const float (&a)[M][DR_CHUNK], const float (&top)[M],
                                                 const float (&log_s)[M], const DistillArgs& e) {
#pragma unroll
    for (int i = 0; i < DR_CHUNK; ++i) {
        float zc[M];
#pragma unroll
        for (int m = 0; m < M; ++m) zc[m] = a[m][i];
        y[i] = dr_teacher<M>(zc, top, log_s, e.w, e.logw, e.rule);
    }
}

template <int M>
__global__ __launch_bounds__(DR_NT) void ce_distill_rows_kernel(DistillArgs e) {
    const int V = e.V, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DR_NT / 64) + (threadIdx.x >> 6);
    if (row >= e.rows) return;
    const int tgt = e.tgt[row];
    float* d = e.d ? e.d + (size_t)row * V : nullptr;
    if (tgt == e.pad) {          // selected, not multiplied: no logit of this row is read
        if (d)
            for (int v = lane; v < V; v += 64) d[v] = 0.f;
        if (lane == 0) { e.row_hard[row] = 0.f; e.row_soft[row] = 0.f; e.row_keep[row] = 0.f; }
        return;
    }
    const DistillCoef k = e.k;
    const float* x = e.x + (size_t)row * V;
    const float* z[M];
    float xs[DR_CHUNK], a[M][DR_CHUNK], y[DR_CHUNK], mx[M], s[M], top[M], log_s[M];
#pragma unroll
    for (int m = 0; m < M; ++m) { z[m] = e.z[m] + (size_t)row * e.ld[m]; mx[m] = -INFINITY; s[m] = 0.f; top[m] = 0.f; log_s[m] = 0.f; }
    const int chunks = (V + 64 * DR_CHUNK - 1) / (64 * DR_CHUNK);
    // pass 1
    float xm1 = -INFINITY, s1 = 0.f, xmp = -INFINITY, sp = 0.f, sx = 0.f;
    for (int c = 0; c < chunks; ++c) {
        dr_load_chunk<M>(xs, a, x, z, c, V, lane);
#pragma unroll
        for (int i = 0; i < DR_CHUNK; ++i) {
            dr_accumulate(xm1, s1, xs[i], 1.f);
            dr_accumulate(xmp, sp, xs[i], k.inv_tau);
            sx += (c * DR_CHUNK + i) * 64 + lane < V ? xs[i] : 0.f;
            if (M > 1) {
#pragma unroll
                for (int m = 0; m < M; ++m) ens_accumulate(mx[m], s[m], a[m][i]);
            }
        }
    }
    DistillRow r;
    r.xmx = wave_max(xm1);
    r.s1 = wave_sum(dr_rescale(xm1, s1, r.xmx, 1.f));
    r.sp = wave_sum(dr_rescale(xmp, sp, r.xmx, k.inv_tau));
    r.log_sp = logf(r.sp);
    sx = wave_sum(sx);
    if (M > 1) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            top[m] = wave_max(mx[m]);
            log_s[m] = logf(wave_sum(ens_rescale(mx[m], s[m], top[m])));
        }
    }
    // pass 2, backwards: the last chunk of pass 1 is still in registers
    float ym = -INFINITY, sq = 0.f;
    for (int c = chunks - 1; c >= 0; --c) {
        if (c != chunks - 1) dr_load_chunk<M>(xs, a, x, z, c, V, lane);
        dr_teacher_chunk<M>(y, a, top, log_s, e);
#pragma unroll
        for (int i = 0; i < DR_CHUNK; ++i) dr_accumulate(ym, sq, y[i], k.inv_tau);
    }
    r.ymx = wave_max(ym);
    r.sq = wave_sum(dr_rescale(ym, sq, r.ymx, k.inv_tau));
    r.log_sq = logf(r.sq);
    // pass 3, forwards: chunk 0 and its y are still in registers
    const int tg = dr_clamp_target(tgt, V);
    float kl_sum = 0.f;
    for (int c = 0; c < chunks; ++c) {
        if (c != 0) {
            dr_load_chunk<M>(xs, a, x, z, c, V, lane);
            dr_teacher_chunk<M>(y, a, top, log_s, e);
        }
#pragma unroll
        for (int i = 0; i < DR_CHUNK; ++i) {
            const int v = (c * DR_CHUNK + i) * 64 + lane;
            if (v < V) {
                float kl;
                const float g = dr_column(xs[i], y[i], v == tg, r, k, kl);
                kl_sum += kl;
                if (d) d[v] = g;
            }
        }
    }
    kl_sum = wave_sum(kl_sum);
    if (lane == 0) {
        e.row_hard[row] = dr_hard(r.xmx, r.s1, sx, x[tg], V, k.eps);
        e.row_soft[row] = dr_soft(kl_sum, k.tau);
        e.row_keep[row] = 1.f;
    }
}

// out[0] = alpha sum(hard) + (1 - alpha) sum(soft), out[1] = sum(keep), parts[0] = sum(hard), parts[1] = sum(soft)
__global__ __launch_bounds__(256) void distill_sum3_kernel(const float* __restrict__ hard, const float* __restrict__ soft,
                                                           const float* __restrict__ keep, size_t n, float alpha,
                                                           float* __restrict__ out, float* __restrict__ parts) {
    __shared__ double ra[256], rb[256], rc[256];
    double sa = 0.0, sb = 0.0, sc = 0.0;
    for (size_t i = threadIdx.x; i < n; i += 256) { sa += hard[i]; sb += soft[i]; sc += keep[i]; }
    ra[threadIdx.x] = sa; rb[threadIdx.x] = sb; rc[threadIdx.x] = sc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            ra[threadIdx.x] += ra[threadIdx.x + off];
            rb[threadIdx.x] += rb[threadIdx.x + off];
            rc[threadIdx.x] += rc[threadIdx.x + off];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = (float)((double)alpha * ra[0] + (double)(1.f - alpha) * rb[0]);
        out[1] = (float)rc[0];
        if (parts) { parts[0] = (float)ra[0]; parts[1] = (float)rb[0]; }
    }
}

template <int M>
void launch_distill(int n, const DistillArgs& e, hipStream_t s) {
    if (n == M) {
        hipLaunchKernelGGL(ce_distill_rows_kernel<M>, dim3(i2l_cdiv(e.rows, DR_NT / 64)), dim3(DR_NT), 0, s, e);
        return;
    }
    if constexpr (M < ENS_MAX) launch_distill<M + 1>(n, e, s);
}
