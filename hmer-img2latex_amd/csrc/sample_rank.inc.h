// Ranking the samples of an image on the device (included by decode.hip inside its anonymous namespace, after
// sample_batched.inc.h): the rules of sample_rank_rules.inc.h on ids[images][samples][steps], the last two launches of
// i2l_sample_decode_multi and the whole of i2l_sample_rank.
//
//   sample_distance_kernel<W>  grid (images, samples), one workgroup per (image, sample i), one WAVE per sample j: the
//                              wave cuts both rows, computes d(i, j), and thread 0 sums the row into risk[i] and writes
//                              the cut of sample i.  risk, len and finished are outputs of the entry, so the second
//                              launch needs no scratch.
//   sample_order_kernel        one 64-thread workgroup per image: the keys, then ONE thread orders the <= 16 samples.
//
// One workgroup per (image, sample), not per image: the 16 x 16 distances of an image are its whole cost, and 16 waves a
// row keep every one of them in flight at once -- 16 images x 16 samples are 256 workgroups, one for each compute unit,
// where a workgroup per image would walk its 256 distances on one.  d(i, j) and d(j, i) are both computed; that spares
// an exchange between workgroups, and there is no poll, no atomic and no cooperative launch.
//
// The distance is myers_wave.inc.h's wave_edit_distance (Myers' bit-vector algorithm in blocks of 64 tokens; the risk
// objective's i2l_risk_rows calls the same function): both samples' tokens sit in registers, so the kernel touches no
// LDS but the 16 distances of its row.  Exact: integers throughout.  Every loop is bounded by steps <= 64 W.
#include "myers_wave.inc.h"

constexpr int SRK_NT = 64 * SR_MAX_SAMPLES;

struct RankParams {
    const int32_t* ids;      // [images][samples][steps]
    int images, samples, steps, end_id, rank;
    const double* score;     // [images][samples]
    const double* norm;      // [steps + 1] or null
    int32_t *len, *fin, *risk;
    double* key;
    int32_t* order;
    int32_t* dist;           // [images][samples][samples] or null
};

// blockDim.x == 64 * samples; steps <= 64 * W
template <int W>
__global__ __launch_bounds__(SRK_NT) void sample_distance_kernel(RankParams p) {
    typedef unsigned long long u64;
    __shared__ int drow[SR_MAX_SAMPLES];
    const int img = blockIdx.x, i = blockIdx.y, lane = threadIdx.x & 63, S = p.samples, T = p.steps;
    const int j = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int32_t* a = p.ids + ((size_t)img * S + i) * T;
    const int32_t* b = p.ids + ((size_t)img * S + j) * T;
    int pa[W], tb[W];
    int fa = T, fb = T;                                  // the place of the first END: sr_first_end, 64 places a ballot
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int at = 64 * w + lane;
        const bool in = at < T;
        pa[w] = in ? a[at] : 0;
        tb[w] = in ? b[at] : 0;
        const u64 ea = __ballot(in && pa[w] == p.end_id), eb = __ballot(in && tb[w] == p.end_id);
        if (ea && fa == T) fa = 64 * w + __builtin_ctzll(ea);
        if (eb && fb == T) fb = 64 * w + __builtin_ctzll(eb);
    }
    const SrCut ca = sr_cut_at(fa, T);
    const int R = ca.n, C = sr_cut_at(fb, T).n;
    const int d = wave_edit_distance<W>(pa, R, tb, C, lane);
    if (lane == 0) {
        drow[j] = d;
        if (p.dist) p.dist[((size_t)img * S + i) * S + j] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int risk = 0;
        for (int s = 0; s < S; ++s) risk += drow[s];
        const size_t at = (size_t)img * S + i;
        p.risk[at] = risk;
        p.len[at] = ca.len;
        p.fin[at] = ca.finished;
    }
}

// after sample_distance_kernel; grid images, 64 threads
__global__ __launch_bounds__(64) void sample_order_kernel(RankParams p) {
    __shared__ int risk[SR_MAX_SAMPLES];
    __shared__ double score[SR_MAX_SAMPLES], key[SR_MAX_SAMPLES];
    __shared__ int32_t order[SR_MAX_SAMPLES];
    const int img = blockIdx.x, s = threadIdx.x, S = p.samples;
    const size_t at = (size_t)img * S + s;
    if (s < S) {
        risk[s] = p.risk[at];
        score[s] = p.score[at];
        key[s] = sr_key(p.rank, risk[s], score[s], p.len[at], p.norm);
        p.key[at] = key[s];
    }
    __syncthreads();
    if (s == 0) sr_order(p.rank, S, risk, score, key, order);
    __syncthreads();
    if (s < S) p.order[at] = order[s];
}
