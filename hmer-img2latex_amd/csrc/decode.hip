// LSTM decoder step loop as ONE persistent launch (reference decoder.py:197-284 driven
// by seq2seq.py:210-221 / predictor.py:283-347).
//
// Design (DESIGN.md "decode"): the recurrence of one batch row never touches another
// row, so rows are partitioned over workgroups and a workgroup runs ALL steps of its
// rows with no inter-workgroup communication: no grid barrier, no host sync, nothing
// that can deadlock.  Per step a workgroup streams the recurrent and projection
// weights (L2-resident: 1.5 MB at E=H=256,V=512) as coalesced 16-byte loads; the state
// (h, c) lives in LDS for the whole loop.
//
// Weight images built once per call by i2l_decoder_prepare():
//   WhhT[l][k][4j+g] = W_hh_l[g*H+j][k]      gate-interleaved transpose: thread j reads one
//   WihT[l][k][4j+g] = W_ih_l[g*H+j][k] (l>0) float4 per k = (i,f,g,o) of hidden unit j
//   P[v][4j+g]       = sum_e Emb[v][e] * W_ih_0[g*H+j][e]          token half of layer-0 gates
//   Genc[b][4j+g]    = sum_e enc[b][e] * W_ih_0[g*H+j][E+e] + b_ih_0 + b_hh_0   image half
//   WoutT[k][v]      = W_out[v][k], columns padded to a multiple of 512 (bias -inf)
// so a step is: gates = P[tok] + Genc + h @ W_hh^T (a k-ordered fmaf chain per gate),
// LSTM pointwise, logits = h' @ W_out^T + b, first-index argmax by wave shuffles.
#include <math.h>
#include <stdlib.h>
#include <type_traits>

#include "common.h"

namespace {

#include "lstm_rows.inc.h"

constexpr int MAXL = I2L_MAX_LSTM_LAYERS;
constexpr int NT = 256;        // threads per workgroup
constexpr int VCHUNK = 2 * NT;  // vocab columns per projection pass

constexpr size_t GROUP_STATUS_BYTES = 2048;   // status words in front of a grouped kernel's exchange granules
inline bool group_shape_ok(int V, int H, int L) { return L == 1 && H == 256 && V <= 512; }

// out[k][c] = W[n(c)][k] for c < Npad; n(c) = (c&3)*perm_h + (c>>2) when perm_h > 0 else c; rows n >= N read as 0.
__global__ __launch_bounds__(256) void transpose_perm_kernel(const float* __restrict__ W, int N, int K,
                                                             float* __restrict__ out, int ld_out, int Npad,
                                                             int perm_h) {
    __shared__ float tile[64][65];
    const int c0 = blockIdx.x * 64, k0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, k = k0 + tx;
        const int n = perm_h > 0 ? (c & 3) * perm_h + (c >> 2) : c;
        tile[i][tx] = (c < Npad && n < N && k < K) ? W[(size_t)n * K + k] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int k = k0 + i, c = c0 + tx;
        if (k < K && c < Npad) out[(size_t)k * ld_out + c] = tile[tx][i];
    }
}

__global__ void bias_perm_kernel(const float* __restrict__ b_ih, const float* __restrict__ b_hh,
                                 float* __restrict__ out, int H) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < 4 * H) {
        const int n = (c & 3) * H + (c >> 2);
        out[c] = b_ih[n] + b_hh[n];
    }
}

__global__ void bout_pad_kernel(const float* __restrict__ b_out, float* __restrict__ out, int V, int Vp) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < Vp) out[v] = v < V ? b_out[v] : -INFINITY;
}

struct StepWeights {
    int H, L, V, Vp;
    const float* P;
    const float* Genc;
    const float* WhhT[MAXL];
    const float* WihT[MAXL];
    const float* biasP[MAXL];
    const float* WoutT;
    const float* boutP;
    const void* wpack16;      // decode_group16_kernel's operand image (null when the dimensions have no grouped path)
};

struct DecodeParams {
    StepWeights w;
    int B, T;
    const int32_t* tok0;
    const int32_t* forced;
    const float* h0;
    const float* c0;
    float* h_out;
    float* c_out;
    int32_t* ids;
    float* logits;
    float temperature;
    int use_temp, select, stop, end_id;
    int top_k; float top_p; unsigned long long seed; float* probs;   // I2L_SELECT_SAMPLE only
};

// All L layers of one LSTM time step for R rows of one workgroup (decoder.py:247/277 at seq len 1).
// h is double-buffered in LDS: reads hs[par], writes hs[par^1]; c_in -> c_out (may alias: each
// element is read and written by the same thread).  tok[r] selects the row of P, grow[r] the row of Genc.
// Ends with a __syncthreads(): hs[par^1] is complete on return.
template <int R>
__device__ __forceinline__ void lstm_layers(const StepWeights& w, const int (&tok)[R], const int (&grow)[R],
                                            float* hs, const float* c_in, float* c_out, int par, int tid) {
    const int H = w.H, L = w.L;
    const size_t G = 4 * (size_t)H;
    for (int l = 0; l < L; ++l) {
        const float* h_old = hs + ((size_t)par * L + l) * R * H;
        float* h_new = hs + ((size_t)(par ^ 1) * L + l) * R * H;
        for (int j = tid; j < H; j += NT) {
            float4 acc[R];
            if (l == 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 a = *reinterpret_cast<const float4*>(w.P + (size_t)tok[r] * G + 4 * j);
                    const float4 e = *reinterpret_cast<const float4*>(w.Genc + (size_t)grow[r] * G + 4 * j);
                    acc[r] = make_float4(a.x + e.x, a.y + e.y, a.z + e.z, a.w + e.w);
                }
            } else {
                const float4 bb = *reinterpret_cast<const float4*>(w.biasP[l] + 4 * j);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = bb;
                matvec<R, float4>(acc, w.WihT[l] + 4 * j, G, hs + ((size_t)(par ^ 1) * L + (l - 1)) * R * H, H, H);
            }
            matvec<R, float4>(acc, w.WhhT[l] + 4 * j, G, h_old, H, H);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const size_t ci = ((size_t)l * R + r) * H + j;
                const float ig = sigmoidf_(acc[r].x), fg = sigmoidf_(acc[r].y);
                const float gg = tanhf_(acc[r].z), og = sigmoidf_(acc[r].w);
                const float cn = fg * c_in[ci] + ig * gg;
                c_out[ci] = cn;
                h_new[r * H + j] = og * tanhf_(cn);
            }
        }
        __syncthreads();
    }
}

// logits = h_top @ W_out^T + b for R rows, 512 vocabulary columns per pass.  16-byte loads only
// (8-byte streams run at ~0.55x the 16-byte rate on gfx950): thread t owns the 4 columns
// 4*(t&127).. and HALF of k -- threads 0-127 sum k < H/2 (starting from the bias), threads 128-255
// sum k >= H/2; the two partial chains meet through LDS (psum) in a fixed order, so results are
// deterministic.  Optionally writes raw logits to global (lp[r] != null), keeps logit/temperature
// in LDS (lg != null), and returns each thread's running (max, first index); upper-half threads
// return -inf.  Contains __syncthreads(); every thread of the workgroup must call it.
template <int R, bool PRE = false>
__device__ __forceinline__ void project(const StepWeights& w, const float* h_top, float* const (&lp)[R],
                                        float* lg, bool use_temp, float temperature, float (&best)[R],
                                        int (&besti)[R], float* psum, int tid, float4 (*pre)[PF] = nullptr) {
    const int half = tid >> 7, c4 = (tid & 127) * 4;
    const int Hh = w.H >> 1;
#pragma unroll
    for (int r = 0; r < R; ++r) { best[r] = -INFINITY; besti[r] = 0x7fffffff; }
    for (int v0 = c4; v0 < w.Vp; v0 += VCHUNK) {
        float4 acc[R];
        const float4 bb = half == 0 ? *reinterpret_cast<const float4*>(w.boutP + v0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = bb;
        if (PRE && v0 == c4)      // first pass: rows 0..PF-1 were prefetched before the LSTM step
            matvec_pre<R, float4>(acc, *pre, w.WoutT + (size_t)half * Hh * w.Vp + v0, (size_t)w.Vp, h_top + half * Hh, w.H, Hh);
        else
            matvec<R, float4>(acc, w.WoutT + (size_t)half * Hh * w.Vp + v0, (size_t)w.Vp, h_top + half * Hh, w.H, Hh);
        if (half == 1) {
#pragma unroll
            for (int r = 0; r < R; ++r) *reinterpret_cast<float4*>(psum + ((size_t)r * 128 + (tid & 127)) * 4) = acc[r];
        }
        __syncthreads();
        if (half == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 u = *reinterpret_cast<const float4*>(psum + ((size_t)r * 128 + tid) * 4);
                float a[4] = {acc[r].x + u.x, acc[r].y + u.y, acc[r].z + u.z, acc[r].w + u.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (lp[r] && v0 + e < w.V) lp[r][v0 + e] = a[e];
                    if (use_temp) a[e] = a[e] / temperature;
                    if (lg) lg[r * w.Vp + v0 + e] = a[e];
                    if (a[e] > best[r]) { best[r] = a[e]; besti[r] = v0 + e; }
                }
            }
        }
        if (v0 + VCHUNK < w.Vp) __syncthreads();          // psum is reused by the next pass
    }
}

// Fold per-thread (max, index) pairs over the workgroup; on return every thread holds the result.
// redv/redi: LDS [NT/64][R].  Contains two __syncthreads().
template <int R>
__device__ __forceinline__ void block_argmax(float (&best)[R], int (&besti)[R], float* redv, int* redi, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        wave_argmax(best[r], besti[r]);
        if (lane == 0) { redv[wave * R + r] = best[r]; redi[wave * R + r] = besti[r]; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float bv = redv[r];
        int bi = redi[r];
#pragma unroll
        for (int wv = 1; wv < NT / 64; ++wv) {
            const float ov = redv[wv * R + r];
            const int oi = redi[wv * R + r];
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        best[r] = bv; besti[r] = bi;
    }
    __syncthreads();
}

// workgroup-wide sum / max (every thread gets the result); red: LDS [NT/64]; contain two __syncthreads()
__device__ __forceinline__ float block_sum(float v, float* red, int tid) {
    v = wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < NT / 64; ++wv) s += red[wv];
    __syncthreads();
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red, int tid) {
    v = wave_max(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float s = red[0];
#pragma unroll
    for (int wv = 1; wv < NT / 64; ++wv) s = fmaxf(s, red[wv]);
    __syncthreads();
    return s;
}
// counter-based uniform in [0,1): splitmix64 finaliser of (seed, row, step); 24 random bits
__device__ __forceinline__ float uniform01(unsigned long long seed, unsigned row, unsigned step) {
    unsigned long long z = seed + ((unsigned long long)row << 32 | step) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// Phase (c) of a beam step for one live slot, by one wave: log_softmax of the row x[0, V) in fp32 (seq2seq.py:266) and
// its top K (:267: descending, the lower index first on ties) by K rounds of first-index wave arg max.  Lane 0 writes
// topv[0, K) / topi[0, K).  V <= 2048: the taken-mask has 32 bits per lane.
//
// `al` is the slot's pick policy, the one select_row takes (decode_batched.inc.h).  Under AllowAll every test of it is a
// constant and this is the function as written above.  Under a policy that forbids columns (beam_constrained.inc.h) the
// class byte is read beside the logit ONCE, in the max pass, into a 32-bit mask per lane; max, sum, log and the arg-max
// rounds run over the allowed columns only -- a forbidden column enters the softmax as -inf, the constrained sampler's
// convention.
// Returns, in every lane, how many rounds found a column: the list ends at the first one that finds none (every later
// round finds none either; the plain list is read to K all the same, as it always was).
template <class Pick>
__device__ __forceinline__ int beam_topk_row(const float* x, int V, int K, int lane, const Pick& al, float* topv, int* topi) {
    unsigned off = 0;                                    // bit i: element lane + 64*i is not allowed
    float m = -INFINITY;
    for (int v = lane, i = 0; v < V; v += 64, ++i) {
        const float a = x[v];
        if (al.allows(v, al.cls(v))) m = fmaxf(m, a);
        else off |= 1u << i;
    }
    m = wave_max(m);
    float s = 0.f;
    for (int v = lane, i = 0; v < V; v += 64, ++i)
        if (!((off >> i) & 1u)) s += expf(x[v] - m);
    s = wave_sum(s);
    const float lse = logf(s);
    unsigned taken = off;                                // bit i: element lane + 64*i already selected, or not allowed
    int n = 0;
    for (int j = 0; j < K; ++j) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int v = lane, i = 0; v < V; v += 64, ++i)
            if (!((taken >> i) & 1u) && x[v] > bv) { bv = x[v]; bi = v; }
        wave_argmax(bv, bi);
        if (bi < V && (bi & 63) == lane) taken |= 1u << (bi >> 6);
        if (lane == 0) { topv[j] = (bv - m) - lse; topi[j] = bi < V ? bi : 0; }
        if (bi < V) ++n;                                 // a round without a column: so are all later ones
    }
    return n;
}

#include "decode_group.inc.h"
#include "decode_group16.inc.h"
#include "beam_group.inc.h"
#include "decode_batched.inc.h"
#include "sample_batched.inc.h"
#include "sample_rank_rules.inc.h"
#include "sample_rank.inc.h"
#include "argument_rules.inc.h"      // and bracket_rules.inc.h
#include "decode_constrained.inc.h"
#include "beam_bracket_rules.inc.h"
#include "beam_batched.inc.h"
#include "beam_nbest.inc.h"
#include "beam_constrained.inc.h"

// KR / KL > 0 (fast path for R == 1, L == 1, H <= 256: thread j owns hidden unit j for the whole loop):
// rows [0,KR) of WhhT stay in the thread's registers and rows [KR,KR+KL) in LDS for all steps, so only
// H-KR-KL rows are streamed from L2 per step.  The fmaf chain still runs k = 0..H-1 in order, so the
// results are bit-identical to the streaming-only kernel.
template <int R, int KR, int KL, bool SAMPLE = false>
__global__ __launch_bounds__(NT) void decode_kernel(DecodeParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const StepWeights& w = p.w;
    const int H = w.H, L = w.L, B = p.B, T = p.T, V = w.V;
    float* hs = smem;                          // [2][L][R][H]  double-buffered h
    float* cs = hs + 2 * L * R * H;            // [L][R][H]
    float* redv = cs + L * R * H;              // [4][R]
    int* redi = reinterpret_cast<int*>(redv + 4 * R);   // [4][R]
    int* tok_s = redi + 4 * R;                 // [R]
    int* fin_s = tok_s + R;                    // [R]
    float* psum = reinterpret_cast<float*>(fin_s + R + ((4 - ((10 * R) & 3)) & 3));   // [R][128][4], 16-byte aligned
    float* wl = psum + R * 512;                         // [KL][4H] resident rows of WhhT[0]
    float* lg = wl + (size_t)KL * 4 * H;                // [R][Vp], only with I2L_SELECT_SOFTMAX / _SAMPLE

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * R;
    int grow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) grow[r] = min(row0 + r, B - 1);

    for (int idx = tid; idx < L * R * H; idx += NT) {
        const int l = idx / (R * H);
        const int rem = idx - l * (R * H);
        const int r = rem / H, j = rem - r * H;
        const size_t g = ((size_t)l * B + min(row0 + r, B - 1)) * H + j;
        hs[idx] = p.h0 ? p.h0[g] : 0.f;
        cs[idx] = p.c0 ? p.c0[g] : 0.f;
    }
    if (tid < R) {
        tok_s[tid] = p.tok0[min(row0 + tid, B - 1)];
        fin_s[tid] = 0;
    }
    // resident slices of WhhT[0] (loaded once per launch)
    float4 wres[KR > 0 ? KR : 1];
    const int jj = min(tid, H - 1);
    if (KR > 0) {
#pragma unroll
        for (int k = 0; k < KR; ++k) wres[k] = *reinterpret_cast<const float4*>(w.WhhT[0] + (size_t)k * 4 * H + 4 * jj);
    }
    float4 genc_reg[R];                                   // image half of the layer-0 gates: constant over the loop
#pragma unroll
    for (int r = 0; r < R; ++r)
        genc_reg[r] = (KR + KL > 0) ? *reinterpret_cast<const float4*>(w.Genc + (size_t)grow[r] * 4 * H + 4 * jj)
                                    : make_float4(0.f, 0.f, 0.f, 0.f);
    if (KL > 0) {
        const float4* src = reinterpret_cast<const float4*>(w.WhhT[0] + (size_t)KR * 4 * H);
        for (int idx = tid; idx < KL * H; idx += NT) reinterpret_cast<float4*>(wl)[idx] = src[idx];
    }
    __syncthreads();

    int par = 0;
    int t = 0;
    for (; t < T; ++t) {
        int tok[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int tk = p.forced ? p.forced[(size_t)grow[r] * T + t] : tok_s[r];
            tok[r] = min(max(tk, 0), V - 1);
        }
        float4 pre[PF];                                   // first batch of the projection stream (fast path)
        if (KR + KL > 0)
            load_batch<float4>(pre, w.WoutT + (size_t)(tid >> 7) * (H >> 1) * w.Vp + (tid & 127) * 4, (size_t)w.Vp);
        if (KR + KL > 0) {
            // L == 1, H <= NT: one LSTM layer, thread tid = hidden unit, R rows share every weight read
            const size_t G = 4 * (size_t)H;
            const float* h_old = hs + (size_t)par * R * H;
            float* h_new = hs + (size_t)(par ^ 1) * R * H;
            if (tid < H) {
                // the token-dependent row of P is only needed at the end of the chain: its L2 latency hides
                // behind the resident rows (the sum starts from the image half, which never changes)
                float4 a[R], acc[R];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    a[r] = *reinterpret_cast<const float4*>(w.P + (size_t)tok[r] * G + 4 * tid);
                    acc[r] = genc_reg[r];
                }
#pragma unroll
                for (int k4 = 0; k4 < KR; k4 += 4) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float4 xa = *reinterpret_cast<const float4*>(h_old + r * H + k4);
                        const float xv[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc[r].x = fmaf(wres[k4 + i].x, xv[i], acc[r].x);
                            acc[r].y = fmaf(wres[k4 + i].y, xv[i], acc[r].y);
                            acc[r].z = fmaf(wres[k4 + i].z, xv[i], acc[r].z);
                            acc[r].w = fmaf(wres[k4 + i].w, xv[i], acc[r].w);
                        }
                    }
                }
#pragma unroll 2
                for (int k4 = 0; k4 < KL; k4 += 4) {
                    float4 wv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) wv[i] = *reinterpret_cast<const float4*>(wl + (size_t)(k4 + i) * G + 4 * tid);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const float4 xa = *reinterpret_cast<const float4*>(h_old + r * H + KR + k4);
                        const float xv[4] = {xa.x, xa.y, xa.z, xa.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            acc[r].x = fmaf(wv[i].x, xv[i], acc[r].x);
                            acc[r].y = fmaf(wv[i].y, xv[i], acc[r].y);
                            acc[r].z = fmaf(wv[i].z, xv[i], acc[r].z);
                            acc[r].w = fmaf(wv[i].w, xv[i], acc[r].w);
                        }
                    }
                }
                matvec<R, float4>(acc, w.WhhT[0] + (size_t)(KR + KL) * G + 4 * tid, G, h_old + KR + KL, H, H - KR - KL);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    acc[r].x += a[r].x; acc[r].y += a[r].y; acc[r].z += a[r].z; acc[r].w += a[r].w;
                    const float ig = sigmoidf_(acc[r].x), fg = sigmoidf_(acc[r].y);
                    const float gg = tanhf_(acc[r].z), og = sigmoidf_(acc[r].w);
                    const float cn = fg * cs[r * H + tid] + ig * gg;
                    cs[r * H + tid] = cn;
                    h_new[r * H + tid] = og * tanhf_(cn);
                }
            }
            __syncthreads();
        } else {
            lstm_layers<R>(w, tok, grow, hs, cs, cs, par, tid);
        }

        // ---------------- output projection + token selection
        const float* h_top = hs + ((size_t)(par ^ 1) * L + (L - 1)) * R * H;
        float* lp[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
            lp[r] = (p.logits && row0 + r < B) ? p.logits + ((size_t)(row0 + r) * T + t) * V : nullptr;
        float best[R];
        int besti[R];
        if (KR + KL > 0)
            project<R, true>(w, h_top, lp, p.select != I2L_SELECT_LOGITS ? lg : nullptr, p.use_temp != 0,
                             p.temperature, best, besti, psum, tid, &pre);
        else
            project<R>(w, h_top, lp, p.select != I2L_SELECT_LOGITS ? lg : nullptr, p.use_temp != 0, p.temperature,
                       best, besti, psum, tid);
        block_argmax<R>(best, besti, redv, redi, tid);
        if (p.select == I2L_SELECT_SOFTMAX) {
            // argmax(softmax(x)): probabilities in fp32 as torch.softmax (exp(x - max) / sum), first index wins
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float s = 0.f;
                for (int v = tid; v < V; v += NT) s += expf(lg[r * w.Vp + v] - best[r]);
                s = wave_sum(s);
                if (lane == 0) redv[wave * R + r] = s;
            }
            __syncthreads();
            float pbest[R];
            int pbesti[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float s = 0.f;
#pragma unroll
                for (int wv = 0; wv < NT / 64; ++wv) s += redv[wv * R + r];
                pbest[r] = -1.f; pbesti[r] = 0x7fffffff;
                for (int v = tid; v < V; v += NT) {
                    const float pr = expf(lg[r * w.Vp + v] - best[r]) / s;
                    if (pr > pbest[r]) { pbest[r] = pr; pbesti[r] = v; }
                }
            }
            __syncthreads();
            block_argmax<R>(pbest, pbesti, redv, redi, tid);
#pragma unroll
            for (int r = 0; r < R; ++r) besti[r] = pbesti[r];
        }
        if (SAMPLE) {
            // predictor.py:295-331: probs = softmax(logits / T); top-k mask (keep p >= k-th largest); top-p mask
            // (drop a token once the probability mass sorted before it exceeds top_p); renormalise; one multinomial
            // draw by inverse CDF with a counter-based uniform of (seed, row, step).
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float* pr = lg + (size_t)r * w.Vp;
                float sm = 0.f;
                for (int v = tid; v < V; v += NT) sm += expf(pr[v] - best[r]);
                sm = block_sum(sm, redv, tid);
                for (int v = tid; v < V; v += NT) pr[v] = expf(pr[v] - best[r]) / sm;
                __syncthreads();
                if (p.top_k > 0) {
                    const int kk = min(p.top_k, V);
                    float kth = -1.f;
                    for (int v = tid; v < V; v += NT) {
                        const float pv = pr[v];
                        int gt = 0, ge = 0;
                        for (int u = 0; u < V; ++u) { const float pu = pr[u]; gt += pu > pv; ge += pu >= pv; }
                        if (gt < kk && kk <= ge) kth = pv;
                    }
                    kth = block_max(kth, redv, tid);
                    float s2 = 0.f;
                    for (int v = tid; v < V; v += NT) { const float q = pr[v] < kth ? 0.f : pr[v]; pr[v] = q; s2 += q; }
                    s2 = block_sum(s2, redv, tid);
                    if (s2 > 0.f) for (int v = tid; v < V; v += NT) pr[v] = pr[v] / s2;
                    __syncthreads();
                }
                if (p.top_p > 0.f) {
                    float* nx = lg + (size_t)(R + r) * w.Vp;         // second buffer: masked values
                    float s2 = 0.f;
                    for (int v = tid; v < V; v += NT) {
                        const float pv = pr[v];
                        float before = 0.f;                          // mass sorted ahead of v (descending, index breaks ties)
                        for (int u = 0; u < V; ++u) { const float pu = pr[u]; if (pu > pv || (pu == pv && u < v)) before += pu; }
                        const float q = before > p.top_p ? 0.f : pv;
                        nx[v] = q;
                        s2 += q;
                    }
                    __syncthreads();
                    for (int v = tid; v < V; v += NT) pr[v] = nx[v];
                    s2 = block_sum(s2, redv, tid);
                    if (s2 > 0.f) for (int v = tid; v < V; v += NT) pr[v] = pr[v] / s2;
                    __syncthreads();
                }
                if (p.probs && row0 + r < B) {
                    float* po = p.probs + ((size_t)(row0 + r) * T + t) * V;
                    for (int v = tid; v < V; v += NT) po[v] = pr[v];
                }
                // inverse CDF: thread t owns the contiguous chunk [t*CH, (t+1)*CH)
                const int CH = (V + NT - 1) / NT;
                float part = 0.f;
                for (int v = tid * CH; v < min(V, (tid + 1) * CH); ++v) part += pr[v];
                float* scan = psum;                                  // [NT] scratch (psum is free here)
                scan[tid] = part;
                __syncthreads();
                if (tid == 0) {
                    float run = 0.f;
                    for (int i = 0; i < NT; ++i) { const float x = scan[i]; scan[i] = run; run += x; }
                    scan[NT] = run;
                }
                __syncthreads();
                const float total = scan[NT];
                const float target = uniform01(p.seed, (unsigned)(row0 + r), (unsigned)t) * total;
                int pick = 0x7fffffff;
                float run = scan[tid];
                for (int v = tid * CH; v < min(V, (tid + 1) * CH); ++v) {
                    const float q = pr[v];
                    if (q > 0.f && run + q > target && pick == 0x7fffffff && run <= target) pick = v;
                    run += q;
                }
                float dummy = pick == 0x7fffffff ? -1.f : 1.f;
                int pk = pick;
                float bv[1] = {dummy};
                int bi[1] = {pk};
                block_argmax<1>(bv, bi, redv, redi, tid);            // the (unique) thread that found the crossing wins
                besti[r] = bi[0] < V ? bi[0] : besti[r];             // rounding corner: fall back to the arg max
            }
        }
        if (tid == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int row = row0 + r;
                const int sel = besti[r] < V ? besti[r] : 0;
                const int was_fin = fin_s[r];
                if (p.ids && row < B) p.ids[(size_t)row * T + t] = (p.stop == I2L_STOP_STICKY && was_fin) ? -1 : sel;
                tok_s[r] = sel;
                if (sel == p.end_id || row >= B) fin_s[r] = 1;
            }
        }
        __syncthreads();
        par ^= 1;
        if (p.stop == I2L_STOP_STICKY) {
            bool all = true;
#pragma unroll
            for (int r = 0; r < R; ++r) all = all && (fin_s[r] != 0);
            if (all) { ++t; break; }
        }
    }
    // steps never executed (sticky stop): ids = -1
    if (p.ids && t < T) {
        for (int idx = tid; idx < R * (T - t); idx += NT) {
            const int r = idx / (T - t), tt = t + (idx - r * (T - t));
            if (row0 + r < B) p.ids[(size_t)(row0 + r) * T + tt] = -1;
        }
    }
    if (p.h_out || p.c_out) {
        for (int idx = tid; idx < L * R * H; idx += NT) {
            const int l = idx / (R * H);
            const int rem = idx - l * (R * H);
            const int r = rem / H, j = rem - r * H;
            if (row0 + r < B) {
                const size_t g = ((size_t)l * B + row0 + r) * H + j;
                if (p.h_out) p.h_out[g] = hs[(size_t)par * L * R * H + idx];
                if (p.c_out) p.c_out[g] = cs[idx];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Beam search: one workgroup per image, K beams = K rows of the step (seq2seq.py:234-298 at B=1).
// The kernel is the decoder step (b), the gather (e) and the barriers; the search's decisions are shared with the
// step-batched kernels: phase (c) is beam_topk_row above, the serial rules (a), (d), (f) and the result are
// beam_rules.inc.h's, run by thread 0 on the LDS arrays below.
// ---------------------------------------------------------------------------------------------
struct BeamParams {
    StepWeights w;
    int images, T, start_id, end_id;
    int32_t* tokhist;    // [images][T][K]  token chosen for slot q at step t
    int32_t* parhist;    // [images][T][K]  slot (of step t-1) it extends
    int32_t* seq_out;    // [images][T+1]
    int32_t* len_out;    // [images]
    double* score_out;   // [images] or null
};

template <int K>
__global__ __launch_bounds__(NT) void beam_kernel(BeamParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const StepWeights& w = p.w;
    const int H = w.H, L = w.L, T = p.T, V = w.V, Vp = w.Vp;
    const int LKH = L * K * H;
    float* hs = smem;                                   // [2][L][K][H]
    float* cs = hs + 2 * LKH;                           // [2][L][K][H]
    float* lg = cs + 2 * LKH;                           // [K][Vp]
    float* psum = lg + (size_t)K * Vp;                  // [K][128][4]
    double* score = reinterpret_cast<double*>(psum + K * 512);   // [K]   (offset is a multiple of 8 bytes)
    double* nscore = score + K;                         // [K]
    float* topv = reinterpret_cast<float*>(nscore + K); // [K][K] log-probs, descending
    int* topi = reinterpret_cast<int*>(topv + K * K);   // [K][K]
    int* last = topi + K * K;                           // [K] last token of each beam
    int* live = last + K;                               // [K]
    int* npar = live + K;                               // [K] parent slot of the new beams
    int* ntok = npar + K;                               // [K]
    int* ctl = ntok + K;                                // [0] = the search has ended (thread 0's im.done, for all threads)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int img = blockIdx.x;
    int32_t* tokhist = p.tokhist + (size_t)img * T * K;
    int32_t* parhist = p.parhist + (size_t)img * T * K;

    for (int idx = tid; idx < 2 * LKH; idx += NT) { hs[idx] = 0.f; cs[idx] = 0.f; }
    // the image's record and the serial rules (beam_rules.inc.h) are thread 0's; (a) of step 0 here, of step t + 1 in
    // the ending of step t
    BeamImage im{};
    int nnew = 0;
    if (tid == 0) {
        beam_start(im, BeamBest{}, score, last, live, K, p.start_id, p.end_id);
        ctl[0] = im.done;
    }
    __syncthreads();

    const int par = 0, cpar = 0;
    for (int t = 0; t < T && !ctl[0]; ++t) {
        // (b) one decoder step for the K slots (retired / unused slots compute on a clamped token, ignored)
        int tok[K], grow[K];
#pragma unroll
        for (int r = 0; r < K; ++r) { tok[r] = min(max(last[r], 0), V - 1); grow[r] = img; }
        lstm_layers<K>(w, tok, grow, hs, cs + (size_t)cpar * LKH, cs + (size_t)(cpar ^ 1) * LKH, par, tid);
        const float* h_top = hs + ((size_t)(par ^ 1) * L + (L - 1)) * K * H;
        float* lp[K];
#pragma unroll
        for (int r = 0; r < K; ++r) lp[r] = nullptr;
        float best[K];
        int besti[K];
        project<K>(w, h_top, lp, lg, false, 1.f, best, besti, psum, tid);
        __syncthreads();

        // (c) log_softmax and top-K, a wave per live slot
        for (int r = wave; r < K; r += NT / 64)
            if (live[r]) beam_topk_row(lg + (size_t)r * Vp, V, K, lane, AllowAll{}, topv + r * K, topi + r * K);   // wave-uniform
        __syncthreads();

        // (d) the ranking of the K x K candidates and the history rows
        if (tid == 0)
            nnew = beam_rank(live, score, topv, topi, K, nullptr, npar, ntok, nscore, tokhist + (size_t)t * K, parhist + (size_t)t * K);
        __syncthreads();

        // (e) new beam q inherits the fresh state of its parent (hidden.clone(), :272): gather into the other buffers
        {
            const float* hsrc = hs + (size_t)(par ^ 1) * LKH;
            float* hdst = hs + (size_t)par * LKH;
            const float* csrc = cs + (size_t)(cpar ^ 1) * LKH;
            float* cdst = cs + (size_t)cpar * LKH;
            for (int idx = tid; idx < LKH; idx += NT) {
                const int l = idx / (K * H);
                const int rem = idx - l * (K * H);
                const int q = rem / H, j = rem - q * H;
                const size_t src = ((size_t)l * K + npar[q]) * H + j;
                hdst[idx] = hsrc[src];
                cdst[idx] = csrc[src];
            }
        }
        __syncthreads();
        // par / cpar unchanged: the gathered state sits in hs[par], cs[cpar] again
        // (f) the step's ending and (a) of the next step
        if (tid == 0) {
            beam_step_end(im, BeamBest{}, nnew, ntok, nscore, score, last, live, K, p.end_id, t, T);
            ctl[0] = im.done;
        }
        __syncthreads();
    }

    if (tid == 0) {
        double sc;
        p.len_out[img] = beam_best_result(im, score, tokhist, parhist, K, p.end_id, T, p.seq_out + (size_t)img * (T + 1), &sc);
        if (p.score_out) p.score_out[img] = sc;
    }
}

// The grouped greedy kernels, in the order launch_decode tries them.  A group is `rows` workgroups (one per member and
// row), the grid is padded to a multiple of 8 groups, and the exchange region is [groups padded to 8][xchg_per_group].
// The 16- and 8-member kernels run only when their flag asks for them and take ids only (no logits output, no forced
// tokens); the 4-member kernel takes every grouped greedy call.
struct GroupVariant {
    void (*kernel)(GroupParams);
    int flag;                 // I2L_FLAG_DECODE_GROUP16 / GROUP8; 0: the 4-member kernel
    int rows, threads;
    size_t lds, xchg_per_group;
};
constexpr int GROUP_VARIANTS = 3;
template <int M>   // decode_group_kernel<M> (decode_group.inc.h)
constexpr GroupVariant grouped_variant(int flag) {
    using S = GroupShape<M>;
    return {decode_group_kernel<M>, flag, M, S::NT, S::LDS, S::XCHG_PER_GROUP};
}
// (a table inside a function: the library keeps no data symbols beyond its attribute caches)
constexpr GroupVariant group_variant(int i) {
    constexpr GroupVariant table[GROUP_VARIANTS] = {
        // sixteen members x sixteen rows, the per-step products on the matrix cores (decode_group16.inc.h)
        {decode_group16_kernel<1>, I2L_FLAG_DECODE_GROUP16, G16Q, G16NT, GRP16_LDS, GROUP16_XCHG_PER_GROUP},
        // eight members x eight rows: one wave per SIMD and ~80 KB of LDS per CU, i.e. room for a conv workgroup beside it
        grouped_variant<8>(I2L_FLAG_DECODE_GROUP8),
        // four members x four rows (decode_group.inc.h)
        grouped_variant<4>(0),
    };
    return table[i];
}

struct Layout {
    size_t P, Genc, WhhT[MAXL], WihT[MAXL], biasP[MAXL], WoutT, boutP, wpack16, gemm_ws, xchg, xchg_bytes, state, state_bytes, total;
    int Vp;
};

Layout make_layout(int rows, int V, int E, int H, int L) {
    Layout o{};
    size_t off = 0;
    auto take = [&](size_t floats) { size_t r = off; off += i2l_align(floats * sizeof(float)); return r; };
    const size_t G = 4 * (size_t)H;
    o.Vp = i2l_cdiv(V, VCHUNK) * VCHUNK;
    o.P = take((size_t)V * G);
    o.Genc = take((size_t)rows * G);
    for (int l = 0; l < L; ++l) o.WhhT[l] = take((size_t)H * G);
    for (int l = 1; l < L; ++l) o.WihT[l] = take((size_t)H * G);
    for (int l = 1; l < L; ++l) o.biasP[l] = take(G);
    o.WoutT = take((size_t)H * o.Vp);
    o.boutP = take(o.Vp);
    // decode_group16_kernel: the weights pre-split into bf16 pieces in the matrix cores' operand layout, [member 16][wave 4]
    // [fragment 36][lane 64] x 16 bytes (weight-only: built with the other weight images under I2L_PREP_WEIGHTS)
    if (group_shape_ok(V, H, L)) o.wpack16 = take((size_t)16 * 4 * 36 * 64 * 4);
    size_t g1 = i2l_gemm_workspace_bytes(V, 4 * H, E), g2 = i2l_gemm_workspace_bytes(rows, 4 * H, E);
    o.gemm_ws = off;
    off += i2l_align(g1 > g2 ? g1 : g2);
    if (group_shape_ok(V, H, L)) {   // status block + the largest exchange region of the grouped greedy kernels
        o.xchg = off;
        size_t most = 0;
        for (int i = 0; i < GROUP_VARIANTS; ++i) {
            const GroupVariant g = group_variant(i);
            const size_t x = group_xchg_bytes(i2l_cdiv(rows, g.rows), g.xchg_per_group);
            most = x > most ? x : most;
        }
        // ... and of the two-tile launch (i2l_greedy_decode_halves), whose members exchange twice the granules
        const size_t x2 = group_xchg_bytes(i2l_cdiv(rows, G16Q), G16Shape<2>::XCHG_PER_GROUP);
        most = x2 > most ? x2 : most;
        o.xchg_bytes = GROUP_STATUS_BYTES + most;
        off += i2l_align(o.xchg_bytes);
        // what this batch's rows carry from the launch of their first steps to the launch of the others (G16State)
        o.state = off;
        o.state_bytes = group16_state_bytes(rows);
        off += i2l_align(o.state_bytes);
    }
    o.total = off;
    return o;
}

int check_weights(const i2l_decoder_weights* w) {
    if (!w || !w->embedding || !w->w_ih || !w->w_hh || !w->b_ih || !w->b_hh || !w->w_out || !w->b_out)
        return I2L_ERR_ARG;
    if (w->vocab <= 0 || w->embed <= 0 || w->hidden <= 0 || w->layers <= 0) return I2L_ERR_ARG;
    if (w->layers > MAXL || w->hidden % 64 != 0 || w->hidden > 2048 || w->embed % 4 != 0) return I2L_ERR_UNSUPPORTED;
    for (int l = 0; l < w->layers; ++l)
        if (!w->w_ih[l] || !w->w_hh[l] || !w->b_ih[l] || !w->b_hh[l]) return I2L_ERR_ARG;
    return I2L_OK;
}

StepWeights step_weights(const Layout& lo, const char* base, int V, int H, int L) {
    auto F = [&](size_t off) { return reinterpret_cast<const float*>(base + off); };
    StepWeights w{};
    w.H = H; w.L = L; w.V = V; w.Vp = lo.Vp;
    w.P = F(lo.P); w.Genc = F(lo.Genc);
    for (int l = 0; l < L; ++l) {
        w.WhhT[l] = F(lo.WhhT[l]);
        w.WihT[l] = l > 0 ? F(lo.WihT[l]) : nullptr;
        w.biasP[l] = l > 0 ? F(lo.biasP[l]) : nullptr;
    }
    w.WoutT = F(lo.WoutT); w.boutP = F(lo.boutP);
    w.wpack16 = lo.wpack16 ? base + lo.wpack16 : nullptr;
    return w;
}

constexpr int RES_KR = 76, RES_KL = 36;   // resident rows of WhhT[0]: registers / LDS (fast path)
constexpr int RES2_KR = 64, RES2_KL = 32; // same with two rows per workgroup (a few more live registers)

size_t decode_lds_bytes(int R, int L, int H, int Vp, int select, int KL = 0) {
    size_t floats = (size_t)3 * L * R * H + 4 * R + 4 * R + R + R + 4 + (size_t)R * 512 + (size_t)KL * 4 * H;
    if (select != I2L_SELECT_LOGITS) floats += (size_t)R * Vp;
    if (select == I2L_SELECT_SAMPLE) floats += (size_t)R * Vp;
    return floats * sizeof(float);
}

inline int use_temp(float temperature) { return temperature != 1.0f ? 1 : 0; }

// f(std::integral_constant<int, W>) for the W among Ws that equals `width`, so that a runtime width (a beam, the rows of
// a workgroup or of a tile) names a template argument; false, and no call, when there is none.  The kernels
// instantiated are exactly those of the list.
template <int... Ws, class F>
bool with_width(int width, F&& f) {
    return ((width == Ws && (f(std::integral_constant<int, Ws>{}), true)) || ...);
}

// The refusals the decode-loop entries share, each stated once and 0 (I2L_OK) when it passes: an entry chains the ones
// it needs with ||.  Their order is part of an entry's contract: it decides which code two bad arguments return.
inline int check_select(int select) {
    return select == I2L_SELECT_LOGITS || select == I2L_SELECT_SOFTMAX ? I2L_OK : I2L_ERR_ARG;
}
inline int check_loop(int rows, int steps) { return rows > 0 && steps > 0 ? I2L_OK : I2L_ERR_ARG; }
inline int check_sample(float temperature, int top_k, float top_p) {
    return sample_args_ok(temperature, top_k, top_p) ? I2L_OK : I2L_ERR_ARG;
}
inline int check_sample_vocab(int vocab) { return vocab > SB_MAXV ? I2L_ERR_UNSUPPORTED : I2L_OK; }

// A constrained selection: the rule set (I2L_CONSTRAIN_BRACKETS or _ARGUMENTS; 0, I2L_CONSTRAIN_NONE, is "absent"), its
// table and the rows' state.  THE place a rule set is added: its state size here, its rule object in with_rule.
struct Constraint {
    int kind;
    const uint8_t* cls;      // [V] table bytes
    void* state;             // [rows] BracketState or ArgumentState
    uint8_t* allowed;        // [rows][V] the allowed sets out, or null (the pick-logits entries)
};
inline size_t constraint_state_bytes(int kind, int rows) {
    const size_t row_bytes = kind == I2L_CONSTRAIN_ARGUMENTS ? sizeof(ArgumentState) : sizeof(BracketState);
    return rows > 0 ? (size_t)rows * row_bytes : 0;
}
// f(rule) with the rule object of c: NoRule, ConstrainRule or ArgumentRule
template <class F>
void with_rule(const Constraint& c, F&& f) {
    if (c.kind == I2L_CONSTRAIN_BRACKETS) f(ConstrainRule{c.cls, static_cast<BracketState*>(c.state), c.allowed});
    else if (c.kind == I2L_CONSTRAIN_ARGUMENTS) f(ArgumentRule{c.cls, static_cast<ArgumentState*>(c.state), c.allowed});
    else f(NoRule{});
}
// the constraint's own arguments; rows > 0 and vocab > 0 are checked before it
int check_constraint(int kind, int rows, int vocab, int end_id, const uint8_t* cls, const void* state, size_t state_bytes) {
    if (end_id < 0 || end_id >= vocab || !cls || !state) return I2L_ERR_ARG;
    if (state_bytes < constraint_state_bytes(kind, rows)) return I2L_ERR_WORKSPACE;
    return I2L_OK;
}

// What a caller asks of a decode loop, the row / grouped one (launch_decode) or the step-batched one (launch_batched):
// an entry zero-initialises the record and fills what it takes.  Null or 0 is "absent" throughout.
struct DecodeCall {
    const i2l_decoder_weights* w;
    const void* workspace;
    int rows, steps;
    int samples;                       // launch_batched: > 1: `samples` consecutive rows share an encoder row and a tok0 entry
    const int32_t *tok0, *forced;
    const float *h0, *c0;
    float temperature;
    int select, stop, end_id;
    SampleRule sample;                 // select == I2L_SELECT_SAMPLE: the masks, the seed, the probabilities out
    int32_t* ids_out;
    float *logits_out, *h_out, *c_out;
    int flags;
    uint32_t* resident_flag;
    uint32_t resident_value;
    i2l_stream_t stream;
    int rows_per_wg;                   // launch_decode: 0 = its own choice
    Constraint constraint;             // launch_batched: the constrained selection
    void* scratch;                     // launch_batched
    size_t scratch_bytes;
    // launch_batched, i2l_ensemble_decode only: the decoders, in the place of w, workspace, h0, c0, h_out and c_out
    const i2l_ensemble_member* members;
    int n_members, combine;
};

}  // namespace

extern "C" size_t i2l_decoder_workspace_bytes(int rows, int vocab, int embed, int hidden, int layers) {
    if (rows <= 0 || vocab <= 0 || embed <= 0 || hidden <= 0 || layers <= 0 || layers > MAXL) return 0;
    return make_layout(rows, vocab, embed, hidden, layers).total;
}

extern "C" int i2l_decoder_prepare(const i2l_decoder_weights* w, const float* enc, int rows, int what,
                                   void* workspace, size_t workspace_bytes, i2l_stream_t stream) {
    int rc = check_weights(w);
    if (rc != I2L_OK) return rc;
    if (rows <= 0 || (what & ~I2L_PREP_ALL) || what == 0) return I2L_ERR_ARG;
    if ((what & I2L_PREP_ROWS) && !enc) return I2L_ERR_ARG;
    const int V = w->vocab, E = w->embed, H = w->hidden, L = w->layers;
    const Layout lo = make_layout(rows, V, E, H, L);
    if (!workspace || workspace_bytes < lo.total) return I2L_ERR_WORKSPACE;
    char* base = static_cast<char*>(workspace);
    hipStream_t s = i2l_s(stream);
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    const int G = 4 * H;

    for (int l = 0; l < L && (what & I2L_PREP_WEIGHTS); ++l) {
        dim3 grid(i2l_cdiv(G, 64), i2l_cdiv(H, 64));
        hipLaunchKernelGGL(transpose_perm_kernel, grid, dim3(256), 0, s, w->w_hh[l], G, H, F(lo.WhhT[l]), G, G, H);
        I2L_CHECK_LAUNCH();
        if (l > 0) {
            hipLaunchKernelGGL(transpose_perm_kernel, grid, dim3(256), 0, s, w->w_ih[l], G, H, F(lo.WihT[l]), G, G, H);
            I2L_CHECK_LAUNCH();
            hipLaunchKernelGGL(bias_perm_kernel, dim3(i2l_cdiv(G, 256)), dim3(256), 0, s, w->b_ih[l], w->b_hh[l],
                               F(lo.biasP[l]), H);
            I2L_CHECK_LAUNCH();
        }
    }
    if (what & I2L_PREP_WEIGHTS) {
        dim3 grid(i2l_cdiv(lo.Vp, 64), i2l_cdiv(H, 64));
        hipLaunchKernelGGL(transpose_perm_kernel, grid, dim3(256), 0, s, w->w_out, V, H, F(lo.WoutT), lo.Vp, lo.Vp, 0);
        I2L_CHECK_LAUNCH();
        hipLaunchKernelGGL(bout_pad_kernel, dim3(i2l_cdiv(lo.Vp, 256)), dim3(256), 0, s, w->b_out, F(lo.boutP), V, lo.Vp);
        I2L_CHECK_LAUNCH();
        if (lo.wpack16) {
            hipLaunchKernelGGL(pack16_kernel, dim3(16 * 4), dim3(64), 0, s, F(lo.WhhT[0]), F(lo.WoutT),
                               reinterpret_cast<u32x4_t*>(base + lo.wpack16));
            I2L_CHECK_LAUNCH();
        }
    }
    const size_t gws = lo.total - lo.gemm_ws;
    if (what & I2L_PREP_WEIGHTS) {   // P = Emb @ W_ih_0[:, :E]^T, gate-interleaved columns
        GemmArgs g = gemm_args();
        g.A = w->embedding; g.lda = E;
        g.W = w->w_ih[0]; g.ldw = 2 * E;
        g.C = F(lo.P); g.ldc = G;
        g.M = V; g.N = G; g.K = E; g.perm_h = H;
        rc = i2l_gemm(g, base + lo.gemm_ws, gws, s);
        if (rc != I2L_OK) return rc;
    }
    if (what & I2L_PREP_ROWS) {   // Genc = enc @ W_ih_0[:, E:]^T + b_ih_0 + b_hh_0
        GemmArgs g = gemm_args();
        g.A = enc; g.lda = E;
        g.W = w->w_ih[0] + E; g.ldw = 2 * E;
        g.bias = w->b_ih[0]; g.bias2 = w->b_hh[0];
        g.C = F(lo.Genc); g.ldc = G;
        g.M = rows; g.N = G; g.K = E; g.perm_h = H;
        rc = i2l_gemm(g, base + lo.gemm_ws, gws, s);
        if (rc != I2L_OK) return rc;
    }
    return I2L_OK;
}

namespace {
// the residency signal of a launch that does NOT run a grouped kernel (other dimensions, row-per-workgroup request): its
// workgroups need no partners, so "resident" is said at once -- a waiter never pays its time-out for a kernel choice;
// like the grouped kernels it never moves the word backwards (publish_max32)
__global__ void publish_value32_kernel(unsigned* flag, unsigned value) { publish_max32(flag, value); }

// the persistent loop of i2l_greedy_decode[_ex] and i2l_sample_decode: a grouped kernel where one takes the call, else
// decode_kernel, one workgroup per a.rows_per_wg rows
int launch_decode(const DecodeCall& a) {
    int rc = check_weights(a.w);
    if (rc != I2L_OK) return rc;
    if (!a.workspace || !a.tok0 || check_loop(a.rows, a.steps)) return I2L_ERR_ARG;
    if ((a.h0 == nullptr) != (a.c0 == nullptr)) return I2L_ERR_ARG;
    if (a.stop != I2L_STOP_NONE && a.stop != I2L_STOP_STICKY) return I2L_ERR_ARG;
    const int rows = a.rows, steps = a.steps, select = a.select;
    const int V = a.w->vocab, E = a.w->embed, H = a.w->hidden, L = a.w->layers;
    const Layout lo = make_layout(rows, V, E, H, L);
    const char* base = static_cast<const char*>(a.workspace);

    DecodeParams p{};
    p.w = step_weights(lo, base, V, H, L);
    p.B = rows; p.T = steps;
    p.tok0 = a.tok0; p.forced = a.forced; p.h0 = a.h0; p.c0 = a.c0;
    p.h_out = a.h_out; p.c_out = a.c_out; p.ids = a.ids_out; p.logits = a.logits_out;
    p.temperature = a.temperature; p.use_temp = use_temp(a.temperature);
    p.select = select; p.stop = a.stop; p.end_id = a.end_id;
    p.top_k = a.sample.top_k; p.top_p = a.sample.top_p; p.seed = a.sample.seed; p.probs = a.sample.probs;

    // grouped kernels (group_variant): the workgroups of a group share its rows, weights fully on chip
    // I2L_SELECT_SOFTMAX takes them too: softmax is monotone, so its arg max is the logits' arg max unless fp32 rounding
    // makes two DIFFERENT scaled logits equal probabilities, which needs the two largest to be adjacent floats AND the
    // largest below 2 in magnitude (exp(x2 - x1) is then within 2 ulp of 1); the row-per-workgroup kernel evaluates
    // the probabilities literally and is one argument away (rows_per_workgroup != 0)
    if (a.rows_per_wg == 0 && lo.xchg_bytes && check_select(select) == I2L_OK && !a.h0 && !a.h_out && !a.c_out &&
        steps >= 8 && steps <= 65000) {   // the candidate granule carries step + 1 in 16 bits
        GroupParams gp{};
        gp.w = p.w; gp.B = rows; gp.T = steps;
        gp.tok0 = a.tok0; gp.forced = a.forced; gp.ids = a.ids_out; gp.logits = a.logits_out;
        gp.temperature = a.temperature; gp.use_temp = p.use_temp; gp.stop = a.stop; gp.end_id = a.end_id;
        char* xb = const_cast<char*>(base) + lo.xchg;           // scratch region of the workspace
        gp.status = reinterpret_cast<unsigned*>(xb);
        gp.xchg = reinterpret_cast<u64_t*>(xb + GROUP_STATUS_BYTES);
        gp.opts = group_opts(steps, a.flags);
        gp.resident_flag = a.resident_flag; gp.resident_value = a.resident_value;
        hipStream_t gs = i2l_s(a.stream);
        const bool ids_only = a.ids_out && !a.logits_out && !a.forced;
        static std::atomic<unsigned> attr[GROUP_VARIANTS]{};   // per variant and device
        for (int i = 0; i < GROUP_VARIANTS; ++i) {
            const GroupVariant g = group_variant(i);
            if (g.flag && !((a.flags & g.flag) && ids_only)) continue;
            if (!i2l_lds_attr(reinterpret_cast<const void*>(g.kernel), g.lds, attr[i])) continue;   // try the next one
            if (!(a.flags & I2L_FLAG_DECODE_REGION_CLEARED) && hipMemsetAsync(xb, 0, lo.xchg_bytes, gs) != hipSuccess) return I2L_ERR_LAUNCH;
            gp.n_groups = i2l_cdiv(rows, g.rows);
            hipLaunchKernelGGL(g.kernel, dim3(group_grid(gp.n_groups, g.rows)), dim3(g.threads), g.lds, gs, gp);
            I2L_CHECK_LAUNCH();
            return I2L_OK;
        }
    }
    hipStream_t s = i2l_s(a.stream);
    if (a.resident_flag) {
        hipLaunchKernelGGL(publish_value32_kernel, dim3(1), dim3(1), 0, s, a.resident_flag, a.resident_value);
        I2L_CHECK_LAUNCH();
    }
    // rows per workgroup: fill the 256 CUs first, then stack rows (weights are streamed once per workgroup per step)
    int R = rows <= 256 ? 1 : (rows <= 512 ? 2 : 4);
    if (a.rows_per_wg > 0) R = a.rows_per_wg;
    while (R > 1 && decode_lds_bytes(R, L, H, lo.Vp, select) > 64 * 1024) R >>= 1;
    const size_t lds = decode_lds_bytes(R, L, H, lo.Vp, select);
    if (lds > 64 * 1024) return I2L_ERR_UNSUPPORTED;
    const dim3 grid(i2l_cdiv(rows, R));
    const bool sampled = select == I2L_SELECT_SAMPLE;
    // fast path: weights partly resident on chip; pays a one-off fill, so only for real loops
    if (!sampled && (R == 1 || R == 2) && L == 1 && H == 256 && steps >= 8) {
        const size_t lds_r = decode_lds_bytes(R, 1, H, lo.Vp, select, R == 1 ? RES_KL : RES2_KL);
        auto kern = R == 1 ? decode_kernel<1, RES_KR, RES_KL> : decode_kernel<2, RES2_KR, RES2_KL>;
        if (lds_r <= 160 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_r) == hipSuccess) {
            hipLaunchKernelGGL(kern, grid, dim3(NT), lds_r, s, p);
            I2L_CHECK_LAUNCH();
            return I2L_OK;
        }
    }
    with_width<1, 2, 4>(R, [&](auto r) {
        if (sampled) hipLaunchKernelGGL((decode_kernel<r, 0, 0, true>), grid, dim3(NT), lds, s, p);
        else hipLaunchKernelGGL((decode_kernel<r, 0, 0>), grid, dim3(NT), lds, s, p);
    });
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
}  // namespace

extern "C" int i2l_greedy_decode_ex(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                    const int32_t* tok0, const int32_t* forced, const float* h0, const float* c0,
                                    float temperature, int select, int stop, int end_id, int rows_per_workgroup,
                                    int32_t* ids_out, float* logits_out, float* h_out, float* c_out, int flags,
                                    uint32_t* resident_flag, uint32_t resident_value, i2l_stream_t stream) {
    if (check_select(select)) return I2L_ERR_ARG;
    if (rows_per_workgroup != 0 && rows_per_workgroup != 1 && rows_per_workgroup != 2 && rows_per_workgroup != 4)
        return I2L_ERR_ARG;
    DecodeCall a{};
    a.w = w; a.workspace = workspace; a.rows = rows; a.steps = steps;
    a.tok0 = tok0; a.forced = forced; a.h0 = h0; a.c0 = c0;
    a.temperature = temperature; a.select = select; a.stop = stop; a.end_id = end_id;
    a.ids_out = ids_out; a.logits_out = logits_out; a.h_out = h_out; a.c_out = c_out;
    a.flags = flags; a.resident_flag = resident_flag; a.resident_value = resident_value; a.stream = stream;
    a.rows_per_wg = rows_per_workgroup;
    return launch_decode(a);
}

extern "C" int i2l_greedy_decode(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                 const int32_t* tok0, const int32_t* forced, const float* h0, const float* c0,
                                 float temperature, int select, int stop, int end_id, int32_t* ids_out,
                                 float* logits_out, float* h_out, float* c_out, i2l_stream_t stream) {
    return i2l_greedy_decode_ex(w, workspace, rows, steps, tok0, forced, h0, c0, temperature, select, stop, end_id, 0,
                                ids_out, logits_out, h_out, c_out, 0, nullptr, 0, stream);
}

extern "C" int i2l_sample_decode(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                 const int32_t* tok0, const float* h0, const float* c0, float temperature, int top_k,
                                 float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out, float* probs_out,
                                 float* h_out, float* c_out, i2l_stream_t stream) {
    int rc;
    if ((rc = check_sample(temperature, top_k, top_p)) || (rc = w ? check_sample_vocab(w->vocab) : I2L_OK)) return rc;
    DecodeCall a{};
    a.w = w; a.workspace = workspace; a.rows = rows; a.steps = steps;
    a.tok0 = tok0; a.h0 = h0; a.c0 = c0;
    a.temperature = temperature; a.select = I2L_SELECT_SAMPLE; a.stop = stop; a.end_id = end_id;
    a.sample = SampleRule{top_k, top_p, (unsigned long long)seed, probs_out};
    a.ids_out = ids_out; a.h_out = h_out; a.c_out = c_out; a.stream = stream;
    return launch_decode(a);
}

// ---------------------------------------------------------------------------------------------
// Two batches per 16-member grouped launch, a range of the steps of each (decode_group16_kernel<2>).
// ---------------------------------------------------------------------------------------------
namespace {
int check_half(const i2l_decode_half* h) {
    if (!h) return I2L_OK;
    if (!h->workspace || !h->tok0 || !h->ids_out || h->rows <= 0 || h->steps <= 0) return I2L_ERR_ARG;
    if (h->first_step < 0 || h->n_steps < 0 || h->first_step > h->steps - h->n_steps) return I2L_ERR_ARG;
    if (h->steps > 65000) return I2L_ERR_UNSUPPORTED;         // the candidate granule carries step + 1 in 16 bits
    return I2L_OK;
}
}  // namespace

extern "C" int i2l_greedy_decode_halves(const i2l_decoder_weights* w, const i2l_decode_half* older,
                                        const i2l_decode_half* newer, float temperature, int select, int stop, int end_id,
                                        int flags, uint32_t* resident_flag, uint32_t resident_value, i2l_stream_t stream) {
    // every refusal is decided here, before the first HIP call
    int rc = check_weights(w);
    if (rc != I2L_OK) return rc;
    if (select != I2L_SELECT_LOGITS && select != I2L_SELECT_SOFTMAX) return I2L_ERR_ARG;
    if (stop != I2L_STOP_NONE && stop != I2L_STOP_STICKY) return I2L_ERR_ARG;
    if ((rc = check_half(older)) != I2L_OK || (rc = check_half(newer)) != I2L_OK) return rc;
    const int V = w->vocab, E = w->embed, H = w->hidden, L = w->layers;
    // with a sticky stop a range of steps has no fixed length; other dimensions have no 16-member kernel
    if (stop != I2L_STOP_NONE || !group_shape_ok(V, H, L)) return I2L_ERR_UNSUPPORTED;
    const i2l_decode_half* half[2] = {older && older->n_steps > 0 ? older : nullptr, newer && newer->n_steps > 0 ? newer : nullptr};
    hipStream_t s = i2l_s(stream);
    if (!half[0] && !half[1]) {                               // no step to run: nothing waits for a partner
        if (resident_flag) {
            hipLaunchKernelGGL(publish_value32_kernel, dim3(1), dim3(1), 0, s, resident_flag, resident_value);
            I2L_CHECK_LAUNCH();
        }
        return I2L_OK;
    }
    // weights, status block and exchange region: the newer batch's workspace (the one a pipeline has just prepared and
    // cleared), the older one's when there is no newer batch; the region must hold the groups of BOTH
    const i2l_decode_half* home = half[1] ? half[1] : half[0];
    const Layout lo = make_layout(home->rows, V, E, H, L);
    int n_groups = 0, most_steps = 0;
    for (int k = 0; k < 2; ++k)
        if (half[k]) {
            n_groups = std::max(n_groups, i2l_cdiv(half[k]->rows, G16Q));
            most_steps = std::max(most_steps, half[k]->n_steps);
        }
    if (!lo.wpack16 || GROUP_STATUS_BYTES + group_xchg_bytes(n_groups, G16Shape<2>::XCHG_PER_GROUP) > lo.xchg_bytes)
        return I2L_ERR_UNSUPPORTED;
    char* base = static_cast<char*>(const_cast<void*>(home->workspace));

    GroupParams gp{};
    gp.w = step_weights(lo, base, V, H, L);
    gp.n_groups = n_groups;
    gp.temperature = temperature; gp.use_temp = use_temp(temperature); gp.stop = stop; gp.end_id = end_id;
    char* xb = base + lo.xchg;
    gp.status = reinterpret_cast<unsigned*>(xb);
    gp.xchg = reinterpret_cast<u64_t*>(xb + GROUP_STATUS_BYTES);
    gp.opts = group_opts(most_steps, flags);
    gp.resident_flag = resident_flag; gp.resident_value = resident_value;
    for (int k = 0; k < 2; ++k) {
        HalfTile& t = gp.tile[k];
        if (!half[k]) continue;                               // n = 0: absent
        const i2l_decode_half& h = *half[k];
        const Layout hl = make_layout(h.rows, V, E, H, L);
        char* hb = static_cast<char*>(const_cast<void*>(h.workspace));
        t.Genc = reinterpret_cast<const float*>(hb + hl.Genc);
        t.tok0 = h.tok0; t.ids = h.ids_out; t.B = h.rows; t.T = h.steps; t.t0 = h.first_step; t.n = h.n_steps;
        t.state_in = h.first_step > 0 ? hb + hl.state : nullptr;
        t.state_out = h.first_step + h.n_steps < h.steps ? hb + hl.state : nullptr;
    }
    static std::atomic<unsigned> attr{};
    if (!i2l_lds_attr(reinterpret_cast<const void*>(decode_group16_kernel<2>), G16Shape<2>::LDS, attr)) return I2L_ERR_UNSUPPORTED;
    if (!(flags & I2L_FLAG_DECODE_REGION_CLEARED) && hipMemsetAsync(xb, 0, lo.xchg_bytes, s) != hipSuccess) return I2L_ERR_LAUNCH;
    hipLaunchKernelGGL(decode_group16_kernel<2>, dim3(group_grid(n_groups, G16Q)), dim3(G16NT), G16Shape<2>::LDS, s, gp);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

// ---------------------------------------------------------------------------------------------
// Step-batched greedy decode (decode_batched.inc.h): L + 2 plain launches per step on the caller's stream.
// ---------------------------------------------------------------------------------------------
extern "C" size_t i2l_decode_batched_scratch_bytes(int rows, int vocab, int hidden, int layers) {
    if (!batched_dims_ok(rows, vocab, hidden, layers)) return 0;
    return batched_layout(rows, i2l_cdiv(vocab, VCHUNK) * VCHUNK, hidden, layers).total;
}

namespace {
template <int TB>
void launch_batched_lstm(const BatchedParams& p, int t, hipStream_t s) {
    for (int l = 0; l < p.w.L; ++l)
        hipLaunchKernelGGL(lstm_step_mfma_kernel<TB>, dim3(p.w.H / 16, i2l_cdiv(p.B, TB)), dim3(DB_NT), 0, s, p, l, t);
}
template <int TB>
void launch_batched_logits(const BatchedParams& p, int t, hipStream_t s) {
    hipLaunchKernelGGL(logits_mfma_kernel<TB>, dim3(p.w.Vp / DB_COLS, i2l_cdiv(p.B, TB)), dim3(DB_NT), 0, s, p, t);
}
// the L LSTM launches and the logits launch of step t on p's rows; tb_*: batched_tile_rows of either grid
void launch_batched_step(const BatchedParams& p, int tb_lstm, int tb_logits, int t, hipStream_t s) {
    with_width<16, 32, 64>(tb_lstm, [&](auto tb) { launch_batched_lstm<tb>(p, t, s); });
    with_width<16, 32, 64>(tb_logits, [&](auto tb) { launch_batched_logits<tb>(p, t, s); });
}

// the last launch of a step: the arg max, or the draw when the call samples, under the rule's pick policy
template <class Rule>
void launch_batched_select(const BatchedParams& p, const DecodeCall& a, const Rule& rule, int t, hipStream_t s) {
    if (a.select == I2L_SELECT_SAMPLE && a.sample.score)
        hipLaunchKernelGGL((sample_batched_kernel<Rule, true>), dim3(p.B), dim3(NT), 0, s, p, a.sample, rule, t);
    else if (a.select == I2L_SELECT_SAMPLE)
        hipLaunchKernelGGL(sample_batched_kernel<Rule>, dim3(p.B), dim3(NT), 0, s, p, a.sample, rule, t);
    else
        hipLaunchKernelGGL(select_batched_kernel<Rule>, dim3(i2l_cdiv(p.B, DB_NT / 64)), dim3(DB_NT), 0, s, p, rule, t);
}

#include "decode_ensemble.inc.h"

// THE loop of the step-batched entries, for one decoder (a.w .. a.c_out) or an ensemble's (a.members): every member
// runs its own recurrences and logits on its own batched_layout slice of the scratch, tok / fin / live are member 0's,
// and ONE selection picks per step -- from member 0's logits, or for n > 1 from the combined rows behind the slices.  A
// single-decoder entry's scratch is batched_layout's alone, an ensemble's has the combined buffer whatever n is.  The
// caller has checked the weights and its own arguments; every other refusal is decided here, before the first HIP
// call.  A constrained call starts from the rows' zeroed state.
int launch_batched(const DecodeCall& a) {
    const i2l_ensemble_member self{a.w, a.workspace, a.h0, a.c0, a.h_out, a.c_out, 1.f};
    const i2l_ensemble_member* members = a.members ? a.members : &self;
    const int n = a.members ? a.n_members : 1, rows = a.rows, steps = a.steps;
    const int per = a.samples > 1 ? a.samples : 1;              // rows of one encoder row (the workspace's: rows / per)
    if (!a.tok0 || check_loop(rows, steps)) return I2L_ERR_ARG;
    if (a.stop != I2L_STOP_NONE && a.stop != I2L_STOP_STICKY) return I2L_ERR_ARG;
    float weight[ENS_MAX];
    for (int m = 0; m < n; ++m) {
        const i2l_ensemble_member& mem = members[m];
        if (!mem.workspace || (mem.h0 == nullptr) != (mem.c0 == nullptr) || !ens_weight_ok(mem.weight)) return I2L_ERR_ARG;
        weight[m] = mem.weight;
    }
    const int V = members[0].w->vocab, Vp = i2l_cdiv(V, VCHUNK) * VCHUNK;
    const EnsembleLayout el = ensemble_layout(members, n, rows, Vp);
    if (!a.scratch || a.scratch_bytes < (a.members ? el.total : el.combined)) return I2L_ERR_WORKSPACE;

    char* sb = static_cast<char*>(a.scratch);
    BatchedParams p[ENS_MAX];
    int tb_lstm[ENS_MAX], tb_logits[ENS_MAX], copy_grid[ENS_MAX];
    EnsembleRows e{};
    for (int m = 0; m < n; ++m) {
        const i2l_decoder_weights& w = *members[m].w;
        const Layout lo = make_layout(rows / per, V, w.embed, w.hidden, w.layers);
        const BatchedLayout bl = batched_layout(rows, Vp, w.hidden, w.layers);
        char* mb = sb + el.member[m];
        BatchedParams& q = p[m];
        q = BatchedParams{};
        q.w = step_weights(lo, static_cast<const char*>(members[m].workspace), V, w.hidden, w.layers);
        q.B = rows; q.T = steps; q.genc_div = per; q.forced = a.forced;
        q.h = reinterpret_cast<float*>(mb + bl.h); q.c = reinterpret_cast<float*>(mb + bl.c);
        q.lg = reinterpret_cast<float*>(mb + bl.lg);
        // tok, fin and live are member 0's words for every member; ids and the distribution belong to the selection
        q.tok = m ? p[0].tok : reinterpret_cast<int*>(mb + bl.tok);
        q.fin = m ? p[0].fin : reinterpret_cast<int*>(mb + bl.fin);
        q.live = m ? p[0].live : reinterpret_cast<unsigned*>(mb + bl.live);
        q.temperature = a.temperature; q.use_temp = use_temp(a.temperature);
        q.select = a.select; q.stop = a.stop; q.end_id = a.end_id;
        tb_lstm[m] = batched_tile_rows(w.hidden / 16, rows);
        tb_logits[m] = batched_tile_rows(Vp / DB_COLS, rows);
        const size_t LBH = (size_t)w.layers * rows * w.hidden, BT = (size_t)rows * steps;
        const size_t most = LBH > BT ? LBH : BT, copy_blocks = (most + DB_NT - 1) / DB_NT;
        copy_grid[m] = (int)(copy_blocks < 1024 ? copy_blocks : 1024);
        e.lg[m] = q.lg; e.ld[m] = Vp;
    }
    p[0].ids = a.ids_out; p[0].logits_out = a.logits_out;
    BatchedParams pe = p[0];                                    // the selection's: member 0's, the combined rows for n > 1
    if (n > 1) {
        pe.lg = reinterpret_cast<float*>(sb + el.combined);
        ens_normalise(weight, n, e.w, e.logw);
        e.out = pe.lg; e.ld_out = Vp; e.B = rows; e.V = V; e.rule = a.combine; e.live = pe.live;
    }

    hipStream_t s = i2l_s(a.stream);
    if (a.resident_flag) {      // nothing here waits for a partner: "resident" is said at once
        hipLaunchKernelGGL(publish_value32_kernel, dim3(1), dim3(1), 0, s, a.resident_flag, a.resident_value);
        I2L_CHECK_LAUNCH();
    }
    const Constraint& con = a.constraint;
    if (con.kind != I2L_CONSTRAIN_NONE && hipMemsetAsync(con.state, 0, constraint_state_bytes(con.kind, rows), s) != hipSuccess)
        return I2L_ERR_LAUNCH;
    for (int m = 0; m < n; ++m) {
        hipLaunchKernelGGL(init_batched_kernel, dim3(copy_grid[m]), dim3(DB_NT), 0, s, p[m], a.tok0, members[m].h0, members[m].c0);
        I2L_CHECK_LAUNCH();
    }
    for (int t = 0; t < steps; ++t) {
        for (int m = 0; m < n; ++m) launch_batched_step(p[m], tb_lstm[m], tb_logits[m], t, s);
        if (n > 1)
            with_width<2, 3, 4, 5, 6, 7, 8>(n, [&](auto M) {
                hipLaunchKernelGGL(ensemble_combine_kernel<M>, dim3(i2l_cdiv(rows, DB_NT / 64)), dim3(DB_NT), 0, s, e);
            });
        with_rule(con, [&](const auto& rule) { launch_batched_select(pe, a, rule, t, s); });
        I2L_CHECK_LAUNCH();
    }
    for (int m = 0; m < n; ++m)
        if (members[m].h_out || members[m].c_out) {
            hipLaunchKernelGGL(state_out_batched_kernel, dim3(copy_grid[m]), dim3(DB_NT), 0, s, p[m], members[m].h_out,
                               members[m].c_out);
            I2L_CHECK_LAUNCH();
        }
    return I2L_OK;
}
}  // namespace

extern "C" int i2l_greedy_decode_batched(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                         const int32_t* tok0, const int32_t* forced, const float* h0, const float* c0,
                                         float temperature, int select, int stop, int end_id, int32_t* ids_out,
                                         float* logits_out, float* h_out, float* c_out, void* scratch,
                                         size_t scratch_bytes, int flags, uint32_t* resident_flag,
                                         uint32_t resident_value, i2l_stream_t stream) {
    int rc;
    if ((rc = check_weights(w)) || (rc = check_select(select))) return rc;
    DecodeCall a{};
    a.w = w; a.workspace = workspace; a.rows = rows; a.steps = steps;
    a.tok0 = tok0; a.forced = forced; a.h0 = h0; a.c0 = c0;
    a.temperature = temperature; a.select = select; a.stop = stop; a.end_id = end_id;
    a.ids_out = ids_out; a.logits_out = logits_out; a.h_out = h_out; a.c_out = c_out;
    a.flags = flags; a.resident_flag = resident_flag; a.resident_value = resident_value; a.stream = stream;
    a.scratch = scratch; a.scratch_bytes = scratch_bytes;
    return launch_batched(a);
}

// ---------------------------------------------------------------------------------------------
// Step-batched sampling (sample_batched.inc.h): the same loop, sample_batched_kernel as the last launch of a step.
// Every refusal is decided on the host, here and in launch_batched, before the first HIP call.
// ---------------------------------------------------------------------------------------------
extern "C" int i2l_sample_decode_batched(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                         const int32_t* tok0, const float* h0, const float* c0, float temperature,
                                         int top_k, float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out,
                                         float* probs_out, float* h_out, float* c_out, void* scratch,
                                         size_t scratch_bytes, int flags, i2l_stream_t stream) {
    int rc;
    if ((rc = check_weights(w)) || (rc = check_sample(temperature, top_k, top_p)) || (rc = check_loop(rows, steps)) ||
        (rc = check_sample_vocab(w->vocab)))
        return rc;
    DecodeCall a{};
    a.w = w; a.workspace = workspace; a.rows = rows; a.steps = steps;
    a.tok0 = tok0; a.h0 = h0; a.c0 = c0;
    a.temperature = temperature; a.select = I2L_SELECT_SAMPLE; a.stop = stop; a.end_id = end_id;
    a.sample = SampleRule{top_k, top_p, (unsigned long long)seed, probs_out};
    a.ids_out = ids_out; a.h_out = h_out; a.c_out = c_out; a.flags = flags; a.stream = stream;
    a.scratch = scratch; a.scratch_bytes = scratch_bytes;
    return launch_batched(a);
}

extern "C" int i2l_sample_logits(const float* logits, int ld, int rows, int vocab, float temperature, int top_k,
                                 float top_p, uint64_t seed, int step, int32_t* ids_out, float* probs_out,
                                 i2l_stream_t stream) {
    int rc;
    if ((rc = check_sample(temperature, top_k, top_p))) return rc;
    if (rows <= 0 || vocab <= 0 || ld < vocab || step < 0) return I2L_ERR_ARG;
    if ((rc = check_sample_vocab(vocab))) return rc;
    if (!logits || !ids_out) return I2L_ERR_ARG;
    const SampleRule rule{top_k, top_p, (unsigned long long)seed, probs_out};
    hipLaunchKernelGGL(sample_logits_kernel<NoRule>, dim3(rows), dim3(NT), 0, i2l_s(stream), logits, ld, vocab, temperature,
                       use_temp(temperature), rule, (unsigned)step, NoRule{}, 0, 0, ids_out);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

// ---------------------------------------------------------------------------------------------
// Constrained step-batched decode (bracket_rules.inc.h, argument_rules.inc.h, decode_constrained.inc.h): the same loop,
// the selection kernels under ConstrainRule or ArgumentRule as the last launch of a step.  The ..._constrained entries
// (groups nest; 16 bytes of caller-owned state per row) and the ..._arguments ones (and every command gets the arguments
// it demands; 32 bytes) are one body each, taking the kind, with the same argument lists and the same refusals.  Every
// refusal is decided on the host, here and in launch_batched, before the first HIP call; the library keeps no state.
// ---------------------------------------------------------------------------------------------
namespace {
int greedy_decode_constrained(int kind, const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                              const int32_t* tok0, const float* h0, const float* c0, float temperature, int select, int stop,
                              int end_id, int32_t* ids_out, float* logits_out, float* h_out, float* c_out, void* scratch,
                              size_t scratch_bytes, int flags, uint32_t* resident_flag, uint32_t resident_value,
                              const uint8_t* cls, void* state, size_t state_bytes, i2l_stream_t stream) {
    int rc;
    if ((rc = check_weights(w)) || (rc = check_select(select)) || (rc = check_loop(rows, steps)) ||
        (rc = check_constraint(kind, rows, w->vocab, end_id, cls, state, state_bytes)))
        return rc;
    DecodeCall a{};
    a.w = w; a.workspace = workspace; a.rows = rows; a.steps = steps;
    a.tok0 = tok0; a.h0 = h0; a.c0 = c0;
    a.temperature = temperature; a.select = select; a.stop = stop; a.end_id = end_id;
    a.ids_out = ids_out; a.logits_out = logits_out; a.h_out = h_out; a.c_out = c_out;
    a.flags = flags; a.resident_flag = resident_flag; a.resident_value = resident_value; a.stream = stream;
    a.constraint = Constraint{kind, cls, state, nullptr};
    a.scratch = scratch; a.scratch_bytes = scratch_bytes;
    return launch_batched(a);
}

int sample_decode_constrained(int kind, const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                              const int32_t* tok0, const float* h0, const float* c0, float temperature, int top_k,
                              float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out, float* probs_out,
                              float* h_out, float* c_out, void* scratch, size_t scratch_bytes, int flags,
                              const uint8_t* cls, void* state, size_t state_bytes, i2l_stream_t stream) {
    int rc;
    if ((rc = check_weights(w)) || (rc = check_sample(temperature, top_k, top_p)) || (rc = check_loop(rows, steps)) ||
        (rc = check_sample_vocab(w->vocab)) ||
        (rc = check_constraint(kind, rows, w->vocab, end_id, cls, state, state_bytes)))
        return rc;
    DecodeCall a{};
    a.w = w; a.workspace = workspace; a.rows = rows; a.steps = steps;
    a.tok0 = tok0; a.h0 = h0; a.c0 = c0;
    a.temperature = temperature; a.select = I2L_SELECT_SAMPLE; a.stop = stop; a.end_id = end_id;
    a.sample = SampleRule{top_k, top_p, (unsigned long long)seed, probs_out};
    a.ids_out = ids_out; a.h_out = h_out; a.c_out = c_out; a.flags = flags; a.stream = stream;
    a.constraint = Constraint{kind, cls, state, nullptr};
    a.scratch = scratch; a.scratch_bytes = scratch_bytes;
    return launch_batched(a);
}

int constrained_pick_logits(int kind, const float* logits, int ld, int rows, int vocab, float temperature, int select,
                            int top_k, float top_p, uint64_t seed, int step, int steps, const uint8_t* cls, int end_id,
                            void* state, int32_t* ids_out, float* probs_out, uint8_t* allowed_out, i2l_stream_t stream) {
    const bool greedy = top_k == 0 && top_p == 0.f;
    if (!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f)) return I2L_ERR_ARG;
    if (greedy && check_select(select)) return I2L_ERR_ARG;
    if (rows <= 0 || vocab <= 0 || ld < vocab || step < 0 || steps <= 0 || step >= steps) return I2L_ERR_ARG;
    if (!greedy && check_sample_vocab(vocab)) return I2L_ERR_UNSUPPORTED;
    if (!logits || !ids_out || end_id < 0 || end_id >= vocab || !cls || !state) return I2L_ERR_ARG;
    const int rem = steps - step - 1;
    with_rule(Constraint{kind, cls, state, allowed_out}, [&](const auto& rule) {
        using Rule = std::decay_t<decltype(rule)>;
        if constexpr (!std::is_same_v<Rule, NoRule>) {      // the kind is one of the two: no plain pick kernel exists
            if (greedy) {
                hipLaunchKernelGGL(pick_select_kernel<Rule>, dim3(i2l_cdiv(rows, DB_NT / 64)), dim3(DB_NT), 0, i2l_s(stream),
                                   logits, ld, rows, vocab, temperature, use_temp(temperature), select, rule, end_id, rem,
                                   ids_out);
            } else {
                const SampleRule sample{top_k, top_p, (unsigned long long)seed, probs_out};
                hipLaunchKernelGGL(sample_logits_kernel<Rule>, dim3(rows), dim3(NT), 0, i2l_s(stream), logits, ld, vocab,
                                   temperature, use_temp(temperature), sample, (unsigned)step, rule, end_id, rem, ids_out);
            }
        }
    });
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
}  // namespace

extern "C" size_t i2l_bracket_state_bytes(int rows) { return constraint_state_bytes(I2L_CONSTRAIN_BRACKETS, rows); }
extern "C" size_t i2l_argument_state_bytes(int rows) { return constraint_state_bytes(I2L_CONSTRAIN_ARGUMENTS, rows); }

extern "C" int i2l_greedy_decode_constrained(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                             const int32_t* tok0, const float* h0, const float* c0, float temperature,
                                             int select, int stop, int end_id, int32_t* ids_out, float* logits_out,
                                             float* h_out, float* c_out, void* scratch, size_t scratch_bytes, int flags,
                                             uint32_t* resident_flag, uint32_t resident_value, const uint8_t* cls,
                                             void* state, size_t state_bytes, i2l_stream_t stream) {
    return greedy_decode_constrained(I2L_CONSTRAIN_BRACKETS, w, workspace, rows, steps, tok0, h0, c0, temperature, select, stop,
                                     end_id, ids_out, logits_out, h_out, c_out, scratch, scratch_bytes, flags, resident_flag,
                                     resident_value, cls, state, state_bytes, stream);
}
extern "C" int i2l_greedy_decode_arguments(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                           const int32_t* tok0, const float* h0, const float* c0, float temperature,
                                           int select, int stop, int end_id, int32_t* ids_out, float* logits_out,
                                           float* h_out, float* c_out, void* scratch, size_t scratch_bytes, int flags,
                                           uint32_t* resident_flag, uint32_t resident_value, const uint8_t* cls,
                                           void* state, size_t state_bytes, i2l_stream_t stream) {
    return greedy_decode_constrained(I2L_CONSTRAIN_ARGUMENTS, w, workspace, rows, steps, tok0, h0, c0, temperature, select, stop,
                                     end_id, ids_out, logits_out, h_out, c_out, scratch, scratch_bytes, flags, resident_flag,
                                     resident_value, cls, state, state_bytes, stream);
}

extern "C" int i2l_sample_decode_constrained(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                             const int32_t* tok0, const float* h0, const float* c0, float temperature,
                                             int top_k, float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out,
                                             float* probs_out, float* h_out, float* c_out, void* scratch,
                                             size_t scratch_bytes, int flags, const uint8_t* cls, void* state,
                                             size_t state_bytes, i2l_stream_t stream) {
    return sample_decode_constrained(I2L_CONSTRAIN_BRACKETS, w, workspace, rows, steps, tok0, h0, c0, temperature, top_k, top_p,
                                     seed, stop, end_id, ids_out, probs_out, h_out, c_out, scratch, scratch_bytes, flags, cls,
                                     state, state_bytes, stream);
}
extern "C" int i2l_sample_decode_arguments(const i2l_decoder_weights* w, const void* workspace, int rows, int steps,
                                           const int32_t* tok0, const float* h0, const float* c0, float temperature,
                                           int top_k, float top_p, uint64_t seed, int stop, int end_id, int32_t* ids_out,
                                           float* probs_out, float* h_out, float* c_out, void* scratch,
                                           size_t scratch_bytes, int flags, const uint8_t* cls, void* state,
                                           size_t state_bytes, i2l_stream_t stream) {
    return sample_decode_constrained(I2L_CONSTRAIN_ARGUMENTS, w, workspace, rows, steps, tok0, h0, c0, temperature, top_k, top_p,
                                     seed, stop, end_id, ids_out, probs_out, h_out, c_out, scratch, scratch_bytes, flags, cls,
                                     state, state_bytes, stream);
}

extern "C" int i2l_constrained_pick_logits(const float* logits, int ld, int rows, int vocab, float temperature, int select,
                                           int top_k, float top_p, uint64_t seed, int step, int steps, const uint8_t* cls,
                                           int end_id, void* state, int32_t* ids_out, float* probs_out,
                                           uint8_t* allowed_out, i2l_stream_t stream) {
    return constrained_pick_logits(I2L_CONSTRAIN_BRACKETS, logits, ld, rows, vocab, temperature, select, top_k, top_p, seed, step,
                                   steps, cls, end_id, state, ids_out, probs_out, allowed_out, stream);
}
extern "C" int i2l_arguments_pick_logits(const float* logits, int ld, int rows, int vocab, float temperature, int select,
                                         int top_k, float top_p, uint64_t seed, int step, int steps, const uint8_t* cls,
                                         int end_id, void* state, int32_t* ids_out, float* probs_out,
                                         uint8_t* allowed_out, i2l_stream_t stream) {
    return constrained_pick_logits(I2L_CONSTRAIN_ARGUMENTS, logits, ld, rows, vocab, temperature, select, top_k, top_p, seed, step,
                                   steps, cls, end_id, state, ids_out, probs_out, allowed_out, stream);
}

// ---------------------------------------------------------------------------------------------
// Ensemble decode (ensemble_rules.inc.h, decode_ensemble.inc.h; this package): the step-batched loop over M decoders of
// one vocabulary, one combine launch per step, the selection kernels above on the combined row.  Every refusal is
// decided on the host, here and in launch_batched, before the first HIP call; the library keeps no state.
// ---------------------------------------------------------------------------------------------
extern "C" size_t i2l_ensemble_scratch_bytes(const i2l_ensemble_member* members, int n, int rows) {
    if (check_members(members, n) != I2L_OK) return 0;
    for (int m = 0; m < n; ++m)
        if (!batched_dims_ok(rows, members[m].w->vocab, members[m].w->hidden, members[m].w->layers)) return 0;
    return ensemble_layout(members, n, rows, i2l_cdiv(members[0].w->vocab, VCHUNK) * VCHUNK).total;
}

extern "C" int i2l_ensemble_decode(const i2l_ensemble_member* members, int n, int combine, int rows, int steps,
                                   const int32_t* tok0, const int32_t* forced, float temperature, int select, int top_k,
                                   float top_p, uint64_t seed, int stop, int end_id, const uint8_t* cls, int cls_kind,
                                   void* state, size_t state_bytes, int32_t* ids_out, float* dist_out, void* scratch,
                                   size_t scratch_bytes, int flags, i2l_stream_t stream) {
    int rc;
    if ((rc = check_members(members, n))) return rc;
    if (combine != I2L_ENSEMBLE_LOGPROB && combine != I2L_ENSEMBLE_PROB) return I2L_ERR_ARG;
    const int vocab = members[0].w->vocab;
    const bool sampling = select == I2L_SELECT_SAMPLE;
    if (sampling ? (rc = check_sample(temperature, top_k, top_p)) : (rc = check_select(select))) return rc;
    if ((rc = check_loop(rows, steps)) || (sampling && (rc = check_sample_vocab(vocab)))) return rc;
    if (cls_kind != I2L_CONSTRAIN_NONE && cls_kind != I2L_CONSTRAIN_BRACKETS && cls_kind != I2L_CONSTRAIN_ARGUMENTS)
        return I2L_ERR_ARG;
    if (cls_kind != I2L_CONSTRAIN_NONE && (rc = check_constraint(cls_kind, rows, vocab, end_id, cls, state, state_bytes)))
        return rc;
    if (forced && (sampling || cls_kind != I2L_CONSTRAIN_NONE)) return I2L_ERR_ARG;
    DecodeCall a{};
    a.members = members; a.n_members = n; a.combine = combine;
    a.rows = rows; a.steps = steps; a.tok0 = tok0; a.forced = forced;
    a.temperature = temperature; a.select = select; a.stop = stop; a.end_id = end_id;
    a.ids_out = ids_out; a.flags = flags; a.stream = stream;
    if (sampling) a.sample = SampleRule{top_k, top_p, (unsigned long long)seed, dist_out};
    else a.logits_out = dist_out;
    a.constraint = Constraint{cls_kind, cls, state, nullptr};
    a.scratch = scratch; a.scratch_bytes = scratch_bytes;
    return launch_batched(a);
}

// ---------------------------------------------------------------------------------------------
// Consensus decode (sample_rank_rules.inc.h, sample_rank.inc.h): images * samples rows of the step-batched sampling loop
// on the workspace of `images` rows, the sequence score kept by sample_batched_kernel<Rule, true>, then the two ranking
// launches.  Every refusal is decided on the host, here and in launch_batched, before the first HIP call.
// ---------------------------------------------------------------------------------------------
namespace {
struct MultiLayout {
    size_t loop, state, total;      // batched_layout of the rows | their constraint states
};
MultiLayout multi_layout(int rows, int Vp, int H, int L, int kind) {
    MultiLayout o{};
    o.loop = 0;
    o.state = i2l_align(batched_layout(rows, Vp, H, L).total);
    o.total = o.state + (kind == I2L_CONSTRAIN_NONE ? 0 : i2l_align(constraint_state_bytes(kind, rows)));
    return o;
}
inline int check_rank_dims(int images, int samples, int steps, int rank) {
    if (images <= 0 || samples <= 0 || steps <= 0) return I2L_ERR_ARG;
    if (rank != I2L_RANK_CONSENSUS && rank != I2L_RANK_LOGPROB) return I2L_ERR_ARG;
    if (samples > I2L_MAX_NBEST || steps > I2L_MAX_RANK_STEPS) return I2L_ERR_UNSUPPORTED;
    if ((long long)images * samples > 0x7fffffffll / steps) return I2L_ERR_UNSUPPORTED;
    return I2L_OK;
}
inline bool constrain_kind_ok(int kind) {
    return kind == I2L_CONSTRAIN_NONE || kind == I2L_CONSTRAIN_BRACKETS || kind == I2L_CONSTRAIN_ARGUMENTS;
}
// the two ranking launches; arguments already checked
int launch_sample_rank(const RankParams& p, hipStream_t s) {
    const dim3 grid(p.images, p.samples), block(64 * p.samples);
    const bool took = with_width<1, 2, 3, 4, 8, 16>(p.steps <= 256 ? i2l_cdiv(p.steps, 64) : p.steps <= 512 ? 8 : 16, [&](auto w) {
        hipLaunchKernelGGL(sample_distance_kernel<w>, grid, block, 0, s, p);
    });
    if (!took) return I2L_ERR_UNSUPPORTED;
    I2L_CHECK_LAUNCH();
    hipLaunchKernelGGL(sample_order_kernel, dim3(p.images), dim3(64), 0, s, p);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
}  // namespace

extern "C" size_t i2l_sample_multi_scratch_bytes(int images, int samples, int vocab, int hidden, int layers, int steps,
                                                 int constrain_kind) {
    if (check_rank_dims(images, samples, steps, I2L_RANK_CONSENSUS) != I2L_OK || !constrain_kind_ok(constrain_kind)) return 0;
    if (!batched_dims_ok(images * samples, vocab, hidden, layers) || check_sample_vocab(vocab) != I2L_OK) return 0;
    return multi_layout(images * samples, i2l_cdiv(vocab, VCHUNK) * VCHUNK, hidden, layers, constrain_kind).total;
}

extern "C" int i2l_sample_decode_multi(const i2l_decoder_weights* w, const void* workspace, int images, int samples,
                                       int steps, const int32_t* tok0, float temperature, int top_k, float top_p,
                                       uint64_t seed, int end_id, int constrain_kind, const uint8_t* cls, int rank,
                                       const double* length_norm, void* scratch, size_t scratch_bytes, int32_t* ids_out,
                                       int32_t* len_out, int32_t* finished_out, double* score_out, int32_t* risk_out,
                                       double* key_out, int32_t* order_out, int flags, i2l_stream_t stream) {
    int rc;
    if ((rc = check_weights(w)) || (rc = check_sample(temperature, top_k, top_p)) ||
        (rc = check_rank_dims(images, samples, steps, rank)) || (rc = check_sample_vocab(w->vocab)))
        return rc;
    if (!constrain_kind_ok(constrain_kind)) return I2L_ERR_ARG;
    if (!workspace || !tok0 || !ids_out || !len_out || !finished_out || !score_out || !risk_out || !key_out || !order_out)
        return I2L_ERR_ARG;
    const int rows = images * samples, V = w->vocab;
    if (constrain_kind != I2L_CONSTRAIN_NONE && (end_id < 0 || end_id >= V || !cls)) return I2L_ERR_ARG;
    const MultiLayout ml = multi_layout(rows, i2l_cdiv(V, VCHUNK) * VCHUNK, w->hidden, w->layers, constrain_kind);
    if (!scratch || scratch_bytes < ml.total) return I2L_ERR_WORKSPACE;
    char* sb = static_cast<char*>(scratch);
    hipStream_t s = i2l_s(stream);

    DecodeCall a{};
    a.w = w; a.workspace = workspace; a.rows = rows; a.steps = steps; a.samples = samples;
    a.tok0 = tok0;
    a.temperature = temperature; a.select = I2L_SELECT_SAMPLE; a.stop = I2L_STOP_STICKY; a.end_id = end_id;
    a.sample = SampleRule{top_k, top_p, (unsigned long long)seed, nullptr, score_out};
    a.ids_out = ids_out; a.flags = flags; a.stream = stream;
    if (constrain_kind != I2L_CONSTRAIN_NONE) a.constraint = Constraint{constrain_kind, cls, sb + ml.state, nullptr};
    a.scratch = sb + ml.loop; a.scratch_bytes = ml.state;
    if (hipMemsetAsync(score_out, 0, (size_t)rows * sizeof(double), s) != hipSuccess) return I2L_ERR_LAUNCH;
    if ((rc = launch_batched(a))) return rc;

    RankParams p{};
    p.ids = ids_out; p.images = images; p.samples = samples; p.steps = steps; p.end_id = end_id; p.rank = rank;
    p.score = score_out; p.norm = length_norm;
    p.len = len_out; p.fin = finished_out; p.risk = risk_out; p.key = key_out; p.order = order_out;
    return launch_sample_rank(p, s);
}

extern "C" int i2l_sample_rank(const int32_t* ids, int images, int samples, int steps, int end_id, const double* score,
                               int rank, const double* length_norm, int32_t* len_out, int32_t* finished_out,
                               int32_t* risk_out, double* key_out, int32_t* order_out, int32_t* dist_out,
                               i2l_stream_t stream) {
    int rc;
    if ((rc = check_rank_dims(images, samples, steps, rank))) return rc;
    if (!ids || !score || !len_out || !finished_out || !risk_out || !key_out || !order_out) return I2L_ERR_ARG;
    RankParams p{};
    p.ids = ids; p.images = images; p.samples = samples; p.steps = steps; p.end_id = end_id; p.rank = rank;
    p.score = score; p.norm = length_norm;
    p.len = len_out; p.fin = finished_out; p.risk = risk_out; p.key = key_out; p.order = order_out; p.dist = dist_out;
    return launch_sample_rank(p, i2l_s(stream));
}

namespace {

size_t beam_lds_bytes(int K, int L, int H, int Vp) {
    size_t b = (size_t)4 * L * K * H * sizeof(float) + (size_t)K * Vp * sizeof(float) + (size_t)K * 512 * sizeof(float);
    b = (b + 7) / 8 * 8;
    b += 2 * (size_t)K * sizeof(double) + (size_t)2 * K * K * 4 + (size_t)4 * K * 4 + 4 * 4;
    return b;
}

template <int K>
int launch_beam(const BeamParams& p, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&beam_kernel<K>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return I2L_ERR_UNSUPPORTED;
    }
    hipLaunchKernelGGL(beam_kernel<K>, dim3(p.images), dim3(NT), lds, s, p);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

}  // namespace

namespace {
// grouped beam search (beam_group.inc.h): shape and beam widths it is built for
inline bool beam_group_ok(int beam, int H, int L) { return L == 1 && H == 256 && beam >= 2 && beam <= 6; }
inline int beam_groups(int images, int beam) { return i2l_cdiv(images, BG_S / beam); }
inline size_t beam_hist_bytes(int images, int beam, int steps) {
    return i2l_align((size_t)2 * images * steps * beam * sizeof(int32_t));
}
template <int K>
int launch_beam_group(const BeamGroupParams& p, hipStream_t s) {
    constexpr size_t lds = bg_lds_bytes();
    static_assert(lds <= 160 * 1024, "beam_group_kernel LDS");
    static std::atomic<unsigned> attr{0};
    if (!i2l_lds_attr(reinterpret_cast<const void*>(&beam_group_kernel<K>), lds, attr)) return I2L_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(beam_group_kernel<K>, dim3(group_grid(p.n_groups, GQ)), dim3(GNT), lds, s, p);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
}  // namespace

extern "C" size_t i2l_beam_workspace_bytes(int images, int beam, int hidden, int layers, int steps) {
    if (images <= 0 || beam <= 0 || beam > I2L_MAX_BEAM || steps <= 0) return 0;
    size_t b = beam_hist_bytes(images, beam, steps);
    if (beam_group_ok(beam, hidden, layers))
        b += GROUP_STATUS_BYTES + group_xchg_bytes(beam_groups(images, beam), BEAM_XCHG_PER_GROUP);
    return b;
}

extern "C" int i2l_beam_decode(const i2l_decoder_weights* w, const void* workspace, int images, int beam, int steps,
                               int start_id, int end_id, void* beam_workspace, size_t beam_workspace_bytes,
                               int32_t* seq_out, int32_t* len_out, double* score_out, int flags, i2l_stream_t stream) {
    int rc = check_weights(w);
    if (rc != I2L_OK) return rc;
    if (!workspace || !beam_workspace || !seq_out || !len_out || images <= 0 || steps <= 0 || beam <= 0)
        return I2L_ERR_ARG;
    if (beam > I2L_MAX_BEAM || beam > w->vocab) return I2L_ERR_UNSUPPORTED;
    const size_t need = (size_t)2 * images * steps * beam * sizeof(int32_t);
    if (beam_workspace_bytes < need) return I2L_ERR_WORKSPACE;
    const int V = w->vocab, E = w->embed, H = w->hidden, L = w->layers;
    const Layout lo = make_layout(images, V, E, H, L);
    if (lo.Vp > 64 * 32) return I2L_ERR_UNSUPPORTED;      // top-k exclusion mask: 32 elements per lane
    hipStream_t s = i2l_s(stream);
    // grouped kernel: 4 workgroups share 12 beam slots, weights fully on chip (beam_group.inc.h); a caller falls back
    // with I2L_FLAG_NO_GROUP after a -3 result
    const bool group_on = !(flags & I2L_FLAG_NO_GROUP);
    if (group_on && beam_group_ok(beam, H, L) && V <= 512 && steps <= 65000 &&
        beam_workspace_bytes >= i2l_beam_workspace_bytes(images, beam, H, L, steps)) {
        BeamGroupParams gp{};
        gp.w = step_weights(lo, static_cast<const char*>(workspace), V, H, L);
        gp.images = images; gp.T = steps; gp.n_groups = beam_groups(images, beam);
        gp.start_id = start_id; gp.end_id = end_id;
        gp.tokhist = static_cast<int32_t*>(beam_workspace);
        gp.parhist = gp.tokhist + (size_t)images * steps * beam;
        gp.seq_out = seq_out; gp.len_out = len_out; gp.score_out = score_out;
        char* xb = static_cast<char*>(beam_workspace) + beam_hist_bytes(images, beam, steps);
        const size_t xbytes = GROUP_STATUS_BYTES + group_xchg_bytes(gp.n_groups, BEAM_XCHG_PER_GROUP);
        gp.status = reinterpret_cast<unsigned*>(xb);
        gp.xchg = reinterpret_cast<u64_t*>(xb + GROUP_STATUS_BYTES);
        gp.opts = group_opts(steps, flags);
        if (hipMemsetAsync(xb, 0, xbytes, s) != hipSuccess) return I2L_ERR_LAUNCH;
        with_width<2, 3, 4, 5, 6>(beam, [&](auto k) { rc = launch_beam_group<k>(gp, s); });   // beam_group_ok: one of these
        return rc;
    }
    BeamParams p{};
    p.w = step_weights(lo, static_cast<const char*>(workspace), V, H, L);
    p.images = images; p.T = steps; p.start_id = start_id; p.end_id = end_id;
    p.tokhist = static_cast<int32_t*>(beam_workspace);
    p.parhist = p.tokhist + (size_t)images * steps * beam;
    p.seq_out = seq_out; p.len_out = len_out; p.score_out = score_out;
    const size_t lds = beam_lds_bytes(beam, L, H, lo.Vp);
    if (lds > 160 * 1024) return I2L_ERR_UNSUPPORTED;
    rc = I2L_ERR_UNSUPPORTED;
    with_width<1, 2, 3, 4, 5, 6, 7, 8>(beam, [&](auto k) { rc = launch_beam<k>(p, lds, s); });
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Step-batched beam search (beam_batched.inc.h): the images x beam slots are the rows of one batched step, L + 2 plain
// launches per step on the caller's stream.
// ---------------------------------------------------------------------------------------------
extern "C" size_t i2l_beam_batched_scratch_bytes(int images, int beam, int vocab, int hidden, int layers, int steps) {
    if (!beam_batched_dims_ok(images, beam, vocab, hidden, layers, steps)) return 0;
    return beam_batched_layout(images, beam, i2l_cdiv(vocab, VCHUNK) * VCHUNK, hidden, layers, steps).total;
}

namespace {
// nbest: the step that keeps every completed beam (beam_nbest.inc.h); con: that step under the bracket constraint
// (beam_constrained.inc.h)
template <int K>
void launch_beam_step_batched(const BeamBatchedParams& p, bool nbest, const ConstrainRule* con, float* c_cur, float* c_next,
                              int t, hipStream_t s) {
    if (con)
        hipLaunchKernelGGL((beam_step_batched_kernel<K, true, ConstrainRule>), dim3(p.images), dim3(DB_NT), 0, s, p, c_cur,
                           c_next, t, *con);
    else if (nbest)
        hipLaunchKernelGGL((beam_step_batched_kernel<K, true>), dim3(p.images), dim3(DB_NT), 0, s, p, c_cur, c_next, t, NoRule{});
    else
        hipLaunchKernelGGL((beam_step_batched_kernel<K, false>), dim3(p.images), dim3(DB_NT), 0, s, p, c_cur, c_next, t, NoRule{});
}

// The launches of both step-batched beam entries, arguments already checked: init, per step the GEMM launches of
// decode_batched.inc.h on the images * beam rows and the step kernel, then the final kernel.  `nb` (the outputs of the
// n-best entry; bp then carries N, norm and list) selects the n-best kernels (beam_nbest.inc.h), `con` (with nb: the class
// bytes and the slots' bracket states) the well-formed search (beam_constrained.inc.h).
int beam_batched_enqueue(const i2l_decoder_weights* w, const void* workspace, const Layout& lo, const BeamBatchedLayout& bl,
                         int images, int beam, int steps, int start_id, int end_id, char* sb, BeamBatchedParams bp,
                         const BeamNbestOut* nb, const ConstrainRule* con, hipStream_t s) {
    const int V = w->vocab, H = w->hidden, L = w->layers;
    const int R = images * beam;
    const size_t LRH = (size_t)L * R * H;
    bp.images = images; bp.T = steps; bp.V = V; bp.Vp = lo.Vp; bp.H = H; bp.L = L;
    bp.start_id = start_id; bp.end_id = end_id;
    bp.tokhist = reinterpret_cast<int32_t*>(sb + bl.hist);
    bp.parhist = bp.tokhist + (size_t)images * steps * beam;
    bp.h = reinterpret_cast<float*>(sb + bl.h); bp.c = reinterpret_cast<float*>(sb + bl.c);
    bp.lg = reinterpret_cast<float*>(sb + bl.lg);
    bp.score = reinterpret_cast<double*>(sb + bl.score);
    bp.last = reinterpret_cast<int*>(sb + bl.last); bp.slot_live = reinterpret_cast<int*>(sb + bl.slot_live);
    bp.img = reinterpret_cast<BeamImage*>(sb + bl.img);
    bp.live = reinterpret_cast<unsigned*>(sb + bl.live);

    // the GEMM launches of decode_batched.inc.h on the R rows: the slot's last token, the image's Genc row, parity 0
    BatchedParams p{};
    p.w = step_weights(lo, static_cast<const char*>(workspace), V, H, L);
    p.B = R; p.T = steps; p.genc_div = beam; p.forced = nullptr;
    p.h = bp.h; p.lg = reinterpret_cast<float*>(sb + bl.lg);
    p.tok = bp.last; p.live = bp.live;
    p.temperature = 1.0f; p.select = I2L_SELECT_LOGITS; p.stop = I2L_STOP_NONE; p.end_id = end_id;

    const size_t init_blocks = (2 * LRH + DB_NT - 1) / DB_NT;
    hipLaunchKernelGGL(beam_init_batched_kernel, dim3((unsigned)(init_blocks < 1024 ? init_blocks : 1024)), dim3(DB_NT), 0,
                       s, bp, beam);
    I2L_CHECK_LAUNCH();
    if (nb && start_id == end_id) {
        hipLaunchKernelGGL(beam_nbest_init_kernel, dim3(i2l_cdiv(images, DB_NT)), dim3(DB_NT), 0, s, bp);
        I2L_CHECK_LAUNCH();
    }
    if (con) {
        hipLaunchKernelGGL(beam_constrained_init_kernel, dim3(i2l_cdiv(R, DB_NT)), dim3(DB_NT), 0, s, con->state, (size_t)R);
        I2L_CHECK_LAUNCH();
    }
    const int tb_lstm = batched_tile_rows(H / 16, R), tb_logits = batched_tile_rows(lo.Vp / DB_COLS, R);
    for (int t = 0; t < steps; ++t) {
        float* c_cur = bp.c + (size_t)(t & 1) * LRH;
        float* c_next = bp.c + (size_t)((t + 1) & 1) * LRH;
        p.c = c_cur;
        launch_batched_step(p, tb_lstm, tb_logits, 0, s);
        with_width<1, 2, 3, 4, 5, 6, 7, 8>(beam, [&](auto k) {
            launch_beam_step_batched<k>(bp, nb != nullptr, con, c_cur, c_next, t, s);
        });
        I2L_CHECK_LAUNCH();
    }
    if (nb)
        hipLaunchKernelGGL(beam_nbest_final_kernel, dim3((unsigned)(((size_t)images * bp.N + DB_NT - 1) / DB_NT)), dim3(DB_NT),
                           0, s, bp, *nb, beam);
    else
        hipLaunchKernelGGL(beam_final_batched_kernel, dim3(i2l_cdiv(images, DB_NT)), dim3(DB_NT), 0, s, bp, beam);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
}  // namespace

extern "C" int i2l_beam_decode_batched(const i2l_decoder_weights* w, const void* workspace, int images, int beam,
                                       int steps, int start_id, int end_id, void* scratch, size_t scratch_bytes,
                                       int32_t* seq_out, int32_t* len_out, double* score_out, int flags,
                                       i2l_stream_t stream) {
    (void)flags;
    // every refusal is decided here, before the first HIP call
    int rc = check_weights(w);
    if (rc != I2L_OK) return rc;
    if (!workspace || !scratch || !seq_out || !len_out || images <= 0 || steps <= 0 || beam <= 0) return I2L_ERR_ARG;
    const int V = w->vocab, E = w->embed, H = w->hidden, L = w->layers;
    if (!beam_batched_dims_ok(images, beam, V, H, L, steps)) return I2L_ERR_UNSUPPORTED;
    const Layout lo = make_layout(images, V, E, H, L);
    const BeamBatchedLayout bl = beam_batched_layout(images, beam, lo.Vp, H, L, steps);
    if (scratch_bytes < bl.total) return I2L_ERR_WORKSPACE;

    BeamBatchedParams bp{};
    bp.seq_out = seq_out; bp.len_out = len_out; bp.score_out = score_out;
    return beam_batched_enqueue(w, workspace, lo, bl, images, beam, steps, start_id, end_id, static_cast<char*>(scratch), bp,
                                nullptr, nullptr, i2l_s(stream));
}

// ---------------------------------------------------------------------------------------------
// N-best beam search with length-normalised ranking (beam_nbest.inc.h): the search above, every completed beam kept
// in a per-image list sorted by score / norm[length] instead of the best raw score alone.
// ---------------------------------------------------------------------------------------------
extern "C" size_t i2l_beam_nbest_scratch_bytes(int images, int beam, int nbest, int vocab, int hidden, int layers,
                                               int steps) {
    if (!beam_nbest_dims_ok(images, beam, nbest, vocab, hidden, layers, steps)) return 0;
    return beam_nbest_layout(images, beam, nbest, i2l_cdiv(vocab, VCHUNK) * VCHUNK, hidden, layers, steps).total;
}

extern "C" int i2l_beam_decode_nbest(const i2l_decoder_weights* w, const void* workspace, int images, int beam, int nbest,
                                     int steps, int start_id, int end_id, const double* length_norm, void* scratch,
                                     size_t scratch_bytes, int32_t* seq_out, int32_t* len_out, double* score_out,
                                     double* key_out, int32_t* finished_out, int32_t* count_out, int flags,
                                     i2l_stream_t stream) {
    (void)flags;
    // every refusal is decided here, before the first HIP call
    int rc = check_weights(w);
    if (rc != I2L_OK) return rc;
    if (!workspace || !scratch || !seq_out || !len_out || !score_out || !count_out || images <= 0 || steps <= 0 ||
        beam <= 0 || nbest <= 0)
        return I2L_ERR_ARG;
    const int V = w->vocab, E = w->embed, H = w->hidden, L = w->layers;
    if (!beam_nbest_dims_ok(images, beam, nbest, V, H, L, steps)) return I2L_ERR_UNSUPPORTED;
    const Layout lo = make_layout(images, V, E, H, L);
    const BeamNbestLayout nl = beam_nbest_layout(images, beam, nbest, lo.Vp, H, L, steps);
    if (scratch_bytes < nl.total) return I2L_ERR_WORKSPACE;

    char* sb = static_cast<char*>(scratch);
    BeamBatchedParams bp{};
    bp.N = nbest; bp.norm = length_norm;
    bp.list = reinterpret_cast<NbestEntry*>(sb + nl.list);
    BeamNbestOut nb{};
    nb.seq_out = seq_out; nb.len_out = len_out; nb.score_out = score_out; nb.key_out = key_out;
    nb.finished_out = finished_out; nb.count_out = count_out;
    return beam_batched_enqueue(w, workspace, lo, nl.b, images, beam, steps, start_id, end_id, sb, bp, &nb, nullptr,
                                i2l_s(stream));
}

// ---------------------------------------------------------------------------------------------
// Well-formed N-best beam search (beam_bracket_rules.inc.h, beam_constrained.inc.h): the search above in which a slot
// extends only by columns its bracket state allows, so every returned row nests and ends on END.
// ---------------------------------------------------------------------------------------------
extern "C" size_t i2l_beam_nbest_constrained_scratch_bytes(int images, int beam, int nbest, int vocab, int hidden, int layers,
                                                           int steps) {
    if (!beam_nbest_dims_ok(images, beam, nbest, vocab, hidden, layers, steps)) return 0;
    return beam_constrained_layout(images, beam, nbest, i2l_cdiv(vocab, VCHUNK) * VCHUNK, hidden, layers, steps).total;
}

extern "C" int i2l_beam_decode_nbest_constrained(const i2l_decoder_weights* w, const void* workspace, int images, int beam,
                                                 int nbest, int steps, int start_id, int end_id, const double* length_norm,
                                                 void* scratch, size_t scratch_bytes, int32_t* seq_out, int32_t* len_out,
                                                 double* score_out, double* key_out, int32_t* finished_out,
                                                 int32_t* count_out, int flags, const uint8_t* cls, i2l_stream_t stream) {
    (void)flags;
    // every refusal is decided here, before the first HIP call
    int rc = check_weights(w);
    if (rc != I2L_OK) return rc;
    if (!workspace || !scratch || !seq_out || !len_out || !score_out || !count_out || !cls || images <= 0 || steps <= 0 ||
        beam <= 0 || nbest <= 0)
        return I2L_ERR_ARG;
    const int V = w->vocab, E = w->embed, H = w->hidden, L = w->layers;
    if (end_id < 0 || end_id >= V) return I2L_ERR_ARG;
    if (!beam_nbest_dims_ok(images, beam, nbest, V, H, L, steps)) return I2L_ERR_UNSUPPORTED;
    const Layout lo = make_layout(images, V, E, H, L);
    const BeamConstrainedLayout cl = beam_constrained_layout(images, beam, nbest, lo.Vp, H, L, steps);
    if (scratch_bytes < cl.total) return I2L_ERR_WORKSPACE;

    char* sb = static_cast<char*>(scratch);
    BeamBatchedParams bp{};
    bp.N = nbest; bp.norm = length_norm;
    bp.list = reinterpret_cast<NbestEntry*>(sb + cl.n.list);
    BeamNbestOut nb{};
    nb.seq_out = seq_out; nb.len_out = len_out; nb.score_out = score_out; nb.key_out = key_out;
    nb.finished_out = finished_out; nb.count_out = count_out;
    const ConstrainRule con{cls, reinterpret_cast<BracketState*>(sb + cl.state), nullptr};
    return beam_batched_enqueue(w, workspace, lo, cl.n.b, images, beam, steps, start_id, end_id, sb, bp, &nb, &con,
                                i2l_s(stream));
}

extern "C" size_t i2l_decoder_group_status_offset(int rows, int vocab, int embed, int hidden, int layers) {
    const Layout lo = make_layout(rows, vocab, embed, hidden, layers);
    return lo.xchg_bytes ? lo.xchg : 0;
}

// Size of the region that starts there (status words + the groups' exchange granules): what a grouped launch zeroes before its
// kernel -- or the caller, earlier and on another stream, with I2L_FLAG_DECODE_REGION_CLEARED.
extern "C" size_t i2l_decoder_group_region_bytes(int rows, int vocab, int embed, int hidden, int layers) {
    return make_layout(rows, vocab, embed, hidden, layers).xchg_bytes;
}
// The state block of i2l_greedy_decode_halves inside the workspace: 0 bytes where these dimensions have no such launch.
extern "C" size_t i2l_decoder_group_state_offset(int rows, int vocab, int embed, int hidden, int layers) {
    return make_layout(rows, vocab, embed, hidden, layers).state;
}
extern "C" size_t i2l_decoder_group_state_bytes(int rows, int vocab, int embed, int hidden, int layers) {
    return make_layout(rows, vocab, embed, hidden, layers).state_bytes;
}

#ifdef I2L_GROUP_STAMPS
extern "C" size_t i2l_debug_group_status_offset(int rows, int vocab, int embed, int hidden, int layers) {
    return make_layout(rows, vocab, embed, hidden, layers).xchg;
}
#endif
