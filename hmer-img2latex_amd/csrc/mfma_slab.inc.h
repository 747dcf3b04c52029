// The split-bf16 slab product of the step-batched kernels (decode_batched.inc.h, beam_batched.inc.h, train_batched.inc.h):
// one workgroup's TB rows x 64 columns of X . W on the matrix cores, both operands split into three bf16 pieces while
// they are staged into LDS (bf16_split.inc.h), six partial products v_mfma_f32_16x16x32_bf16, fp32 accumulation.  One
// copy, so that inference and training stage, split and sum in the same way.
// Included inside each translation unit's anonymous namespace.
#pragma once

#include "bf16_split.inc.h"

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

union Frag16 {
    bf16x8_t v;
    u32x4_t q;
    unsigned short s[8];
};

constexpr int DB_NT = 256;       // threads per workgroup: four waves, 16 of the 64 columns each
constexpr int DB_COLS = 64;      // weight columns per workgroup
constexpr int DB_KC = 64;        // K rows per staging round: two MFMA k-steps
constexpr int DB_KG = DB_KC / 8; // 8-element k groups per round (one 16-byte operand fragment each)

// LDS of one staging round: weights [3 pieces][DB_KG][64 columns][8] bf16, activations [3][DB_KG][TB + 1 rows][8] bf16
// (the odd row count spreads the 16-byte stores of a row's eight k groups over the banks)
template <int TB>
struct DbLds {
    static constexpr int WS = 3 * DB_KG * DB_COLS;          // 16-byte fragments
    static constexpr int XSTRIDE = TB + 1;
    static constexpr int XS = 3 * DB_KG * XSTRIDE;
    static constexpr int XRUNS = (TB * DB_KG + DB_NT - 1) / DB_NT;   // activation runs of 8 floats per thread and round
};

__device__ __forceinline__ void db_split8(const float (&v)[8], u32x4_t& q0, u32x4_t& q1, u32x4_t& q2) {
    unsigned s0[4], s1[4], s2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3_pair(v[2 * i], v[2 * i + 1], s0[i], s1[i], s2[i]);
    q0 = u32x4_t{s0[0], s0[1], s0[2], s0[3]};
    q1 = u32x4_t{s1[0], s1[1], s1[2], s1[3]};
    q2 = u32x4_t{s2[0], s2[1], s2[2], s2[3]};
}

// the sum of one row tile's three piece classes, small terms first
__device__ __forceinline__ f32x4_t db_fold(const f32x4_t (&a)[3]) { return (a[2] + a[1]) + a[0]; }

// acc[nt][piece class] += W[0..K)[col0 .. col0 + 63]^T . X[rows row0 .. row0 + TB)[0..K)^T for this workgroup's tile:
// wave w takes columns col0 + 16 w .. + 15 and all TB / 16 row tiles.  W is [K][ldw] fp32, X is [B][ldx] fp32; rows past
// B - 1 read row B - 1 (the caller drops them).  K % DB_KC == 0.  The next round's global loads are issued before this
// round's MFMAs.  Contains __syncthreads(); ends with one, so ws / xs are free on return.
template <int TB>
__device__ __forceinline__ void db_slab(f32x4_t (&acc)[TB / 16][3], const float* __restrict__ W, size_t ldw, int col0,
                                        const float* __restrict__ X, int ldx, int row0, int B, int K, u32x4_t* ws,
                                        u32x4_t* xs, int tid) {
    using S = DbLds<TB>;
    const int lane = tid & 63, wave = tid >> 6;
    const int wcol = tid & 63, wkg = tid >> 6;                    // weights: column wcol, k groups wkg and wkg + 4
    float wv[2][8];
    float xv[S::XRUNS][8];
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j) wv[q][j] = W[(size_t)(k0 + 8 * (wkg + 4 * q) + j) * ldw + col0 + wcol];
#pragma unroll
        for (int q = 0; q < S::XRUNS; ++q) {
            const int idx = tid + DB_NT * q;                      // run idx: row idx >> 3, k group idx & 7
            if (idx < TB * DB_KG) {
                const int row = min(row0 + (idx >> 3), B - 1);
                const float4* src = reinterpret_cast<const float4*>(X + (size_t)row * ldx + k0 + 8 * (idx & 7));
                const float4 a = src[0], b = src[1];
                xv[q][0] = a.x; xv[q][1] = a.y; xv[q][2] = a.z; xv[q][3] = a.w;
                xv[q][4] = b.x; xv[q][5] = b.y; xv[q][6] = b.z; xv[q][7] = b.w;
            }
        }
    };
    load(0);
    for (int k0 = 0; k0 < K; k0 += DB_KC) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            u32x4_t q0, q1, q2;
            db_split8(wv[q], q0, q1, q2);
            const int at = (wkg + 4 * q) * DB_COLS + wcol;
            ws[at] = q0; ws[DB_KG * DB_COLS + at] = q1; ws[2 * DB_KG * DB_COLS + at] = q2;
        }
#pragma unroll
        for (int q = 0; q < S::XRUNS; ++q) {
            const int idx = tid + DB_NT * q;
            if (idx < TB * DB_KG) {
                u32x4_t q0, q1, q2;
                db_split8(xv[q], q0, q1, q2);
                const int at = (idx & 7) * S::XSTRIDE + (idx >> 3);
                xs[at] = q0; xs[DB_KG * S::XSTRIDE + at] = q1; xs[2 * DB_KG * S::XSTRIDE + at] = q2;
            }
        }
        __syncthreads();
        if (k0 + DB_KC < K) load(k0 + DB_KC);
#pragma unroll
        for (int ks = 0; ks < DB_KC / 32; ++ks) {
            // A (weights): lane l holds A[m = l & 15][k = 8 (l >> 4) + j]; B (activations): B[k = 8 (l >> 4) + j][n = l & 15]
            const int kg = 4 * ks + (lane >> 4);
            Frag16 a[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) a[c].q = ws[(c * DB_KG + kg) * DB_COLS + 16 * wave + (lane & 15)];
#pragma unroll
            for (int nt = 0; nt < TB / 16; ++nt) {
                Frag16 b[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) b[c].q = xs[(c * DB_KG + kg) * S::XSTRIDE + 16 * nt + (lane & 15)];
                acc[nt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0].v, b[0].v, acc[nt][0], 0, 0, 0);
                acc[nt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0].v, b[1].v, acc[nt][1], 0, 0, 0);
                acc[nt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1].v, b[0].v, acc[nt][1], 0, 0, 0);
                acc[nt][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0].v, b[2].v, acc[nt][2], 0, 0, 0);
                acc[nt][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1].v, b[1].v, acc[nt][2], 0, 0, 0);
                acc[nt][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2].v, b[0].v, acc[nt][2], 0, 0, 0);
            }
        }
        __syncthreads();
    }
}

// rows per tile: the smallest of 16 / 32 / 64 that keeps the grid within the 256 compute units (B = 256, H = 512: TB = 32,
// 32 x 8 workgroups); larger batches take 64
inline int batched_tile_rows(int col_tiles, int rows) {
    for (int tb = 16; tb < 64; tb *= 2)
        if ((long)col_tiles * i2l_cdiv(rows, tb) <= 256) return tb;
    return 64;
}
