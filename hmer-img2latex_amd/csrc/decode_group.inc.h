// Grouped greedy decode, M = 4 or 8 members x M rows (included by decode.hip inside its anonymous namespace).
//
// The row-per-workgroup kernel streams ~1.1 MB of weights from L2 into every CU at every step (the L2 -> CU path,
// 64 B/clk/CU, bounds it: ~11.5 us/step).  Here M workgroups (one per CU) decode M batch rows together and each keeps
// one M-th of the weights on chip for the whole loop, so nothing is streamed:
//     member m holds  WhhT[:, gate columns of hidden units UPM m .. + UPM - 1]   256 x 1024/M floats in registers
//                     WoutT[:, vocabulary columns CPM m .. + CPM - 1]           256 x CPM floats in LDS
// (UPM = 256 / M, CPM = 512 / M) with 2048 / M threads per workgroup, 128 weights per thread in architectural registers.
//   M = 4: 512 threads, two waves per SIMD (one wave's LDS / DPP / transcendental latencies are the other's issue slots).
//   M = 8: 256 threads, ONE wave per SIMD, <= 256 registers, ~80 KB of LDS: the footprint that leaves room for one conv
//          workgroup (247 registers x 4 waves, 70 KB) on the same CU, so that the encoder of batch i + 1 can run beside
//          the decode of batch i (profiles/r03/coresident.txt).  The FMA count per member and step is
//          the same (8 rows x 1/8 of the columns instead of 4 rows x 1/4); the price is 7 peers to poll instead of 3
//          and a deeper reduce-scatter.
// Per step member m computes, for all M rows, the gates / LSTM cell of ITS hidden units and the logits of ITS vocabulary
// columns; both need the full h of the group, so a step has two small exchanges inside the group:
//     1. every member publishes its UPM x M new h values and reads the other members' ones;
//     2. every member publishes, per row, the (max, first index) of its vocabulary columns; all members combine the M
//        candidates in member (= index) order, so they agree on the token without further talk.
// The recurrent product h . Whh^T of the NEXT step does not depend on the token (only the table row P[token] that is
// added at its end does), so it runs between publishing the candidates and polling for them: exchange 2 is hidden.
//
// Synchronisation inside a workgroup is ONE barrier per step (after the h exchange).  The two others of the first
// design are gone: (i) every WAVE polls the M x M candidate granules of the previous step itself (its own member's too:
// they are published to L2 like the peers'), merges them in registers and -- because it needs nobody's permission --
// does so in the middle of the recurrent product, so that the gather of the token's table row P[token] is in flight
// while the rest of that product runs; (ii) the per-row arg max over the waves is an LDS 64-bit atomic max, and the
// wave that arrives last (an LDS counter tells it) publishes the member's M candidates.  h lives in two LDS buffers by
// step parity, which is what makes the remaining barrier sufficient.
//
// Exchange = 8-byte {value, tag} granules, tag = step + 1, each written by ONE agent-scope relaxed atomic store (sc1,
// write-through) and polled by agent-scope relaxed atomic loads (sc1: never served from this CU's L1 or a stale L2
// line): the data is its own flag, no fences, no dependence on XCD placement.  Two buffers by step parity suffice:
// a member overwrites a slot two steps later, after it has consumed from every peer data that the peer published
// after reading that slot.  The granule block is zeroed by a memset node before every launch.
//
// Seating, progress argument, bounded polls (PollClock), placement exchange: group_common.inc.h.  On a time-out the
// workgroup fills its ids with -3 (and its logits with NaN).
// Memory model: the granule stores are relaxed atomics at AGENT scope (sc1, write-through) and the polls agent-scope
// loads -- conformant HSA.  When the members measure themselves on one XCD the stores drop to WORKGROUP scope (a plain
// store that gfx950's write-through L1 forwards to the XCD's L2, where the peers' L1-bypassing polls find it: 1.28 ->
// 0.50 us per exchange); that relies on the gfx950 cache hierarchy, not on the memory model, so the conformant flavour
// stays selectable (I2L_FLAG_AGENT_SCOPE_EXCHANGE) and tested.
// Logits output and forced tokens: M = 4 only (the 8-member launch is ids only; decode.hip picks the kernel).
#include "group_common.inc.h"

constexpr int GQ = 4;                    // members of the 4-row tiles (decode_group_kernel<4>, beam_group_kernel)
constexpr int GNT = 512;                 // their threads per workgroup
constexpr int GRAN_H = 256;              // h granules per member and step: [unit 256 / M][row M]
constexpr int GRAN_C = GRAN_H;           // M candidate granules (one per row), a 128-byte line of their own
constexpr int GRAN_X = GRAN_H + 16;      // 1 placement granule (XCC id), a line of its own
constexpr int GRAN = GRAN_H + 32;

template <int M>
struct GroupShape {
    static_assert(M == 4 || M == 8, "members per group");
    static constexpr int NT = 2048 / M;  // threads per workgroup
    static constexpr int UPM = 256 / M;  // hidden units per member
    static constexpr int CPM = 512 / M;  // vocabulary columns per member
    // LDS: W_out columns | h [2 parities][256 k][M rows] | (M = 4) per-thread image-side gate constants Genc, read once
    // per step: four registers less across the recurrent product | arg-max keys [2 parities][M rows] | counters [2] + flags
    static constexpr size_t LDS = (size_t)(256 * CPM + 2 * 256 * M + (M == 4 ? 4 * NT : 0)) * sizeof(float) +
                                  (size_t)2 * M * 8 + 8 * sizeof(int);
    static constexpr size_t XCHG_PER_GROUP = (size_t)2 * M * GRAN * 8;   // [2 parities][M][GRAN]
};

// One row tile of decode_group16_kernel<2> (i2l_greedy_decode_halves): 16 rows per group of ITS OWN batch, a range of
// that batch's steps.  n == 0: the tile is absent (it still takes part in the exchanges, see the kernel).
struct HalfTile {
    const float* Genc;    // that batch's image-side gate rows
    const int32_t* tok0;
    int32_t* ids;         // [B][T]
    int B, T;             // rows and steps of the whole batch
    int t0, n;            // this launch runs steps t0 .. t0 + n - 1
    const void* state_in; // t0 > 0: the state block the launch of the earlier steps saved (group16_state_bytes)
    void* state_out;      // t0 + n < T: where to save it
};

struct GroupParams {
    StepWeights w;
    int B, T, n_groups;
    const int32_t* tok0;
    const int32_t* forced;
    int32_t* ids;
    float* logits;
    float temperature;
    int use_temp, stop, end_id;
    u64_t* xchg;          // [n_groups][2][M][GRAN]
    unsigned* status;     // [0] != 0: a poll timed out
    GroupOpts opts;       // poll limits, exchange flavour (group_common.inc.h)
    unsigned* resident_flag;   // may be null: receives resident_value once every group of the launch is resident
    unsigned resident_value;
    HalfTile tile[2];     // decode_group16_kernel<2> only (it ignores B, T, tok0, ids and w.Genc above)
};

constexpr int DPP_SHL12 = 0x10C;

// ---- Tiles.  Gates: thread (ul = tid >> 3, ke = tid & 7) holds the 4 gate columns of hidden unit `unit` for the 32
// k = ke (mod 8).  Logits: thread (cq = tid >> 4, ks = tid & 15) holds vocabulary columns col .. col + 3 for the 16
// k = ks (mod 16).  h is [k][rows] in LDS.  The 4-row tiles serve decode_group_kernel<4> and beam_group_kernel.
template <int NT>
__device__ __forceinline__ void load_weight_image(f32x2 (&wreg)[32][2], float4* wout_s4, const StepWeights& w, int unit,
                                                  int ke, int col, int ks, int tid) {
#pragma unroll
    for (int j = 0; j < 32; ++j) {                          // WhhT[8j + ke][4 unit .. +3] as (i,f), (g,o)
        const float4 t4 = *reinterpret_cast<const float4*>(w.WhhT[0] + (size_t)(8 * j + ke) * 1024 + 4 * unit);
        wreg[j][0] = f32x2{t4.x, t4.y};
        wreg[j][1] = f32x2{t4.z, t4.w};
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)                            // [16 j][NT threads]: WoutT[16j + ks][col ..+3]
        wout_s4[j * NT + tid] = *reinterpret_cast<const float4*>(w.WoutT + (size_t)(16 * j + ks) * 512 + col);
}

// acc[gate][row pair] += the 32 k of this lane for 4 rows; hq4 = h[k = ke] as float4.  8 batches of 4 k, h read one
// batch ahead (two register sets); hook(b) runs before batch b's FMAs.
template <class Hook>
__device__ __forceinline__ void rec_product4(f32x2 (&acc)[4][2], const f32x2 (&wreg)[32][2], const float4* hq4,
                                             Hook&& hook) {
    float4 hb[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) hb[0][i] = hq4[8 * i];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        if (b + 1 < 8) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hb[(b + 1) & 1][i] = hq4[8 * ((b + 1) * 4 + i)];
        }
        hook(b);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) fma_4x4(acc, wreg[b * 4 + i][0], wreg[b * 4 + i][1], hb[b & 1][i]);
    }
}
// fold the 8 k-slices (reduce-scatter: 16 -> 8 -> 4 -> 2 values per lane): lanes ke < 4 end with gates (i, f) of row ke,
// lanes ke >= 4 with (g, o) of row ke - 4
__device__ __forceinline__ void fold_gates4(const f32x2 (&acc)[4][2], int ke, float (&z)[2]) {
    const bool b0 = ke & 1, b1 = ke & 2, b2 = ke & 4;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        float wv[2];
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            const float ux = rs_level<DPP_HMIRROR>(acc[e][rp].x, acc[2 + e][rp].x, b2);
            const float uy = rs_level<DPP_HMIRROR>(acc[e][rp].y, acc[2 + e][rp].y, b2);
            wv[rp] = rs_level<DPP_XOR1>(ux, uy, b0);
        }
        z[e] = rs_level<DPP_XOR2>(wv[0], wv[1], b1);
    }
}
// pa[column][row pair] = the 16 k of this lane for 4 rows; hq4 = h[k = ks] as float4; 8 batches of 2 k, read one ahead
template <int NT>
__device__ __forceinline__ void logits_product4(f32x2 (&pa)[4][2], const float4* wout_s4, const float4* hq4, int tid) {
#pragma unroll
    for (int c = 0; c < 4; ++c) { pa[c][0] = splat2(0.f); pa[c][1] = splat2(0.f); }
    float4 wb[2][2], hb[2][2];
    auto fetch = [&](int set, int b) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            wb[set][i] = wout_s4[(b * 2 + i) * NT + tid];
            hb[set][i] = hq4[16 * (b * 2 + i)];
        }
    };
    fetch(0, 0);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        if (b + 1 < 8) fetch((b + 1) & 1, b + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float4 w4 = wb[b & 1][i];
            fma_4x4(pa, f32x2{w4.x, w4.y}, f32x2{w4.z, w4.w}, hb[b & 1][i]);
        }
    }
}
// fold the 16 k-slices: 16 -> 8 -> 4 -> 2 -> 1; the lane ends with the logit (bias not added) of column
// 2 ((ks >> 2) & 1) + (ks >> 3) of its quad, row ks & 3
__device__ __forceinline__ float fold_logits4(const f32x2 (&pa)[4][2], int ks) {
    const bool b0 = ks & 1, b1 = ks & 2, b2 = ks & 4, b3 = ks & 8;
    float z[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        float wv[2];
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            const float ux = rs_level<DPP_HMIRROR>(pa[e][rp].x, pa[2 + e][rp].x, b2);
            const float uy = rs_level<DPP_HMIRROR>(pa[e][rp].y, pa[2 + e][rp].y, b2);
            wv[rp] = rs_level<DPP_XOR1>(ux, uy, b0);
        }
        z[e] = rs_level<DPP_XOR2>(wv[0], wv[1], b1);
    }
    return rs_level<DPP_ROR8>(z[0], z[1], b3);
}

// The 8-row tiles, [row half] in front: 16 batches of 2 k x two row halves; hq4 = h[k = ke] as 2 float4 per k
template <class Hook>
__device__ __forceinline__ void rec_product8(f32x2 (&acc)[2][4][2], const f32x2 (&wreg)[32][2], const float4* hq4,
                                             Hook&& hook) {
    float4 hb[2][2][2];                                     // [set][k of the pair][row half]
#pragma unroll
    for (int i = 0; i < 2; ++i) { hb[0][i][0] = hq4[16 * i]; hb[0][i][1] = hq4[16 * i + 1]; }
#pragma unroll
    for (int b = 0; b < 16; ++b) {                          // k = 8 (2b + i) + ke
        if (b + 1 < 16) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                hb[(b + 1) & 1][i][0] = hq4[16 * ((b + 1) * 2 + i)];
                hb[(b + 1) & 1][i][1] = hq4[16 * ((b + 1) * 2 + i) + 1];
            }
        }
        hook(b);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            fma_4x4(acc[0], wreg[b * 2 + i][0], wreg[b * 2 + i][1], hb[b & 1][i][0]);
            fma_4x4(acc[1], wreg[b * 2 + i][0], wreg[b * 2 + i][1], hb[b & 1][i][1]);
        }
    }
}
// 32 sums -> the 4 gates of row ke on lane ke (three reduce-scatter levels)
__device__ __forceinline__ void fold_gates8(const f32x2 (&acc)[2][4][2], int ke, float (&z)[4]) {
    const bool b0 = ke & 1, b1 = ke & 2, b2 = ke & 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        // level 1 (lane <-> 7 - lane): lanes 0..3 keep rows 0..3, lanes 4..7 rows 4..7
        const float u0x = rs_level<DPP_HMIRROR>(acc[0][g][0].x, acc[1][g][0].x, b2);   // row 0 | 4
        const float u0y = rs_level<DPP_HMIRROR>(acc[0][g][0].y, acc[1][g][0].y, b2);   // row 1 | 5
        const float u1x = rs_level<DPP_HMIRROR>(acc[0][g][1].x, acc[1][g][1].x, b2);   // row 2 | 6
        const float u1y = rs_level<DPP_HMIRROR>(acc[0][g][1].y, acc[1][g][1].y, b2);   // row 3 | 7
        // level 2 (lane ^ 2): keep the row pair b1
        const float vx = rs_level<DPP_XOR2>(u0x, u1x, b1);
        const float vy = rs_level<DPP_XOR2>(u0y, u1y, b1);
        // level 3 (lane ^ 1): keep row b0 of the pair
        z[g] = rs_level<DPP_XOR1>(vx, vy, b0);
    }
}
// pa[row half][column][row pair] = the 16 k of this lane for 8 rows; hq4 = h[k = ks] as 2 float4 per k
template <int NT>
__device__ __forceinline__ void logits_product8(f32x2 (&pa)[2][4][2], const float4* wout_s4, const float4* hq4, int tid) {
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int c = 0; c < 4; ++c) { pa[hf][c][0] = splat2(0.f); pa[hf][c][1] = splat2(0.f); }
    float4 wb[2], hb[2][2];
    wb[0] = wout_s4[tid];
    hb[0][0] = hq4[0]; hb[0][1] = hq4[1];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j + 1 < 16) {
            wb[(j + 1) & 1] = wout_s4[(j + 1) * NT + tid];
            hb[(j + 1) & 1][0] = hq4[32 * (j + 1)];
            hb[(j + 1) & 1][1] = hq4[32 * (j + 1) + 1];
        }
        __builtin_amdgcn_sched_barrier(0);
        const float4 w4 = wb[j & 1];
        fma_4x4(pa[0], f32x2{w4.x, w4.y}, f32x2{w4.z, w4.w}, hb[j & 1][0]);
        fma_4x4(pa[1], f32x2{w4.x, w4.y}, f32x2{w4.z, w4.w}, hb[j & 1][1]);
    }
}
// fold the 16 k-slices: 32 -> 16 -> 8 -> 4 -> 2; the lane ends with columns 2 (ks & 1), +1 of its quad (bias not
// added), row ks >> 1
__device__ __forceinline__ void fold_logits8(const f32x2 (&pa)[2][4][2], int ks, float (&lv)[2]) {
    const bool b0 = ks & 1, b1 = ks & 2, b2 = ks & 4, b3 = ks & 8;
    float v[4];                                             // per column: row (ks >> 1) after three row levels
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        // level 1 (lane ^ 8 within 16): lanes ks < 8 keep rows 0..3, the others rows 4..7
        const float u0x = rs_level<DPP_ROR8>(pa[0][c][0].x, pa[1][c][0].x, b3);
        const float u0y = rs_level<DPP_ROR8>(pa[0][c][0].y, pa[1][c][0].y, b3);
        const float u1x = rs_level<DPP_ROR8>(pa[0][c][1].x, pa[1][c][1].x, b3);
        const float u1y = rs_level<DPP_ROR8>(pa[0][c][1].y, pa[1][c][1].y, b3);
        // level 2 (lane <-> 7 - lane within 8): keep the row pair b2
        const float wx = rs_level<DPP_HMIRROR>(u0x, u1x, b2);
        const float wy = rs_level<DPP_HMIRROR>(u0y, u1y, b2);
        // level 3 (lane ^ 2): keep row b1 of the pair
        v[c] = rs_level<DPP_XOR2>(wx, wy, b1);
    }
    // level 4 (lane ^ 1): keep the column pair b0
    lv[0] = rs_level<DPP_XOR1>(v[0], v[2], b0);
    lv[1] = rs_level<DPP_XOR1>(v[1], v[3], b0);
}

template <int M>
__global__ __launch_bounds__(GroupShape<M>::NT) void decode_group_kernel(GroupParams p) {
    using S = GroupShape<M>;
    constexpr int NT = S::NT, UPM = S::UPM, CPM = S::CPM;
    constexpr bool FULL = M == 4;                           // logits output and forced tokens
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float4* wout_s4 = reinterpret_cast<float4*>(smem);      // [16 j][NT threads]: WoutT[16j + ks][CPM m + 4cq ..+3]
    float* h_s = smem + 256 * CPM;                          // [2][256 k][M rows]  full h of step t in buffer t & 1
    float4* genc_s = reinterpret_cast<float4*>(h_s + 2 * 256 * M);   // M = 4: [NT threads] Genc[row ke & 3][4 unit ..+3]
    u64_t* redk = reinterpret_cast<u64_t*>(genc_s + (M == 4 ? NT : 0));   // [2][M rows] arg-max keys of this member
    int* cnt_s = reinterpret_cast<int*>(redk + 2 * M);      // [0..1] waves that added their keys (by parity),
                                                            // [2] a poll timed out, [3] members share one XCD

    const StepWeights& w = p.w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GroupSeat seat = group_seat<M>();
    const int group = seat.group, m = seat.m;
    if (group >= p.n_groups) return;
    const int B = p.B, T = p.T, V = w.V;
    const int row0 = group * M;
    // gates: hidden unit UPM m + ul, k = ke (mod 8) -> 32 k, 4 gates x M rows; cell: lanes ke < M own (unit, row ke)
    const int ul = tid >> 3, ke = tid & 7;
    const int unit = UPM * m + ul;
    // logits: columns CPM m + 4cq ..+3, k = ks (mod 16) -> 16 k, 4 columns x M rows; afterwards the lane owns the
    // logits l_v (M = 8: and l_v + 1) of row l_row
    const int cq = tid >> 4, ks = tid & 15;
    const int l_row = M == 4 ? ks & 3 : ks >> 1;
    const int l_v = CPM * m + 4 * cq + (M == 4 ? ((ks >> 2) & 1) * 2 + (ks >> 3) : 2 * (ks & 1));
    const int my_r = ke & (M - 1);                          // row of this lane's cell (and of its token)
    constexpr int G = 1024;                                 // 4 * H

    f32x2 wreg[32][2];
    load_weight_image<NT>(wreg, wout_s4, w, unit, ke, CPM * m + 4 * cq, ks, tid);
    for (int idx = tid; idx < 2 * 256 * M; idx += NT) h_s[idx] = 0.f;
    if (tid < 2 * M) redk[tid] = 0;
    if (tid < 4) cnt_s[tid] = 0;
    float4 genc;                                            // M = 8: the image-side gate constants stay in registers
    {
        const float4 g4 = *reinterpret_cast<const float4*>(w.Genc + (size_t)min(row0 + my_r, B - 1) * G + 4 * unit);
        if constexpr (M == 4) genc_s[tid] = g4; else genc = g4;
    }
    float l_bias[M / 4];
#pragma unroll
    for (int i = 0; i < M / 4; ++i) l_bias[i] = w.boutP[l_v + i];
    float c_own = 0.f, h_own = 0.f;
    unsigned fin = 0;                                       // bit r: row r has emitted END (or does not exist)
#pragma unroll
    for (int r = 0; r < M; ++r)
        if (row0 + r >= B) fin |= 1u << r;
    u64_t* xg = p.xchg + (size_t)group * 2 * M * GRAN;
    const bool own_row = row0 + m < B;                      // this member writes the ids of row m
    int32_t* ids_row = (p.ids && own_row) ? p.ids + (size_t)(row0 + m) * T : nullptr;
    float* lrow = (FULL && p.logits && row0 + l_row < B && l_v < V) ? p.logits + (size_t)(row0 + l_row) * T * V + l_v
                                                                    : nullptr;
    // placement: are the members on one XCD?  (equal ids switch the granule stores to the L2-local flavour)
    __syncthreads();                                        // the LDS initialisation above
    if (wave == 0) {
        const Placement pl = group_placement<M>(xg, GRAN, GRAN_X, m, p.opts);
        if (lane == 0) {
            cnt_s[3] = (pl.one_xcd && !pl.timed_out) ? 1 : 0;
            if (pl.timed_out) cnt_s[2] = 1;
            if (m == 0 && !pl.timed_out)
                report_group(p.status, p.n_groups, p.resident_flag, p.resident_value, pl.one_xcd && !p.opts.agent_scope);
        }
    }
    __syncthreads();
    const bool local = cnt_s[3] != 0 && !p.opts.agent_scope;

    // token of the row this lane's cell belongs to and its table row, gathered as early as the token is known
    int mytok = min(max(p.tok0[min(row0 + my_r, B - 1)], 0), V - 1);
    if (FULL && p.forced) mytok = min(max(p.forced[(size_t)min(row0 + my_r, B - 1) * T], 0), V - 1);
    float4 pvec = *reinterpret_cast<const float4*>(w.P + (size_t)mytok * G + 4 * unit);

    int t = 0;
    bool failed = cnt_s[2] != 0;
    I2L_STAMPS_BEGIN;
    for (; !failed; ++t) {
        // ---- A. token-independent part of the gates of step t: sum_k h(t-1)[k] Whh[k][.]; on the way, the tokens chosen
        //         at step t-1: every wave polls the M x M candidate granules {member q, row r} = lane M q + r itself
        f32x2 acc[M / 4][4][2];
#pragma unroll
        for (int hf = 0; hf < M / 4; ++hf)
#pragma unroll
            for (int g = 0; g < 4; ++g) { acc[hf][g][0] = splat2(0.f); acc[hf][g][1] = splat2(0.f); }
        const float* hprev = h_s + ((t - 1) & 1) * 256 * M;
        const u64_t* cand_src = xg + (size_t)((t - 1) & 1) * M * GRAN + (size_t)((lane / M) & (M - 1)) * GRAN + GRAN_C +
                                (lane & (M - 1));
        const unsigned c_epoch = (unsigned)t;               // candidates of step t-1 carry tag t
        bool have = t == 0;                                 // tokens of step t-1 known (wave-uniform)
        int tk[M] = {};
        // The poll is split in two so that the L2 round trip of the sc1 loads hides behind the product: issue() sends the
        // M x M loads, check() -- some k batches later -- looks at what came back: all granules there -> merge (members
        // own disjoint index ranges: any order), broadcast the M tokens, start the gather of this lane's table row.
        u64_t gv = 0;
        auto issue = [&]() {
            if (lane < M * M) gv = load_granule(cand_src);
        };
        auto check = [&]() {
            if (!__all(lane >= M * M || (unsigned)(gv >> 48) == c_epoch)) return;
            u64_t best;
            if constexpr (M == 4) {                         // 16 granules: lanes 4q + r, merged by DPP row shifts
                const int g_lo = (int)(unsigned)gv, g_hi = (int)(unsigned)(gv >> 32);
                best = am_key(__int_as_float(g_lo), g_hi & 0xFFFF);
                best = umax64(best, am_key(__int_as_float(__builtin_amdgcn_mov_dpp(g_lo, DPP_SHL4, 0xF, 0xF, true)),
                                           __builtin_amdgcn_mov_dpp(g_hi, DPP_SHL4, 0xF, 0xF, true) & 0xFFFF));
                best = umax64(best, am_key(__int_as_float(__builtin_amdgcn_mov_dpp(g_lo, DPP_SHL8, 0xF, 0xF, true)),
                                           __builtin_amdgcn_mov_dpp(g_hi, DPP_SHL8, 0xF, 0xF, true) & 0xFFFF));
                best = umax64(best, am_key(__int_as_float(__builtin_amdgcn_mov_dpp(g_lo, DPP_SHL12, 0xF, 0xF, true)),
                                           __builtin_amdgcn_mov_dpp(g_hi, DPP_SHL12, 0xF, 0xF, true) & 0xFFFF));
            } else {                                        // 64 granules: lanes 8q + r
                best = am_key(__uint_as_float((unsigned)gv), (int)((unsigned)(gv >> 32) & 0xFFFFu));
                best = umax64(best, dpp_u64<DPP_SHL8>(best));    // lanes 0..7 of a 16-lane row: members 2j, 2j + 1
                best = umax64(best, (u64_t)__shfl_xor((unsigned long long)best, 16));
                best = umax64(best, (u64_t)__shfl_xor((unsigned long long)best, 32));
            }
            const int bi = am_idx(best);                    // lanes 0..M-1: the token of row = lane
#pragma unroll
            for (int r = 0; r < M; ++r) {
                tk[r] = __builtin_amdgcn_readlane(bi, r);
                tk[r] = tk[r] < V ? tk[r] : 0;
            }
            have = true;
            if (t < T) {
                mytok = tk[0];
#pragma unroll
                for (int r = 1; r < M; ++r) mytok = my_r == r ? tk[r] : mytok;
                if (FULL && p.forced) mytok = min(max(p.forced[(size_t)min(row0 + my_r, B - 1) * T + t], 0), V - 1);
                pvec = *reinterpret_cast<const float4*>(w.P + (size_t)mytok * G + 4 * unit);
            }
        };
        if (t > 0 && t < T) {
            // the peers published their candidates about when this member did: ask early, look a few batches later
            // (M = 4: 8 batches, polls at 1 / 4 / 7; M = 8: 16 batches, polls at 2 / 8 / 14)
            constexpr int NB = 2 * M;
            auto poll = [&](int b) {
                if (b == NB / 8) issue();
                if (b == NB / 2) { check(); if (!have) issue(); }
                if (b == NB - NB / 8 && !have) check();
            };
            if constexpr (M == 4) rec_product4(acc[0], wreg, reinterpret_cast<const float4*>(hprev) + ke, poll);
            else rec_product8(acc, wreg, reinterpret_cast<const float4*>(hprev) + 2 * ke, poll);
        }
        I2L_STAMP(0);
        // ---- B. wait for the tokens if they are not there yet.  A wave whose poll times out does NOT leave on its own:
        //         it raises cnt_s[2], skips the rest of the step's work and meets the others at the step's barrier, after
        //         which every wave leaves together (uniform barrier use on the failure path too)
        bool bail = false;
        if (!have) {
            PollClock clk;
            for (;;) {
                issue();
                check();
                if (have) break;
                if (clk.expired(p.opts.limit_step)) { bail = true; break; }
            }
            if (bail) cnt_s[2] = 1;
        }
        if (t > 0 && !bail) {
            bool all_fin = true;
#pragma unroll
            for (int r = 0; r < M; ++r) {
                const bool was_fin = (fin >> r) & 1u;
                if (r == m && tid == 0 && ids_row) ids_row[t - 1] = (p.stop == I2L_STOP_STICKY && was_fin) ? -1 : tk[r];
                if (tk[r] == p.end_id) fin |= 1u << r;
                all_fin = all_fin && ((fin >> r) & 1u);
            }
            if (t == T || (p.stop == I2L_STOP_STICKY && all_fin)) break;
        }
        I2L_STAMP(1);
        // ---- C. fold the 8 k-slices into the gates of (unit, row my_r), LSTM cell, publish h
        const unsigned epoch = (unsigned)t + 1u;
        const int par = t & 1;
        u64_t* slot = xg + (size_t)par * M * GRAN;
        float* hcur = h_s + par * 256 * M;
        if (!bail) {
            float z[4];                                     // gates (i, f, g, o); M = 4: valid on lanes ke < 4
            if constexpr (M == 4) {
                genc = genc_s[tid];
                float zf[2];                                // lanes ke < 4: gates (i, f); ke >= 4: (g, o); row ke & 3
                fold_gates4(acc[0], ke, zf);
                z[0] = zf[0]; z[1] = zf[1];
                z[2] = dpp_f<DPP_SHL4>(zf[0]); z[3] = dpp_f<DPP_SHL4>(zf[1]);   // (g, o) from lane ke + 4
            } else {
                fold_gates8(acc, ke, z);
            }
            const float xi = (z[0] + genc.x) + pvec.x, xf = (z[1] + genc.y) + pvec.y;
            const float xc = (z[2] + genc.z) + pvec.z, xo = (z[3] + genc.w) + pvec.w;
            const float ig = sigmoidf_(xi), fg = sigmoidf_(xf), gg = tanhf_(xc), og = sigmoidf_(xo);
            // the cell state's rounding, written out (left to contraction it follows the surrounding code): M = 4 rounds
            // both products, M = 8 fuses fg * c -- what the 4- and 8-member kernels have always computed
            if constexpr (M == 4) {
#pragma clang fp contract(off)
                c_own = fg * c_own + ig * gg;
            } else {
                c_own = __builtin_fmaf(fg, c_own, ig * gg);
            }
            h_own = og * tanhf_(c_own);
            if (ke < M) {
                const int gi = M == 8 ? tid : ul * M + ke;  // granule (unit ul, row ke) = h_s[k = UPM m + ul][row ke]
                store_granule(slot + (size_t)m * GRAN + gi, granule(epoch, h_own), local);
                hcur[m * 256 + gi] = h_own;
            }
        }
        I2L_STAMP(2);
        // ---- D. the other members' h: M = 4: threads 0..255 fetch peers 0 and 1, threads 256..511 peer 2; M = 8: every
        //         thread fetches granule `tid` of each of the seven peers
        if (!bail) {
            if constexpr (M == 4) {
                u64_t gr[2];
                const int gi = tid & 255;
                const int qa = tid < 256 ? 0 : 2;
                const u64_t* pa_ = slot + (size_t)(qa + (qa >= m ? 1 : 0)) * GRAN + gi;
                const u64_t* pb_ = slot + (size_t)(1 + (1 >= m ? 1 : 0)) * GRAN + gi;
                PollClock clk;
                for (;;) {
                    gr[0] = load_granule(pa_);
                    gr[1] = tid < 256 ? load_granule(pb_) : gr[0];
                    if ((unsigned)(gr[0] >> 32) == epoch && (unsigned)(gr[1] >> 32) == epoch) break;
                    if (clk.expired(p.opts.limit_step)) { cnt_s[2] = 1; break; }
                }
                I2L_STAMP(3);
                hcur[(qa + (qa >= m ? 1 : 0)) * 256 + gi] = __uint_as_float((unsigned)gr[0]);
                if (tid < 256) hcur[(1 + (1 >= m ? 1 : 0)) * 256 + gi] = __uint_as_float((unsigned)gr[1]);
            } else {
                u64_t gr[7];
                const u64_t* src[7];
#pragma unroll
                for (int q = 0; q < 7; ++q) src[q] = slot + (size_t)(q + (q >= m ? 1 : 0)) * GRAN + tid;
                PollClock clk;
                for (;;) {
                    bool ok = true;
#pragma unroll
                    for (int q = 0; q < 7; ++q) gr[q] = load_granule(src[q]);
#pragma unroll
                    for (int q = 0; q < 7; ++q) ok = ok && (unsigned)(gr[q] >> 32) == epoch;
                    if (ok) break;
                    if (clk.expired(p.opts.limit_step)) { cnt_s[2] = 1; break; }
                }
                I2L_STAMP(3);
#pragma unroll
                for (int q = 0; q < 7; ++q) hcur[(q + (q >= m ? 1 : 0)) * 256 + tid] = __uint_as_float((unsigned)gr[q]);
            }
        }
        __syncthreads();                                    // THE barrier of the step: h(t) complete in hcur
        if (cnt_s[2] != 0) { failed = true; break; }        // some wave's poll timed out: everybody leaves here
        I2L_STAMP(4);

        // ---- E. logits of this member's CPM columns: thread = (4 columns, k = ks mod 16), M rows -> 4 M sums, folded to
        //         the lane's logit(s) of row l_row; key = (max, first column) over the lanes that share the row
        u64_t key;
        bool adds;                                          // the lane that adds the row's key in F
        if constexpr (M == 4) {
            f32x2 pa[4][2];
            logits_product4<NT>(pa, wout_s4, reinterpret_cast<const float4*>(hcur) + ks, tid);
            I2L_STAMP(5);
            float lv = fold_logits4(pa, ks) + l_bias[0];
            if (lrow) lrow[(size_t)t * V] = lv;
            if (p.use_temp) lv = lv / p.temperature;
            key = am_key(lv, l_v);
            key = umax64(key, dpp_u64<DPP_ROR4>(key));      // the 4 lanes of a 16-lane row that share the row (lane & 3)
            key = umax64(key, dpp_u64<DPP_ROR8>(key));
            adds = ks < 4;
        } else {
            f32x2 pa[2][4][2];
            logits_product8<NT>(pa, wout_s4, reinterpret_cast<const float4*>(hcur) + 2 * ks, tid);
            I2L_STAMP(5);
            float lv[2];
            fold_logits8(pa, ks, lv);
            lv[0] += l_bias[0];
            lv[1] += l_bias[1];
            if (p.use_temp) { lv[0] = lv[0] / p.temperature; lv[1] = lv[1] / p.temperature; }
            key = umax64(am_key(lv[0], l_v), am_key(lv[1], l_v + 1));
            key = umax64(key, dpp_u64<DPP_XOR1>(key));      // the two lanes (ks & 1 = 0, 1) that share (column quad, row)
            adds = (ks & 1) == 0;
        }
        // ---- F. arg max of the member's columns per row: LDS atomic max of the wave's (row, column quad) keys; the wave
        //         that adds last publishes the M candidates and clears the other parity for step t+1
        if (adds) atomicMax(reinterpret_cast<unsigned long long*>(redk + par * M + l_row), (unsigned long long)key);
        int arrived = 0;
        if (lane == 0) arrived = atomicAdd(cnt_s + par, 1);   // LDS operations of a wave execute in order
        arrived = __builtin_amdgcn_readfirstlane(arrived);
        if (arrived == NT / 64 - 1) {
            if (lane < M) {
                const u64_t best = redk[par * M + lane];
                store_granule(slot + (size_t)m * GRAN + GRAN_C + lane,
                              granule((epoch << 16) | (unsigned)(am_idx(best) & 0xFFFF), am_val(best)), local);
                redk[(par ^ 1) * M + lane] = 0;
            }
            if (lane == 0) cnt_s[par ^ 1] = 0;
        }
        I2L_STAMP(6);
    }
#ifdef I2L_GROUP_STAMPS
    if (tid == 0 && blockIdx.x < 32) for (int i = 0; i < 8; ++i) p.status[8 + blockIdx.x * 8 + i] = (unsigned)st_.acc[i];
#endif
    // loud failure: NaN logits too (a caller that asked for logits only -- the validation forward -- gets a NaN loss
    // instead of a partly written tensor)
    greedy_finish<NT>(ids_row, failed, t, T, p.status, lrow, V);
}
