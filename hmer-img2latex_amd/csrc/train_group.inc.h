// Grouped training recurrences (included by train_decoder.hip inside its anonymous namespace): the forward
// recurrence and the BPTT of the L = 1, H = 256 LSTM with the same 4-workgroups-share-R-rows scheme as the grouped
// decode kernel (decode_group.inc.h) -- W_hh lives in registers for all T steps, one tagged-granule exchange per
// step inside the group, placement measured through HW_REG_XCC_ID, every poll bounded (group_seat, PollClock and
// group_placement from group_common.inc.h).
//   forward : member m owns hidden units 64m..64m+63: gates = GX[t] + h . Whh^T (its 256 gate columns, R rows),
//             cell, stores ACT / C / Hout / Hprev, publishes its 64 x R h values.
//   backward: member m owns the same units: gate gradients from (dh, dc) for its units, stores DG, publishes its
//             256 x R gate gradients; dh_{t-1}[own units] = sum over ALL 1024 gate rows n of Whh[n][unit] dG[n].
// A timed-out wait raises status[0] and fills the outputs of the affected rows with NaN (the loss turns NaN).
//
// Rows per group R follow the batch (train_group_rows): 1 up to 64 rows, 2 up to 128, 4 above.  With four rows per
// group 64 rows keep only 64 of the 256 CUs busy and a step is bound by the in-group exchange plus the 4-row product
// (0.85 us of packed FMAs); two rows per group spread the same batch over 128 CUs and halve the product and every
// exchange, one row per group over all 256 CUs.  Both directions are one kernel template each; what depends on R is
// the register image of W_hh, the packed-FMA step, the fold after it and the LDS position map (the pieces below).
// R = 2 and R = 4 do the same per-row arithmetic (bit-identical results); R = 1 sums in k pairs (see TrainRows).
#include "group_common.inc.h"

constexpr int TGT = 512;                       // threads per workgroup

// Granules per member and step: forward h [unit 64][row R] + placement line (at 64 R + 16); backward gate gradients
// [gate 4][unit 64][row R] + placement line (at 256 R).
__host__ __device__ constexpr int tgf_gran(int R) { return 64 * R + 32; }
__host__ __device__ constexpr int tgb_gran(int R) { return 256 * R + 16; }
// rows per group of a grouped recurrence over B rows: 1 up to 64 rows (all 256 CUs on a 64-row shard), 2 up to 128, 4 above
inline int train_group_rows(int B) { return B <= 64 ? 1 : (B <= 128 ? 2 : 4); }

struct TrainGroupFwd {
    int B, T, n_groups;
    const float* GX;      // [B*T][4H] gate-interleaved input gates (biases included)
    const float* WhhT;    // [H][4H] gate-interleaved transpose
    float* ACT; float* C; float* Hout; float* Hprev;
    u64_t* xchg;          // [n_groups][2][4][tgf_gran(R)]
    unsigned* status;
    GroupOpts opts;       // poll limits, exchange flavour (group_common.inc.h)
};
struct TrainGroupBwd {
    int B, T, n_groups;
    const float* ACT; const float* C; const float* dHtop;
    const float* Whh;     // (4H, H) as stored by nn.LSTM
    float* DG;            // [B*T][4H] standard gate order
    u64_t* xchg;          // [n_groups][2][4][tgb_gran(R)]
    unsigned* status;
    GroupOpts opts;       // poll limits, exchange flavour (group_common.inc.h)
};

// The product of both directions: a thread (lane `ke` of 8 forward, `ns` of 32 backward: lane stride S) walks the k
// (forward) or n (backward) rows lane, lane + S, ... of its 4 gate columns (forward) or 4 units (backward) and
// accumulates them into acc[4 values][row pairs].
// R = 2, 4: step c covers row S c; the packed FMA's two halves carry two rows of the batch.  A step's weights are two
// pairs {W[.][v0], W[.][v1]}, {W[.][v2], W[.][v3]} (fma_4x4 / fma_4x2).
// R = 1: the packed FMA has no second row to fill its upper half, so it is filled with a second k instead: a thread's
// weights are stored as pairs {W[k0], W[k1]} (k1 = k0 + S), h (or dG) comes from LDS as the matching pair (the LDS
// image is permuted so that the pair is one 8-byte read: lds_pos), an accumulator holds {sum over its k0s, sum over its
// k1s} and the halves are added before the cross-lane fold.  Per step a thread issues 64 packed FMAs (R = 2: 128) and
// the exchanges halve again.  Summation order differs from R = 2 / 4 (k pairs): results agree to fp32 rounding, not to
// the bit.
template <int R>
struct TrainRows {
    static_assert(R == 1 || R == 2 || R == 4, "rows per group");
    static constexpr int KS = R == 1 ? 16 : 32;    // product steps
    static constexpr int WP = 64 / KS;             // weight pairs per step
    static constexpr int RP = R == 4 ? 2 : 1;      // accumulator row pairs
    typedef typename std::conditional<R == 4, float4, f32x2>::type HV;    // a step's h / dG values in LDS
};

// p points at row `lane` of the walk, at the thread's 4 columns; ld = floats per row
template <int R, int S>
__device__ __forceinline__ void load_whh(f32x2 (&w)[TrainRows<R>::KS][TrainRows<R>::WP], const float* p, int ld) {
    if constexpr (R == 1) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {                 // w[i][v] = {W[2S i][v], W[2S i + S][v]}
            const float4 t0 = *reinterpret_cast<const float4*>(p + (size_t)(2 * S * i) * ld);
            const float4 t1 = *reinterpret_cast<const float4*>(p + (size_t)(2 * S * i + S) * ld);
            w[i][0] = f32x2{t0.x, t1.x}; w[i][1] = f32x2{t0.y, t1.y};
            w[i][2] = f32x2{t0.z, t1.z}; w[i][3] = f32x2{t0.w, t1.w};
        }
    } else {
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float4 t4 = *reinterpret_cast<const float4*>(p + (size_t)(S * j) * ld);
            w[j][0] = f32x2{t4.x, t4.y};
            w[j][1] = f32x2{t4.z, t4.w};
        }
    }
}

// LDS position of element i of the plain image [k or n][row R]; R = 1 pairs k with k + S (one 8-byte read):
// k = 2S a + S s + e lives at ((a S + e) * 2 + s)
template <int R, int S>
__device__ __forceinline__ int lds_pos(int i) {
    if constexpr (R == 1) return (((i / (2 * S)) * S + (i % S)) << 1) + ((i / S) & 1);
    else return i;
}

// acc += the step's weights x its h (or dG) values
template <int R>
__device__ __forceinline__ void fma_step(f32x2 (&acc)[4][TrainRows<R>::RP], const f32x2 (&w)[TrainRows<R>::WP],
                                         typename TrainRows<R>::HV h) {
    if constexpr (R == 4) {
        fma_4x4(acc, w[0], w[1], h);
    } else if constexpr (R == 2) {                     // acc[4 values] (one row pair each) += w4 x h2 (2 rows)
        pkfma_lo(acc[0][0], w[0], h); pkfma_hi(acc[1][0], w[0], h);
        pkfma_lo(acc[2][0], w[1], h); pkfma_hi(acc[3][0], w[1], h);
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) asm("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(acc[v][0]) : "v"(w[v]), "v"(h));
    }
}

// acc = the thread's share of the product: LDS values of step c at hq[S c], read a batch of four steps ahead
template <int R, int S>
__device__ __forceinline__ void row_product(f32x2 (&acc)[4][TrainRows<R>::RP],
                                            const f32x2 (&w)[TrainRows<R>::KS][TrainRows<R>::WP],
                                            const typename TrainRows<R>::HV* hq) {
    constexpr int NB = TrainRows<R>::KS / 4;
    typename TrainRows<R>::HV hb[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) hb[0][i] = hq[S * i];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b + 1 < NB) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hb[(b + 1) & 1][i] = hq[S * ((b + 1) * 4 + i)];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i) fma_step<R>(acc, w[b * 4 + i], hb[b & 1][i]);
    }
}

// The first levels of the fold over a group of 8 lanes (bits of `sel`: the lane within the 8), both directions.
// R = 4: 8 -> 4 -> 2 value pairs: z = (value e of row sel & 3 for e = 0, 1; values 2, 3 sit 4 lanes up)
// R = 2: 8 -> 4 -> 2 -> 1 value per lane: value 2*(sel>>2) + (sel>>1 & 1) of row sel & 1, in z.x
// R = 1: halves, then 4 -> 2 -> 1 value per lane (value 2*(sel>>2) + (sel & 1)), then the two lane pairs add up: z.x
template <int R>
__device__ __forceinline__ f32x2 fold8(const f32x2 (&acc)[4][TrainRows<R>::RP], int sel) {
    const bool b0 = sel & 1, b1 = sel & 2, b2 = sel & 4;
    if constexpr (R == 4) {
        float z[2];
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
        return f32x2{z[0], z[1]};
    } else if constexpr (R == 2) {
        float wv[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float ux = rs_level<DPP_HMIRROR>(acc[e][0].x, acc[2 + e][0].x, b2);
            const float uy = rs_level<DPP_HMIRROR>(acc[e][0].y, acc[2 + e][0].y, b2);
            wv[e] = rs_level<DPP_XOR1>(ux, uy, b0);
        }
        return f32x2{rs_level<DPP_XOR2>(wv[0], wv[1], b1), 0.f};
    } else {
        const float s0 = acc[0][0].x + acc[0][0].y, s1 = acc[1][0].x + acc[1][0].y;
        const float s2 = acc[2][0].x + acc[2][0].y, s3 = acc[3][0].x + acc[3][0].y;
        const float u0 = rs_level<DPP_HMIRROR>(s0, s2, b2), u1 = rs_level<DPP_HMIRROR>(s1, s3, b2);
        const float wv = rs_level<DPP_XOR1>(u0, u1, b0);
        return f32x2{wv + dpp_f<DPP_XOR2>(wv), 0.f};
    }
}

// Gathers the three peers' P granules of step `epoch` from the exchange slot into the LDS image `dst`: thread tid
// takes granules tid, tid + TGT, ... of the 3 P in peer order.  Member q's granule e is element
// (e / 64R) * 256R + 64R q + e % 64R of the plain image (forward [k][row]: e < 64R; backward [n][row]: gate e / 64R).
// Returns false when the poll timed out.
template <int R, int S, int P, int GRAN>
__device__ __forceinline__ bool gather_peers(float* dst, const u64_t* slot, int m, unsigned epoch, long long limit) {
    constexpr int NJ = (3 * P + TGT - 1) / TGT;
    const int tid = threadIdx.x;
    if (tid >= 3 * P) return true;                     // R = 1, 2 forward: fewer granules than threads
    auto has = [&](int j) { return (3 * P) % TGT == 0 || tid + TGT * j < 3 * P; };
    u64_t gr[NJ];
    bool failed = false;
    PollClock clk;
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int e = tid + TGT * j, qi = e / P, q = qi + (qi >= m ? 1 : 0);
            if (has(j)) {
                gr[j] = load_granule(slot + (size_t)q * GRAN + e % P);
                ok = ok && (unsigned)(gr[j] >> 32) == epoch;
            }
        }
        if (ok) break;
        if (clk.expired(limit)) { failed = true; break; }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = tid + TGT * j, qi = e / P, q = qi + (qi >= m ? 1 : 0), g = e % P;
        if (has(j)) dst[lds_pos<R, S>((g / (64 * R)) * 256 * R + 64 * R * q + g % (64 * R))] = __uint_as_float((unsigned)gr[j]);
    }
    return !failed;
}

// Are the four members on one XCD?  (group_placement, group_common.inc.h.)  Returns via LDS word flag[1]; flag[0] is
// set when the wait itself timed out.  Called by every thread; contains a barrier.  No placement statistics.
__device__ __forceinline__ bool group_placement_local(u64_t* xg, int gran, int xslot, int m, int* flag, const GroupOpts& o) {
    if (threadIdx.x < 64) {
        const Placement pl = group_placement<4>(xg, gran, xslot, m, o);
        if (threadIdx.x == 0) { flag[1] = (pl.one_xcd && !pl.timed_out) ? 1 : 0; flag[0] = pl.timed_out ? 1 : 0; }
    }
    __syncthreads();
    return flag[1] != 0;
}

template <int R>
__global__ __launch_bounds__(TGT) void lstm_train_fwd_group_kernel(TrainGroupFwd p) {
    typedef TrainRows<R> TR;
    constexpr int GRAN = tgf_gran(R);
    __shared__ __attribute__((aligned(16))) float h_s[2][256 * R];      // [parity][k][row]: h of the previous step
    __shared__ int flag[4];
    const int tid = threadIdx.x;
    const GroupSeat seat = group_seat<4>();
    const int m = seat.m;
    if (seat.group >= p.n_groups) return;
    const int B = p.B, T = p.T;
    const int row0 = seat.group * R;
    const int ul = tid >> 3, ke = tid & 7, kr = ke & (R - 1);
    const int unit = 64 * m + ul;
    constexpr int G = 1024, H = 256;
    f32x2 w[TR::KS][TR::WP];                                // W_hh^T rows ke, ke + 8, ... of the unit's 4 gate columns
    load_whh<R, 8>(w, p.WhhT + (size_t)ke * G + 4 * unit, G);
    for (int idx = tid; idx < 2 * 256 * R; idx += TGT) (&h_s[0][0])[idx] = 0.f;
    u64_t* xg = p.xchg + (size_t)seat.group * 2 * 4 * GRAN;
    const bool local = group_placement_local(xg, GRAN, 64 * R + 16, m, flag, p.opts) && !p.opts.agent_scope;   // barrier inside: h_s zeroed
    const int row = min(row0 + kr, B - 1);
    const bool live = ke < R && row0 + kr < B;                                  // this lane owns (unit, row kr)
    float c_own = 0.f, h_own = 0.f;
    bool failed = false;
    int t = 0;
    // the input-side gates of step t+1 are requested at the top of step t: with one row per group the recurrent product is
    // only ~0.2 us, far too short to hide an HBM round trip behind
    float4 gx_next = *reinterpret_cast<const float4*>(p.GX + (size_t)row * T * G + 4 * unit);
    for (; t < T; ++t) {
        const size_t bt = (size_t)row * T + t;
        const float4 gx = gx_next;
        if (t + 1 < T) gx_next = *reinterpret_cast<const float4*>(p.GX + (bt + 1) * G + 4 * unit);
        f32x2 acc[4][TR::RP];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int rp = 0; rp < TR::RP; ++rp) acc[g][rp] = splat2(0.f);
        if (t > 0) row_product<R, 8>(acc, w, reinterpret_cast<const typename TR::HV*>(h_s[t & 1]) + ke);
        {
            // lane ke < R ends with the four gate sums of (unit, row ke): R = 4 holds gates i, f and finds g, o 4 lanes up;
            // R = 2 / 1 hold gate i and find f, g, o R, 4 and 4 + R lanes up (row_shl)
            const f32x2 z = fold8<R>(acc, ke);
            float zi = z.x, zf = z.y, zg, zo;
            if constexpr (R == 4) {
                zg = dpp_f<DPP_SHL4>(z.x); zo = dpp_f<DPP_SHL4>(z.y);
            } else {
                zf = dpp_f<0x100 + R>(zi); zg = dpp_f<DPP_SHL4>(zi); zo = dpp_f<0x104 + R>(zi);
            }
            const float ig = sigmoidf_(gx.x + zi), fg = sigmoidf_(gx.y + zf);
            const float gg = tanhf_(gx.z + zg), og = sigmoidf_(gx.w + zo);
            const float h_prev = h_own;
            c_own = fg * c_own + ig * gg;
            h_own = og * tanhf_(c_own);
            if (live) {
                *reinterpret_cast<float4*>(p.ACT + bt * G + 4 * unit) = make_float4(ig, fg, gg, og);
                p.C[bt * H + unit] = c_own;
                p.Hout[bt * H + unit] = h_own;
                p.Hprev[bt * H + unit] = h_prev;
            }
        }
        if (t + 1 == T) break;
        const unsigned epoch = (unsigned)t + 1u;
        u64_t* slot = xg + (size_t)(t & 1) * 4 * GRAN;
        if (ke < R) store_granule(slot + (size_t)m * GRAN + ul * R + ke, granule(epoch, h_own), local);
        float* hn = h_s[(t + 1) & 1];
        if (!gather_peers<R, 8, 64 * R, GRAN>(hn, slot, m, epoch, p.opts.limit_step)) failed = true;
        if (ke < R) hn[lds_pos<R, 8>(m * 64 * R + ul * R + ke)] = h_own;
        if (failed) flag[0] = 1;
        __syncthreads();
        if (flag[0]) { failed = true; break; }
    }
    if (failed || flag[0]) {
        if (tid == 0) atomicOr(p.status, 1u);
        if (live) for (int tt = 0; tt < T; ++tt) p.Hout[((size_t)row * T + tt) * H + unit] = __int_as_float(0x7fc00000);
    }
}

// After the fold every lane of a group of 8 (R = 4: of 16) holds dh of one (unit 4 jq + o_col, row o_row); the owner
// lanes, one per (unit, row), run the cell backward for it.
struct BwdLane {
    int o_row, o_col;
    bool owner;
};
template <int R>
__device__ __forceinline__ BwdLane bwd_lane(int ns) {
    if constexpr (R == 4) return {ns & 3, ((ns >> 2) & 1) * 2 + ((ns >> 3) & 1), ns < 16};
    else if constexpr (R == 2) return {ns & 1, ((ns >> 2) & 1) * 2 + ((ns >> 1) & 1), ns < 8};
    else return {0, ((ns >> 2) & 1) * 2 + (ns & 1), (ns & ~5) == 0};
}

template <int R>
__global__ __launch_bounds__(TGT) void lstm_train_bwd_group_kernel(TrainGroupBwd p) {
    typedef TrainRows<R> TR;
    constexpr int GRAN = tgb_gran(R);
    __shared__ __attribute__((aligned(16))) float dgs[2][1024 * R];    // [parity][gate row n][row]: gate gradients of a step
    __shared__ int flag[4];
    const int tid = threadIdx.x;
    const GroupSeat seat = group_seat<4>();
    const int m = seat.m;
    if (seat.group >= p.n_groups) return;
    const int B = p.B, T = p.T;
    const int row0 = seat.group * R;
    constexpr int G = 1024, H = 256;
    // product: thread = (unit quad jq, n slice ns): dh[4 units][R rows] += Whh[32 i + ns][units] dG[32 i + ns][rows]
    const int jq = tid >> 5, ns = tid & 31;
    f32x2 w[TR::KS][TR::WP];
    load_whh<R, 32>(w, p.Whh + (size_t)ns * H + 64 * m + 4 * jq, H);
    const BwdLane ln = bwd_lane<R>(ns);
    const int o_row = ln.o_row;
    const int ul = 4 * jq + ln.o_col, unit = 64 * m + ul;
    const int row = min(row0 + o_row, B - 1);
    const bool owner = ln.owner, live = owner && row0 + o_row < B;
    u64_t* xg = p.xchg + (size_t)seat.group * 2 * 4 * GRAN;
    const bool local = group_placement_local(xg, GRAN, 256 * R, m, flag, p.opts) && !p.opts.agent_scope;
    float dh_rec = 0.f, dc_next = 0.f;
    bool failed = false;
    // what the cell backward of step t-1 reads (activations, cell states, dh from above) is requested during step t
    float4 a_nx = make_float4(0.f, 0.f, 0.f, 0.f);
    float c_nx = 0.f, cp_nx = 0.f, dht_nx = 0.f;
    auto prefetch = [&](int tt) {
        if (!owner || tt < 0) return;
        const size_t b2 = (size_t)row * T + tt;
        a_nx = *reinterpret_cast<const float4*>(p.ACT + b2 * G + 4 * unit);
        c_nx = p.C[b2 * H + unit];
        cp_nx = tt > 0 ? p.C[(b2 - 1) * H + unit] : 0.f;
        dht_nx = p.dHtop[b2 * H + unit];
    };
    prefetch(T - 1);
    for (int t = T - 1; t >= 0; --t) {
        const int par = t & 1;
        const unsigned epoch = (unsigned)(T - t);
        const size_t bt = (size_t)row * T + t;
        u64_t* slot = xg + (size_t)par * 4 * GRAN;
        float* dcur = dgs[par];
        const float4 a = a_nx;
        const float c = c_nx, cp = cp_nx, dht = dht_nx;
        prefetch(t - 1);
        if (owner) {
            const float dh = dh_rec + dht;
            const float tc = tanhf_(c);
            const float d_o = dh * tc * a.w * (1.f - a.w);
            const float dc = dh * a.w * (1.f - tc * tc) + dc_next;
            const float d_i = dc * a.z * a.x * (1.f - a.x);
            const float d_f = dc * cp * a.y * (1.f - a.y);
            const float d_g = dc * a.x * (1.f - a.z * a.z);
            dc_next = dc * a.y;
            const float dgv[4] = {d_i, d_f, d_g, d_o};
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (live) p.DG[bt * G + g * H + unit] = dgv[g];
                dcur[lds_pos<R, 32>((g * 256 + 64 * m + ul) * R + o_row)] = dgv[g];
                if (t > 0) store_granule(slot + (size_t)m * GRAN + (g * 64 + ul) * R + o_row, granule(epoch, dgv[g]), local);
            }
        }
        if (t == 0) break;
        if (!gather_peers<R, 32, 256 * R, GRAN>(dcur, slot, m, epoch, p.opts.limit_step)) failed = true;
        if (failed) flag[0] = 1;
        __syncthreads();
        if (flag[0]) { failed = true; break; }
        // dh_{t-1}[own units] = sum_n Whh[n][unit] dG[n]
        f32x2 acc[4][TR::RP];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int rp = 0; rp < TR::RP; ++rp) acc[g][rp] = splat2(0.f);
        row_product<R, 32>(acc, w, reinterpret_cast<const typename TR::HV*>(dcur) + ns);
        {
            const f32x2 z = fold8<R>(acc, ns);                        // the 8 n slices of this lane's group of 8 folded
            float v;
            if constexpr (R == 4) v = rs_level<DPP_ROR8>(z.x, z.y, ns & 8);      // n slices 0..15 (or 16..31) folded
            else v = z.x + dpp_f<DPP_ROR8>(z.x);                      // + the other group of 8 of the 16-lane row
            dh_rec = v + __shfl_xor(v, 16);                           // + the other 16 slices
        }
    }
    if (failed || flag[0]) {
        if (tid == 0) atomicOr(p.status, 1u);
        if (live) for (int tt = 0; tt < T; ++tt) p.DG[((size_t)row * T + tt) * G + unit] = __int_as_float(0x7fc00000);
    }
}
