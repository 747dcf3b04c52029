// Grouped greedy decode on the MATRIX CORES: SIXTEEN members x SIXTEEN rows per group (included by decode.hip inside its
// anonymous namespace, after decode_group.inc.h).  r04; reference decoder.py:247-250,277-280 (LSTM gates, Linear(H -> V)),
// seq2seq.py:210-221 (arg max loop).
//
// Why: in the co-resident pipeline (decode(i) beside the conv workgroups of encoder(i + 1) on every CU) the 8-member
// kernel's per-step products are v_pk_fma_f32 bursts, and a vector burst beside resident conv waves -- which keep the
// vector ALUs busy splitting and staging their own operands -- takes 2.1x its time alone, while the same products as a
// burst of v_mfma_f32_16x16x32_bf16 take 1.13x (profiles/r04/coresident_mfma.txt).  With 16 rows per group the MFMA's
// M = 16 is full, so the split-bf16 form (3 bf16 pieces per fp32 operand, 6 partial products, fp32 accumulation: the
// error class of an fp32 fmaf chain, section "Split-bf16" of DESIGN.md) costs 6/8 of the packed-FMA time instead of 12/8.
//
// A member holds a SIXTEENTH of the weights, pre-split into bf16 pieces, in registers for the whole loop -- as the B
// operands of the MFMAs, in the matrix cores' own lane layout (lane l: B[k = 32 ks + 8 (l >> 4) + j][column l & 15]).
// Every wave w holds the same amount (144 registers):
//     WhhT[:, the 16 gate columns of hidden units 16m + 4w .. +3]                8 k-steps x 3 pieces x 4 registers = 96
//     WoutT[k half (w >> 1), vocabulary columns 32m + 16 (w & 1) .. +15]         4 k-steps x 3 pieces x 4 registers = 48
// h travels as its three bf16 pieces: an exchange granule is {tag 16 | p0 16 | p1 16 | p2 16} (h = p0 + p1 + p2 exactly),
// so nobody splits anything but the lane that computed the value, and LDS holds h only in operand layout:
//     hp[parity][piece][k block of 8][row 16][8]  (a lane's A fragment = one 16-byte read, conflict-free)
// Per step t (one barrier, as in the other grouped kernels):
//   A  gates(t)[16 rows x 16 columns per wave] = h(t-1) . WhhT  (48 MFMAs per wave) -- token independent, so it runs
//      while the candidates of step t-1 are in flight; every wave polls the 16 x 16 candidate granules itself
//   B  tokens of step t-1 (ids out, stop rule)
//   C  4 x 4 transposition inside lane quads brings the four gates of (unit, row) to one lane: ONE cell per lane, + Genc
//      + P[token], h(t) -> pieces -> granule (exchange 1) and own slice of hp
//   D  all threads: the other fifteen sixteenths of h(t): 64-byte runs (8 units of one row) -> three 16-byte LDS stores
//   -- barrier --
//   E  logits(t)[16 rows x 16 columns] = h(t) . WoutT, each wave half of the reduction of one column tile (24 MFMAs);
//      waves 2, 3 hand their partial sums to waves 0, 1 through LDS (an in-order write + flag, no barrier), which add,
//      take the arg max over the 16 lanes of a row, LDS atomic max across the two waves, and the later one publishes the
//      member's 16 candidates (exchange 2); waves 2, 3 are already in A of step t + 1.
// Tags, two buffers by step parity, bounded polls, placement measurement, failure marking (ids -3), residency signal:
// exactly as decode_group_kernel<8>.  Supported: ids out (both stop rules, temperature, arg max of logits / of softmax);
// no logits output, no forced tokens, no initial / returned state.
// decode_group16_kernel<2> (below) runs TWO batches per launch, a range of the steps of each; <1> is this kernel.
#include "mfma_slab.inc.h"      // bf16_split.inc.h, f32x4_t / u32x4_t, Frag16

constexpr int G16Q = 16;                   // members = rows per row tile of a group
constexpr int G16NT = 256;                 // threads per workgroup
constexpr int G16_HP_PIECE = 32 * 16 * 8;  // bf16 elements of one piece image
// Exchange and LDS of decode_group16_kernel<RT>, RT row tiles of 16 rows per group
template <int RT>
struct G16Shape {
    static_assert(RT == 1 || RT == 2, "row tiles per group");
    static constexpr int GRAN_H = 256 * RT;           // h granules per member and step: [tile RT][k block 2][row 16][unit in block 8]
    static constexpr int GRAN_C = GRAN_H;             // 16 RT candidate granules [tile][row], lines of their own
    static constexpr int GRAN_X = GRAN_H + 16 * RT;   // placement granule
    static constexpr int GRAN = GRAN_H + 32 * RT;
    // LDS: hp [2][3 pieces][32][16][8] bf16 (48 KB; the two images are the step parities for RT = 1 and the row tiles for
    // RT = 2) | partial logits [2 column tiles][64 lanes][4] | arg-max keys [2 parities][RT][16] | counters
    static constexpr size_t LDS = (size_t)2 * 3 * G16_HP_PIECE * 2 + (size_t)2 * 64 * 16 + (size_t)2 * RT * 16 * 8 + 8 * sizeof(int);
    static constexpr size_t XCHG_PER_GROUP = (size_t)2 * G16Q * GRAN * 8;
};
constexpr size_t GRP16_LDS = G16Shape<1>::LDS;
constexpr size_t GROUP16_XCHG_PER_GROUP = G16Shape<1>::XCHG_PER_GROUP;

// State block of a batch between the two launches that run its steps (decode_group16_kernel<2>), rows padded to whole
// groups: c [rows][256] fp32 | h [rows][256] fp32 | last token [rows] | fin mask [groups] | failed [groups]
__host__ __device__ constexpr size_t group16_state_rows(int rows) { return (size_t)((rows + G16Q - 1) / G16Q) * G16Q; }
__host__ __device__ constexpr size_t group16_state_bytes(int rows) {
    return group16_state_rows(rows) * (2 * 256 * sizeof(float) + sizeof(int)) + group16_state_rows(rows) / G16Q * 2 * sizeof(unsigned);
}
struct G16State {
    float* c; float* h; int* tok; unsigned* fin; unsigned* failed;
};
__device__ __forceinline__ G16State group16_state(const void* base, int rows) {
    const size_t rp = group16_state_rows(rows);
    G16State s;
    s.c = static_cast<float*>(const_cast<void*>(base));
    s.h = s.c + rp * 256;
    s.tok = reinterpret_cast<int*>(s.h + rp * 256);
    s.fin = reinterpret_cast<unsigned*>(s.tok + rp);
    s.failed = s.fin + rp / G16Q;
    return s;
}

// 16 bytes = two granules, L1 bypassed like load_granule's sc1 polls (each 8-byte half is one peer store: no tearing)
__device__ __forceinline__ void load_run64(const u64_t* src, u32x4_t (&g)[4]) {
    asm volatile(
        "global_load_dwordx4 %0, %4, off sc1\n\t"
        "global_load_dwordx4 %1, %4, off offset:16 sc1\n\t"
        "global_load_dwordx4 %2, %4, off offset:32 sc1\n\t"
        "global_load_dwordx4 %3, %4, off offset:48 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3])
        : "v"(src)
        : "memory");
}

// weight-only preparation (i2l_decoder_prepare, I2L_PREP_WEIGHTS): every (member, wave, lane)'s 36 operand fragments --
// 24 of W_hh^T (8 k-steps x 3 pieces), 12 of W_out^T (4 k-steps x 3 pieces) -- split once and stored lane-contiguously, so
// that the kernel's prologue is 36 coalesced 16-byte loads per lane instead of 192 strided 4-byte loads + 192 splits
// (60 us of every launch, during which the next batch's encoder waits for the decode to report itself resident)
__global__ __launch_bounds__(64) void pack16_kernel(const float* __restrict__ WhhT, const float* __restrict__ WoutT,
                                                    u32x4_t* __restrict__ pack) {
    const int m = blockIdx.x >> 2, wave = blockIdx.x & 3, lane = threadIdx.x;
    const int lhi = lane >> 4, lcol = lane & 15, ltile = wave & 1, lhalf = wave >> 1;
    u32x4_t* dst = pack + (size_t)blockIdx.x * 36 * 64 + lane;
    const float* src = WhhT + 64 * m + 16 * wave + lcol;
    for (int ks = 0; ks < 8; ++ks) {
        Frag16 f0, f1, f2;
#pragma unroll
        for (int j = 0; j < 8; ++j) split3(src[(size_t)(32 * ks + 8 * lhi + j) * 1024], f0.s[j], f1.s[j], f2.s[j]);
        dst[(ks * 3 + 0) * 64] = f0.q; dst[(ks * 3 + 1) * 64] = f1.q; dst[(ks * 3 + 2) * 64] = f2.q;
    }
    const float* srl = WoutT + 32 * m + 16 * ltile + lcol;
    for (int ks = 0; ks < 4; ++ks) {
        Frag16 f0, f1, f2;
#pragma unroll
        for (int j = 0; j < 8; ++j) split3(srl[(size_t)(32 * (4 * lhalf + ks) + 8 * lhi + j) * 512], f0.s[j], f1.s[j], f2.s[j]);
        dst[(24 + ks * 3 + 0) * 64] = f0.q; dst[(24 + ks * 3 + 1) * 64] = f1.q; dst[(24 + ks * 3 + 2) * 64] = f2.q;
    }
}

// two runs at once: both tasks of a thread in flight together (one L2 round trip instead of two)
__device__ __forceinline__ void load_run64x2(const u64_t* s0, const u64_t* s1, u32x4_t (&g)[8]) {
    asm volatile(
        "global_load_dwordx4 %0, %8, off sc1\n\t"
        "global_load_dwordx4 %1, %8, off offset:16 sc1\n\t"
        "global_load_dwordx4 %2, %8, off offset:32 sc1\n\t"
        "global_load_dwordx4 %3, %8, off offset:48 sc1\n\t"
        "global_load_dwordx4 %4, %9, off sc1\n\t"
        "global_load_dwordx4 %5, %9, off offset:16 sc1\n\t"
        "global_load_dwordx4 %6, %9, off offset:32 sc1\n\t"
        "global_load_dwordx4 %7, %9, off offset:48 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]), "=&v"(g[4]), "=&v"(g[5]), "=&v"(g[6]), "=&v"(g[7])
        : "v"(s0), "v"(s1)
        : "memory");
}
// the same from a UNIFORM base and two 32-bit byte offsets (RT = 2: four tasks per thread -- as 64-bit addresses, for both
// step parities, they would take sixteen registers)
__device__ __forceinline__ void load_run64x2_at(const u64_t* base, unsigned oa, unsigned ob, u32x4_t (&g)[8]) {
    asm volatile(
        "global_load_dwordx4 %0, %8, %10 sc1\n\t"
        "global_load_dwordx4 %1, %8, %10 offset:16 sc1\n\t"
        "global_load_dwordx4 %2, %8, %10 offset:32 sc1\n\t"
        "global_load_dwordx4 %3, %8, %10 offset:48 sc1\n\t"
        "global_load_dwordx4 %4, %9, %10 sc1\n\t"
        "global_load_dwordx4 %5, %9, %10 offset:16 sc1\n\t"
        "global_load_dwordx4 %6, %9, %10 offset:32 sc1\n\t"
        "global_load_dwordx4 %7, %9, %10 offset:48 sc1\n\t"
        "s_waitcnt vmcnt(0)"
        : "=&v"(g[0]), "=&v"(g[1]), "=&v"(g[2]), "=&v"(g[3]), "=&v"(g[4]), "=&v"(g[5]), "=&v"(g[6]), "=&v"(g[7])
        : "v"(oa), "v"(ob), "s"(base)
        : "memory");
}
// 8 granules {tag 16 | p0 | p1 | p2} of one (k block, row) -> the three 16-byte operand rows
__device__ __forceinline__ void unpack_run(const u32x4_t* g, u32x4_t* dst) {
    u32x4_t o0, o1, o2;                 // granule = {low word: p1 << 16 | p2, high word: tag << 16 | p0}
    o0.x = (g[0].y & 0xFFFFu) | (g[0].w << 16); o0.y = (g[1].y & 0xFFFFu) | (g[1].w << 16);
    o0.z = (g[2].y & 0xFFFFu) | (g[2].w << 16); o0.w = (g[3].y & 0xFFFFu) | (g[3].w << 16);
    o1.x = (g[0].x >> 16) | (g[0].z & 0xFFFF0000u); o1.y = (g[1].x >> 16) | (g[1].z & 0xFFFF0000u);
    o1.z = (g[2].x >> 16) | (g[2].z & 0xFFFF0000u); o1.w = (g[3].x >> 16) | (g[3].z & 0xFFFF0000u);
    o2.x = (g[0].x & 0xFFFFu) | (g[0].z << 16); o2.y = (g[1].x & 0xFFFFu) | (g[1].z << 16);
    o2.z = (g[2].x & 0xFFFFu) | (g[2].z << 16); o2.w = (g[3].x & 0xFFFFu) | (g[3].z << 16);
    dst[0] = o0;
    dst[G16_HP_PIECE / 8] = o1;
    dst[2 * (G16_HP_PIECE / 8)] = o2;
}

// RT = 1: the kernel described above.  RT = 2 (i2l_greedy_decode_halves): TWO row tiles of 16 rows per group, each of its
// own batch and with its own range of that batch's steps (HalfTile), as two M-tiles of the same B operands in lock step
// on ONE exchange chain: the two L2 exchanges of a step are paid once for 32 rows.  Inside every phase the tiles are run
// one after the other (fragment and accumulator registers are reused), each with exactly the RT = 1 arithmetic -- same
// MFMA order, same (lo + mid) + hi sums, same arg-max tie rule -- so a batch's ids do not depend on which kernel ran
// which of its steps.  Tags count the launch's own steps s (tile k is at its step t0 + s); a tile with fewer steps than
// the other, or none, keeps publishing tagged granules whose values nobody uses, so no poll ever waits for it.
// hp is SINGLE-buffered for RT = 2 (the 48 KB hold the two tiles' images instead of two parities) and a step has TWO
// barriers.  They suffice because every access to hp falls between them in a fixed way: h(s) is WRITTEN only in phases
// C and D of step s, i.e. after barrier 1 of step s and before barrier 2 of step s; it is READ only in phase E of
// step s and phase A of step s + 1, i.e. after barrier 2 of step s and before barrier 1 of step s + 1.  So no wave
// writes h(s) while another still reads h(s - 1) (barrier 1), and none reads h(s) before it is complete (barrier 2).
// The partial logits pass through the ONE lpart image tile after tile: waves 2, 3 rewrite it for tile 1 only after
// waves 0, 1 acknowledged (cnt_s[6..7]) that they have read tile 0's.
// A batch whose steps are split saves (c, h) as fp32, the last token and the fin mask (G16State) at the end of its first
// range and resumes from them: split3 is exact, so the pieces of the reloaded h are those the first launch held.
template <int RT>
__global__ __launch_bounds__(G16NT, 2) void decode_group16_kernel(GroupParams p) {
    using S = G16Shape<RT>;
    constexpr int GRAN = S::GRAN, GRAN_C = S::GRAN_C, GRAN_X = S::GRAN_X;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    unsigned short* hp = reinterpret_cast<unsigned short*>(smem16);                    // [2][3][32][16][8]
    f32x4_t* lpart = reinterpret_cast<f32x4_t*>(smem16 + (size_t)2 * 3 * G16_HP_PIECE * 2);   // [2 tiles][64 lanes]
    u64_t* redk = reinterpret_cast<u64_t*>(lpart + 2 * 64);                           // [2][RT][16 rows]
    int* cnt_s = reinterpret_cast<int*>(redk + 2 * RT * 16); // [0..1] logit waves arrived (by parity), [2] time-out, [3] one XCD,
                                                             // [4..5] epoch of the partial logits of tile 0 / 1 in lpart,
                                                             // [6..7] (RT = 2) the last partial logits that waves 0 / 1 have read
    const StepWeights& w = p.w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int within = blockIdx.x & 127;
    const int group = (blockIdx.x >> 7) * 8 + (within & 7), m = within >> 3;      // a group's members: block ids 8 apart = one XCD
    if (group >= p.n_groups) return;
    const int V = w.V;
    const int row0 = group * G16Q;
    constexpr int G = 1024;
    const int lq = lane & 3, uq = (lane >> 2) & 3, lhi = lane >> 4, lcol = lane & 15;
    const int cell_row = 4 * lhi + lq;                       // the row of this lane's cell (after the quad transposition)
    const int unit = 16 * m + 4 * wave + uq;                 // ... and its hidden unit
    const int ltile = wave & 1, lhalf = wave >> 1;           // logits: column tile, half of the reduction

    // ---- placement exchange FIRST (r04): a member reports itself before it loads its 147 KB of weights, so that the launch's
    // residency word (count_resident_group) -- which the next batch's encoder stream is waiting for -- is published ~10 us
    // earlier; waves 1-3 start their weight loads meanwhile
    u64_t* xg = p.xchg + (size_t)group * 2 * G16Q * GRAN;
    if (tid < 8) cnt_s[tid] = 0;                             // wave 0: in program order before its writes below
    if (wave == 0) {                                        // placement: are the sixteen members on one XCD?
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xFu;
        if (lane == 0 && !(p.opts.drop_member && m == 3))
            store_granule(xg + (size_t)m * GRAN + GRAN_X, granule(0xC0DEu, __uint_as_float(xcc)), false);
        const int pq = (lane & 15) + ((lane & 15) >= m ? 1 : 0);
        u64_t pv = 0;
        bool bad = false;
        long long t_start = 0;
        unsigned spins = 0;
        for (;;) {
            bool ok = true;
            if (lane < 15) { pv = load_granule(xg + (size_t)pq * GRAN + GRAN_X); ok = (unsigned)(pv >> 32) == 0xC0DEu; }
            if (__all(ok)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 255u) == 0) {
                const long long now = (long long)wall_clock64();
                if (t_start == 0) t_start = now;
                else if (now - t_start > p.opts.limit_first) { bad = true; break; }
            }
        }
        const bool all_same = __all(lane >= 15 || (unsigned)pv == xcc);
        if (lane == 0) {
            cnt_s[3] = (all_same && !bad) ? 1 : 0;
            if (bad) cnt_s[2] = 1;
            if (m == 0 && !bad) {
                count_resident_group(p.status, p.n_groups, p.resident_flag, p.resident_value);
                if (all_same && !p.opts.agent_scope) atomicAdd(p.status + GRP_STAT_LOCAL, 1u);
            }
        }
    }
    // ---- the member's weights, pre-split in B-operand layout by pack16_kernel: 36 coalesced 16-byte loads per lane
    bf16x8_t wg[24], wl[12];                                 // [k-step][piece]
    {
        const u32x4_t* pk = static_cast<const u32x4_t*>(w.wpack16) + (size_t)(m * 4 + wave) * 36 * 64 + lane;
#pragma unroll
        for (int i = 0; i < 24; ++i) { Frag16 f; f.q = pk[i * 64]; wg[i] = f.v; }
        // RT = 2 holds only W_hh^T for the whole loop: the 48 registers of W_out^T are fetched again in every step (below,
        // behind barrier 1), because across phase A -- two tiles' products, 32 candidates -- there is no room for them
        if constexpr (RT == 1) {
#pragma unroll
            for (int i = 0; i < 12; ++i) { Frag16 f; f.q = pk[(24 + i) * 64]; wl[i] = f.v; }
        }
    }
    // ---- the row tiles: RT = 1 the launch's batch, RT = 2 the two HalfTile descriptors
    HalfTile tl[RT];
    if constexpr (RT == 1) tl[0] = HalfTile{w.Genc, p.tok0, p.ids, p.B, p.T, 0, p.T, nullptr, nullptr};
    else { tl[0] = p.tile[0]; tl[1] = p.tile[1]; }
    int nk[RT];                                              // steps of tile k in THIS group (0: none -- absent, no rows here,
    bool mark_failed[RT];                                    // or the launch of its earlier steps failed: rows marked -3)
    float4 genc[RT], pvec[RT];
    float c_own[RT], h_own[RT];
    unsigned fin[RT];
    int mytok[RT];
    int32_t* ids_row[RT];
    int n_steps = 0;                                         // steps of this launch in this group
    if constexpr (RT == 1) {
        for (int idx = tid; idx < 2 * 3 * G16_HP_PIECE / 2; idx += G16NT) reinterpret_cast<unsigned*>(hp)[idx] = 0u;   // h(-1) = 0
    }
    if (tid < 32 * RT) redk[tid] = 0;
    const float l_bias = w.boutP[32 * m + 16 * ltile + lcol];
#pragma unroll
    for (int k = 0; k < RT; ++k) {
        const int B = tl[k].B;
        nk[k] = (RT == 1 || (tl[k].n > 0 && row0 < B)) ? tl[k].n : 0;
        mark_failed[k] = false;
        c_own[k] = 0.f; h_own[k] = 0.f;
        fin[k] = 0;
#pragma unroll
        for (int r = 0; r < G16Q; ++r)
            if (row0 + r >= B) fin[k] |= 1u << r;
        const bool own_row = row0 + m < B;
        ids_row[k] = (tl[k].ids && own_row && nk[k] > 0) ? tl[k].ids + (size_t)(row0 + m) * tl[k].T : nullptr;
        genc[k] = float4{0.f, 0.f, 0.f, 0.f};
        pvec[k] = genc[k];
        mytok[k] = 0;
        if constexpr (RT == 2) {
            unsigned short* hk = hp + (size_t)k * 3 * G16_HP_PIECE;
            const bool resume = nk[k] > 0 && tl[k].t0 > 0;
            if (resume) {
                const G16State st = group16_state(tl[k].state_in, B);
                if (st.failed[group] != 0) { nk[k] = 0; mark_failed[k] = true; }
                else {
                    c_own[k] = st.c[(size_t)(row0 + cell_row) * 256 + unit];
                    h_own[k] = st.h[(size_t)(row0 + cell_row) * 256 + unit];
                    mytok[k] = st.tok[row0 + cell_row];
                    fin[k] = st.fin[group];
                    for (int idx = tid; idx < G16Q * 256; idx += G16NT) {       // the group's h: all 256 units of its 16 rows
                        const int r = idx >> 8, u = idx & 255;
                        unsigned short q0, q1, q2;
                        split3(st.h[(size_t)(row0 + r) * 256 + u], q0, q1, q2);
                        const int o = ((u >> 3) * 16 + r) * 8 + (u & 7);
                        hk[o] = q0;
                        hk[G16_HP_PIECE + o] = q1;
                        hk[2 * G16_HP_PIECE + o] = q2;
                    }
                }
            }
            if (!(resume && !mark_failed[k]))
                for (int idx = tid; idx < 3 * G16_HP_PIECE / 2; idx += G16NT) reinterpret_cast<unsigned*>(hk)[idx] = 0u;   // h(-1) = 0
            if (nk[k] > 0 && tl[k].state_out && m == 0 && tid == 0)
                group16_state(tl[k].state_out, B).failed[group] = 0u;
        }
        if (RT == 1 || nk[k] > 0)
            genc[k] = *reinterpret_cast<const float4*>(tl[k].Genc + (size_t)min(row0 + cell_row, B - 1) * G + 4 * unit);
        n_steps = max(n_steps, nk[k]);
    }

    __syncthreads();
    const bool local = cnt_s[3] != 0 && !p.opts.agent_scope;

#pragma unroll
    for (int k = 0; k < RT; ++k) {
        if (RT == 1 || nk[k] > 0) {
            if (RT == 1 || tl[k].t0 == 0) mytok[k] = tl[k].tok0[min(row0 + cell_row, tl[k].B - 1)];
            mytok[k] = min(max(mytok[k], 0), V - 1);
            pvec[k] = *reinterpret_cast<const float4*>(w.P + (size_t)mytok[k] * G + 4 * unit);
        }
    }

    int t = 0;                                               // the launch's step; tile k is at its step tl[k].t0 + t
    bool failed = cnt_s[2] != 0;
#ifdef I2L_GROUP_STAMPS
    long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long st_last = (long long)wall_clock64();
#define I2L_STAMP16(i) do { const long long n_ = (long long)wall_clock64(); st_acc[i] += n_ - st_last; st_last = n_; } while (0)
#else
#define I2L_STAMP16(i) do { } while (0)
#endif
    for (; !failed && (RT == 1 || n_steps > 0); ++t) {
        // ---- A. gates(t) = h(t-1) . WhhT on the matrix cores; on the way every wave polls the 256 RT candidate granules of
        //         step t-1 -- lane (row l & 15, members 4 (l >> 4) .. +3, every tile) -- and merges them into the 16 RT tokens
        f32x4_t acc[RT][3];                                 // hi | mid | lo partial products (RT = 2: [0] their sum)
        bool live[RT];
        bool any_live = false;
#pragma unroll
        for (int k = 0; k < RT; ++k) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[k][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            live[k] = t < nk[k];
            any_live = any_live || live[k];
        }
        const u64_t* cand_src = xg + (size_t)((t - 1) & 1) * G16Q * GRAN + (size_t)(4 * lhi) * GRAN + GRAN_C + lcol;
        const unsigned c_epoch = (unsigned)t & 0xFFFFu;
        bool have = t == 0;
        int tk[16];                                         // RT = 1: the 16 tokens, uniform
#pragma unroll
        for (int r = 0; r < 16; ++r) tk[r] = 0;
        int rowtok[RT];                                     // RT = 2: lane l holds the token of row l & 15
#pragma unroll
        for (int k = 0; k < RT; ++k) rowtok[k] = 0;
        u64_t gv[RT][4];
#pragma unroll
        for (int k = 0; k < RT; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) gv[k][i] = 0;
        auto issue = [&]() {
#pragma unroll
            for (int k = 0; k < RT; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) gv[k][i] = load_granule(cand_src + (size_t)i * GRAN + 16 * k);
        };
        auto check = [&]() {
            bool ok = true;
#pragma unroll
            for (int k = 0; k < RT; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) ok = ok && (unsigned)(gv[k][i] >> 48) == c_epoch;
            if (!__all(ok)) return;
#pragma unroll
            for (int k = 0; k < RT; ++k) {
                u64_t best = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    best = umax64(best, am_key(__uint_as_float((unsigned)gv[k][i]), (int)((unsigned)(gv[k][i] >> 32) & 0xFFFFu)));
                best = umax64(best, (u64_t)__shfl_xor((unsigned long long)best, 16));
                best = umax64(best, (u64_t)__shfl_xor((unsigned long long)best, 32));
                const int bi = am_idx(best);                // every lane: the token of row l & 15
                if constexpr (RT == 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tk[r] = __builtin_amdgcn_readlane(bi, r);
                        tk[r] = tk[r] < V ? tk[r] : 0;
                    }
                }
                rowtok[k] = bi < V ? bi : 0;
                if (live[k]) {
                    mytok[k] = __shfl(bi, cell_row);
                    mytok[k] = mytok[k] < V ? mytok[k] : 0;
                    pvec[k] = *reinterpret_cast<const float4*>(w.P + (size_t)mytok[k] * G + 4 * unit);
                    // RT = 2: the image-side gate row travels with it (the same L2 round trip) instead of holding four more
                    // registers per tile through the whole step
                    if constexpr (RT == 2) genc[k] = *reinterpret_cast<const float4*>(tl[k].Genc + (size_t)min(row0 + cell_row, tl[k].B - 1) * G + 4 * unit);
                }
            }
            have = true;
        };
        if (t > 0 && any_live) issue();
#pragma unroll
        for (int k = 0; k < RT; ++k) {
            if (live[k] && (t > 0 || (RT == 2 && tl[k].t0 > 0))) {
                const u32x4_t* hq = reinterpret_cast<const u32x4_t*>(hp + (size_t)(RT == 1 ? ((t - 1) & 1) : k) * 3 * G16_HP_PIECE) + lhi * 16 + lcol;
                Frag16 fa[2][3];                            // A fragments (rows l & 15, k = 32 ks + 8 (l >> 4) .. +7), one k-step ahead
#pragma unroll
                for (int c = 0; c < 3; ++c) fa[0][c].q = hq[(c * 32) * 16];
#pragma unroll
                for (int ks = 0; ks < 8; ++ks) {
                    if (ks + 1 < 8) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) fa[(ks + 1) & 1][c].q = hq[(c * 32 + 4 * (ks + 1)) * 16];
                    }
                    // (RT = 2: in the LAST tile's product, so that the rows fetched for the tokens are not live through the other's)
                    if (ks == 6 && (RT == 1 || (!have && (k == RT - 1 || !live[RT - 1])))) { check(); if (!have) issue(); }
                    __builtin_amdgcn_sched_barrier(0);
                    const bf16x8_t a0 = fa[ks & 1][0].v, a1 = fa[ks & 1][1].v, a2 = fa[ks & 1][2].v;
                    acc[k][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wg[ks * 3 + 0], acc[k][0], 0, 0, 0);
                    acc[k][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wg[ks * 3 + 1], acc[k][1], 0, 0, 0);
                    acc[k][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wg[ks * 3 + 0], acc[k][1], 0, 0, 0);
                    acc[k][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wg[ks * 3 + 2], acc[k][2], 0, 0, 0);
                    acc[k][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wg[ks * 3 + 1], acc[k][2], 0, 0, 0);
                    acc[k][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, wg[ks * 3 + 0], acc[k][2], 0, 0, 0);
                }
                if constexpr (RT == 2) {                    // small terms first, as phase C of RT = 1 sums them
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[k][0][i] = (acc[k][2][i] + acc[k][1][i]) + acc[k][0][i];
                }
            }
        }
        if (t > 0 && any_live && !have) check();
        I2L_STAMP16(0);
        // ---- B. wait for the tokens if they are not there yet (uniform exit on a time-out: see decode_group_kernel)
        bool bail = false;
        if (!have) {
            long long t_start = 0;
            unsigned spins = 0;
            for (;;) {
                issue();
                check();
                if (have) break;
                __builtin_amdgcn_s_sleep(1);
                if ((++spins & 255u) == 0) {
                    const long long now = (long long)wall_clock64();
                    if (t_start == 0) t_start = now;
                    else if (now - t_start > p.opts.limit_step) { bail = true; break; }
                }
            }
            if (bail) cnt_s[2] = 1;
        }
        if (t > 0 && !bail) {
            bool all_fin = true;
#pragma unroll
            for (int k = 0; k < RT; ++k) {
                if constexpr (RT == 1) {
#pragma unroll
                    for (int r = 0; r < G16Q; ++r) {
                        const bool was_fin = (fin[k] >> r) & 1u;
                        if (r == m && tid == 0 && ids_row[k]) ids_row[k][t - 1] = (p.stop == I2L_STOP_STICKY && was_fin) ? -1 : tk[r];
                        if (tk[r] == p.end_id) fin[k] |= 1u << r;
                        all_fin = all_fin && ((fin[k] >> r) & 1u);
                    }
                } else {
                    if (t > nk[k]) continue;                // that tile's steps ended earlier
                    const int tok_m = __builtin_amdgcn_readlane(rowtok[k], m);     // no sticky stop here: every step is written
                    if (tid == 0 && ids_row[k]) ids_row[k][tl[k].t0 + t - 1] = tok_m;
                    fin[k] |= (unsigned)__ballot(lane < G16Q && rowtok[k] == p.end_id);
                    if (t == nk[k] && tl[k].state_out) {    // the batch goes on in a later launch: what that one starts from
                        const G16State st = group16_state(tl[k].state_out, tl[k].B);
                        st.c[(size_t)(row0 + cell_row) * 256 + unit] = c_own[k];
                        st.h[(size_t)(row0 + cell_row) * 256 + unit] = h_own[k];
                        if (m == 0 && wave == 0 && lane < G16Q) st.tok[row0 + lane] = rowtok[k];
                        if (m == 0 && tid == 0) st.fin[group] = fin[k];
                    }
                }
            }
            if (RT == 1 ? (t == tl[0].T || (p.stop == I2L_STOP_STICKY && all_fin)) : t == n_steps) break;
        }
        I2L_STAMP16(1);
        if constexpr (RT == 2) __syncthreads();             // barrier 1: every wave has read h(t-1) (phases E, A): hp may be rewritten
        if constexpr (RT == 2) {
            // W_out^T fragments of this step: 12 coalesced 16-byte loads from the L2-resident image, in flight across phases C
            // and D, used in E (the offset is made opaque so that the loads stay inside the loop)
            unsigned wl_off = (unsigned)(((m * 4 + wave) * 36 * 64 + lane) * sizeof(u32x4_t));
            asm volatile("" : "+v"(wl_off));
            const u32x4_t* pk = reinterpret_cast<const u32x4_t*>(static_cast<const char*>(w.wpack16) + wl_off);
#pragma unroll
            for (int i = 0; i < 12; ++i) { Frag16 f; f.q = pk[(24 + i) * 64]; wl[i] = f.v; }
        }
        // ---- C. 4 x 4 transposition inside lane quads, cell, publish h(t) as its three bf16 pieces
        const unsigned epoch = ((unsigned)t + 1u) & 0xFFFFu;
        const int par = t & 1;
        u64_t* slot = xg + (size_t)par * G16Q * GRAN;
        unsigned short* hcur = hp + (size_t)(RT == 1 ? par : 0) * 3 * G16_HP_PIECE;
        if (!bail) {
#pragma unroll
            for (int k = 0; k < RT; ++k) {
                if (RT == 1 || live[k]) {
                    const bool b0 = lq & 1, b1 = lq & 2;
                    // D registers: z[i] = gate (l & 3) of unit uq, row 4 (l >> 4) + i.  small terms first
                    float z[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) z[i] = RT == 1 ? (acc[k][2][i] + acc[k][1][i]) + acc[k][0][i] : acc[k][0][i];
                    // stage 1 (lane ^ 1): even lanes send z[1], z[3]; odd lanes send z[0], z[2]
                    const float r0 = dpp_f<DPP_XOR1>(b0 ? z[0] : z[1]), r1 = dpp_f<DPP_XOR1>(b0 ? z[2] : z[3]);
                    const float e0 = b0 ? r0 : z[0], e1 = b0 ? z[1] : r0, e2 = b0 ? r1 : z[2], e3 = b0 ? z[3] : r1;
                    // stage 2 (lane ^ 2): lanes 0, 1 send e2, e3; lanes 2, 3 send e0, e1
                    const float s0 = dpp_f<DPP_XOR2>(b1 ? e0 : e2), s1 = dpp_f<DPP_XOR2>(b1 ? e1 : e3);
                    const float gi = b1 ? s0 : e0, gf = b1 ? s1 : e1, gc = b1 ? e2 : s0, go = b1 ? e3 : s1;   // gates of (unit, row cell_row)
                    const float xi = (gi + genc[k].x) + pvec[k].x, xf = (gf + genc[k].y) + pvec[k].y;
                    const float xc = (gc + genc[k].z) + pvec[k].z, xo = (go + genc[k].w) + pvec[k].w;
                    const float ig = sigmoidf_(xi), fg = sigmoidf_(xf), gg = tanhf_(xc), og = sigmoidf_(xo);
                    c_own[k] = fg * c_own[k] + ig * gg;
                    h_own[k] = og * tanhf_(c_own[k]);
                }
                unsigned short q0, q1, q2;                  // (a tile past its steps publishes its last h again: tags only)
                split3(h_own[k], q0, q1, q2);
                const int ul = 4 * wave + uq;               // unit inside the member: k block ul >> 3, element ul & 7
                const u64_t gran = ((u64_t)epoch << 48) | ((u64_t)q0 << 32) | ((u64_t)q1 << 16) | (u64_t)q2;
                store_granule(slot + (size_t)m * GRAN + 256 * k + ((ul >> 3) * 16 + cell_row) * 8 + (ul & 7), gran, local);
                const int o = ((2 * m + (ul >> 3)) * 16 + cell_row) * 8 + (ul & 7);
                unsigned short* hk = hcur + (size_t)k * 3 * G16_HP_PIECE;
                hk[o] = q0;
                hk[G16_HP_PIECE + o] = q1;
                hk[2 * G16_HP_PIECE + o] = q2;
            }
        }
        I2L_STAMP16(2);
        // ---- D. the other fifteen sixteenths of h(t): task = (tile, peer, k block, row) = 8 granules = 64 bytes; a thread's
        //         tasks (tid, tid + 256, ... < 480 RT) are polled TWO AT A TIME
        if (!bail) {
            constexpr int NTASK = 15 * 32 * RT;
#pragma unroll
            for (int pi = 0; pi < RT; ++pi) {
                const int ja = tid + 2 * G16NT * pi, jb = ja + G16NT < NTASK ? ja + G16NT : ja;   // the last threads: one task (twice)
                const int ka = RT == 2 && ja >= 480 ? 1 : 0, kb = RT == 2 && jb >= 480 ? 1 : 0;
                const int ta = ja - 480 * ka, tb = jb - 480 * kb;
                const int qa_ = ta >> 5, qa = qa_ + (qa_ >= m ? 1 : 0), qb_ = tb >> 5, qb = qb_ + (qb_ >= m ? 1 : 0);
                const u64_t* sa = slot + (size_t)qa * GRAN + 256 * ka + (((ta >> 4) & 1) * 16 + (ta & 15)) * 8;
                const u64_t* sb = slot + (size_t)qb * GRAN + 256 * kb + (((tb >> 4) & 1) * 16 + (tb & 15)) * 8;
                u32x4_t g[8];
                long long t_start = 0;
                unsigned spins = 0;
                for (;;) {
                    if constexpr (RT == 1) load_run64x2(sa, sb, g);
                    else load_run64x2_at(slot, (unsigned)((sa - slot) * sizeof(u64_t)), (unsigned)((sb - slot) * sizeof(u64_t)), g);
                    bool ok = true;
#pragma unroll
                    for (int i = 0; i < 8; ++i) ok = ok && (g[i].y >> 16) == epoch && (g[i].w >> 16) == epoch;
                    if (ok) break;
                    __builtin_amdgcn_s_sleep(1);
                    if ((++spins & 255u) == 0) {
                        const long long now = (long long)wall_clock64();
                        if (t_start == 0) t_start = now;
                        else if (now - t_start > p.opts.limit_step) { cnt_s[2] = 1; break; }
                    }
                }
                u32x4_t* ha = reinterpret_cast<u32x4_t*>(hcur + (size_t)ka * 3 * G16_HP_PIECE);
                u32x4_t* hb = reinterpret_cast<u32x4_t*>(hcur + (size_t)kb * 3 * G16_HP_PIECE);
                unpack_run(g, ha + (2 * qa + ((ta >> 4) & 1)) * 16 + (ta & 15));
                unpack_run(g + 4, hb + (2 * qb + ((tb >> 4) & 1)) * 16 + (tb & 15));
                if (RT == 2 && cnt_s[2] != 0) break;        // a poll ran out: the step fails at the barrier, poll no further
            }
        }
        I2L_STAMP16(3);
        __syncthreads();                                    // THE barrier of the step (RT = 2: barrier 2): h(t) complete in hcur
        if (cnt_s[2] != 0) { failed = true; break; }
        I2L_STAMP16(4);

        // ---- E. logits(t): each wave one column tile over half of k; waves 2, 3 pass their partial sums to waves 0, 1
        {
            auto logits_part = [&](int k) {
                f32x4_t la[3] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
                if (RT == 1 || live[k]) {
                    const u32x4_t* hq = reinterpret_cast<const u32x4_t*>(hcur + (size_t)k * 3 * G16_HP_PIECE) + lhi * 16 + lcol;
                    // RT = 1: all four k-steps' fragments requested at once (12 reads in flight); RT = 2: two k-steps ahead (the
                    // second tile's state lives in the registers the deeper prefetch would take)
                    constexpr int PF = RT == 1 ? 4 : 2;
                    Frag16 fa[4][3];
#pragma unroll
                    for (int ks = 0; ks < PF; ++ks)
#pragma unroll
                        for (int c = 0; c < 3; ++c) fa[ks][c].q = hq[(c * 32 + 4 * (4 * lhalf + ks)) * 16];
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) {
                        const bf16x8_t a0 = fa[ks][0].v, a1 = fa[ks][1].v, a2 = fa[ks][2].v;
                        if (ks + PF < 4) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) fa[ks + PF][c].q = hq[(c * 32 + 4 * (4 * lhalf + ks + PF)) * 16];
                        }
                        if constexpr (RT == 2) __builtin_amdgcn_sched_barrier(0);   // (keeps the reads of later k-steps and of the next tile behind these MFMAs)
                        la[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wl[ks * 3 + 0], la[0], 0, 0, 0);
                        la[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wl[ks * 3 + 1], la[1], 0, 0, 0);
                        la[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wl[ks * 3 + 0], la[1], 0, 0, 0);
                        la[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wl[ks * 3 + 2], la[2], 0, 0, 0);
                        la[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wl[ks * 3 + 1], la[2], 0, 0, 0);
                        la[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, wl[ks * 3 + 0], la[2], 0, 0, 0);
                    }
                }
                f32x4_t part;
#pragma unroll
                for (int i = 0; i < 4; ++i) part[i] = (la[2][i] + la[1][i]) + la[0][i];
                return part;
            };
            // what cnt_s[4 + ltile] / cnt_s[6 + ltile] say once tile k's partial sums are written / have been read
            auto flag_of = [&](int k) { return RT == 1 ? (int)epoch : (int)((epoch << 1) | (unsigned)k); };
            f32x4_t part[RT];
            part[0] = logits_part(0);
            if (lhalf == 1) {                               // waves 2, 3: LDS write, then the flag (LDS keeps a wave's order)
#pragma unroll
                for (int k = 0; k < RT; ++k) {
                    if (k > 0) {                            // lpart still holds the tile before: until waves 0, 1 have read it
                        part[k] = logits_part(k);
                        while (__hip_atomic_load(cnt_s + 6 + ltile, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != flag_of(k - 1))
                            __builtin_amdgcn_s_sleep(0);
                    }
                    lpart[ltile * 64 + lane] = part[k];
                    if (lane == 0) __hip_atomic_store(cnt_s + 4 + ltile, flag_of(k), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                I2L_STAMP16(5);
            } else {                                        // waves 0, 1: the other half, bias, arg max, candidates (exchange 2)
#pragma unroll
                for (int k = 1; k < RT; ++k) part[k] = logits_part(k);
#pragma unroll
                for (int k = 0; k < RT; ++k) {
                    while (__hip_atomic_load(cnt_s + 4 + ltile, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != flag_of(k))
                        __builtin_amdgcn_s_sleep(0);
                    const f32x4_t other = lpart[ltile * 64 + lane];
                    if (k + 1 < RT) {                       // read (the release waits for it): waves 2, 3 may write the next tile's
                        if (lane == 0) __hip_atomic_store(cnt_s + 6 + ltile, flag_of(k), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    if (k == RT - 1) I2L_STAMP16(5);
                    const int l_v = 32 * m + 16 * ltile + lcol; // this lane's vocabulary column; register i = row 4 (l >> 4) + i
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float lv = (part[k][i] + other[i]) + l_bias;
                        if (p.use_temp) lv = lv / p.temperature;
                        // arg max over the 16 lanes (= columns) of a row in 32-bit steps: the value's order-preserving integer image
                        // (am_key's high word) by DPP max, then the FIRST lane that holds it (lowest column wins a tie, as am_key)
                        unsigned vk = __float_as_uint(lv + 0.0f);
                        vk ^= (vk >> 31) ? 0xFFFFFFFFu : 0x80000000u;
                        unsigned mx = vk;
                        mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_ROR8, 0xF, 0xF, true));
                        mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_ROR4, 0xF, 0xF, true));
                        mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_XOR2, 0xF, 0xF, true));
                        mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_XOR1, 0xF, 0xF, true));
                        const unsigned long long hit = __ballot(vk == mx);
                        const int first = __ffs((unsigned)(hit >> (16 * lhi)) & 0xFFFFu) - 1;
                        const u64_t key = ((u64_t)mx << 32) | (u64_t)(0xFFFFFFFFu - (unsigned)(l_v - lcol + first));
                        if (lcol == 0)
                            atomicMax(reinterpret_cast<unsigned long long*>(redk + (par * RT + k) * 16 + 4 * lhi + i), (unsigned long long)key);
                    }
                }
                int arrived = 0;
                if (lane == 0) arrived = atomicAdd(cnt_s + par, 1);
                arrived = __builtin_amdgcn_readfirstlane(arrived);
                if (arrived == 1) {                         // the later of the two publishes
                    if (lane < 16 * RT) {                   // lane = [tile][row]
                        const u64_t best = redk[par * RT * 16 + lane];
                        store_granule(slot + (size_t)m * GRAN + GRAN_C + lane,
                                      granule((epoch << 16) | (unsigned)(am_idx(best) & 0xFFFF), am_val(best)), local);
                        redk[(par ^ 1) * RT * 16 + lane] = 0;
                    }
                    if (lane == 0) cnt_s[par ^ 1] = 0;
                }
                I2L_STAMP16(6);
            }
        }
    }
#ifdef I2L_GROUP_STAMPS
    if (lane == 0 && (wave & 1) == 0 && blockIdx.x < 16)
        for (int i = 0; i < 8; ++i) p.status[8 + blockIdx.x * 16 + (wave >> 1) * 8 + i] = (unsigned)st_acc[i];
#endif
#undef I2L_STAMP16
    if (failed) {
        if (lane == 0) atomicOr(p.status, 1u);
#pragma unroll
        for (int k = 0; k < RT; ++k) {
            if (ids_row[k]) for (int tt = tid; tt < tl[k].T; tt += G16NT) ids_row[k][tt] = -3;
            if constexpr (RT == 2) {
                if (nk[k] > 0 && tl[k].state_out && tid == 0) atomicOr(group16_state(tl[k].state_out, tl[k].B).failed + group, 1u);
            }
        }
        return;
    }
    if constexpr (RT == 1) {
        if (ids_row[0]) for (int tt = t + tid; tt < tl[0].T; tt += G16NT) ids_row[0][tt] = -1;
    } else {
#pragma unroll
        for (int k = 0; k < RT; ++k) {                      // the launch of its earlier steps failed: the host decodes the batch again
            if (!mark_failed[k] || row0 + m >= tl[k].B || !tl[k].ids) continue;
            int32_t* row = tl[k].ids + (size_t)(row0 + m) * tl[k].T;
            for (int tt = tid; tt < tl[k].T; tt += G16NT) row[tt] = -3;
        }
    }
}

// RT = 1 is kept as its own text, the kernel as it was before the row tiles: the template above, instantiated at RT = 1,
// describes the same program, but the compiler does not allocate it the same registers (255 + 8 spilled against 254 and
// none), and the one-batch launch must not move.  A change to a phase belongs in both.
constexpr int G16GRAN_H = G16Shape<1>::GRAN_H, G16GRAN_C = G16Shape<1>::GRAN_C, G16GRAN_X = G16Shape<1>::GRAN_X,
              G16GRAN = G16Shape<1>::GRAN;
template <>
__global__ __launch_bounds__(G16NT, 2) void decode_group16_kernel<1>(GroupParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem16[];
    unsigned short* hp = reinterpret_cast<unsigned short*>(smem16);                    // [2][3][32][16][8]
    f32x4_t* lpart = reinterpret_cast<f32x4_t*>(smem16 + (size_t)2 * 3 * G16_HP_PIECE * 2);   // [2 tiles][64 lanes]
    u64_t* redk = reinterpret_cast<u64_t*>(lpart + 2 * 64);                           // [2][16 rows]
    int* cnt_s = reinterpret_cast<int*>(redk + 2 * 16);      // [0..1] logit waves arrived (by parity), [2] time-out, [3] one XCD,
                                                             // [4..5] epoch of the partial logits of tile 0 / 1 in lpart
    const StepWeights& w = p.w;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int within = blockIdx.x & 127;
    const int group = (blockIdx.x >> 7) * 8 + (within & 7), m = within >> 3;      // a group's members: block ids 8 apart = one XCD
    if (group >= p.n_groups) return;
    const int B = p.B, T = p.T, V = w.V;
    const int row0 = group * G16Q;
    constexpr int G = 1024;
    const int lq = lane & 3, uq = (lane >> 2) & 3, lhi = lane >> 4, lcol = lane & 15;
    const int cell_row = 4 * lhi + lq;                       // the row of this lane's cell (after the quad transposition)
    const int unit = 16 * m + 4 * wave + uq;                 // ... and its hidden unit
    const int ltile = wave & 1, lhalf = wave >> 1;           // logits: column tile, half of the reduction

    // ---- placement exchange FIRST (r04): a member reports itself before it loads its 147 KB of weights, so that the launch's
    // residency word (count_resident_group) -- which the next batch's encoder stream is waiting for -- is published ~10 us
    // earlier; waves 1-3 start their weight loads meanwhile
    u64_t* xg = p.xchg + (size_t)group * 2 * G16Q * G16GRAN;
    if (tid < 8) cnt_s[tid] = 0;                             // wave 0: in program order before its writes below
    if (wave == 0) {                                        // placement: are the sixteen members on one XCD?
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xFu;
        if (lane == 0 && !(p.opts.drop_member && m == 3))
            store_granule(xg + (size_t)m * G16GRAN + G16GRAN_X, granule(0xC0DEu, __uint_as_float(xcc)), false);
        const int pq = (lane & 15) + ((lane & 15) >= m ? 1 : 0);
        u64_t pv = 0;
        bool bad = false;
        long long t_start = 0;
        unsigned spins = 0;
        for (;;) {
            bool ok = true;
            if (lane < 15) { pv = load_granule(xg + (size_t)pq * G16GRAN + G16GRAN_X); ok = (unsigned)(pv >> 32) == 0xC0DEu; }
            if (__all(ok)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 255u) == 0) {
                const long long now = (long long)wall_clock64();
                if (t_start == 0) t_start = now;
                else if (now - t_start > p.opts.limit_first) { bad = true; break; }
            }
        }
        const bool all_same = __all(lane >= 15 || (unsigned)pv == xcc);
        if (lane == 0) {
            cnt_s[3] = (all_same && !bad) ? 1 : 0;
            if (bad) cnt_s[2] = 1;
            if (m == 0 && !bad) {
                count_resident_group(p.status, p.n_groups, p.resident_flag, p.resident_value);
                if (all_same && !p.opts.agent_scope) atomicAdd(p.status + GRP_STAT_LOCAL, 1u);
            }
        }
    }
    // ---- the member's weights, pre-split in B-operand layout by pack16_kernel: 36 coalesced 16-byte loads per lane
    bf16x8_t wg[24], wl[12];                                 // [k-step][piece]
    {
        const u32x4_t* pk = static_cast<const u32x4_t*>(w.wpack16) + (size_t)(m * 4 + wave) * 36 * 64 + lane;
#pragma unroll
        for (int i = 0; i < 24; ++i) { Frag16 f; f.q = pk[i * 64]; wg[i] = f.v; }
#pragma unroll
        for (int i = 0; i < 12; ++i) { Frag16 f; f.q = pk[(24 + i) * 64]; wl[i] = f.v; }
    }
    for (int idx = tid; idx < 2 * 3 * G16_HP_PIECE / 2; idx += G16NT) reinterpret_cast<unsigned*>(hp)[idx] = 0u;   // h(-1) = 0
    if (tid < 32) redk[tid] = 0;
    const float4 genc = *reinterpret_cast<const float4*>(w.Genc + (size_t)min(row0 + cell_row, B - 1) * G + 4 * unit);
    const float l_bias = w.boutP[32 * m + 16 * ltile + lcol];
    float c_own = 0.f, h_own = 0.f;
    unsigned fin = 0;
#pragma unroll
    for (int r = 0; r < G16Q; ++r)
        if (row0 + r >= B) fin |= 1u << r;
    const bool own_row = row0 + m < B;
    int32_t* ids_row = (p.ids && own_row) ? p.ids + (size_t)(row0 + m) * T : nullptr;

    __syncthreads();
    const bool local = cnt_s[3] != 0 && !p.opts.agent_scope;

    int mytok = min(max(p.tok0[min(row0 + cell_row, B - 1)], 0), V - 1);
    float4 pvec = *reinterpret_cast<const float4*>(w.P + (size_t)mytok * G + 4 * unit);

    int t = 0;
    bool failed = cnt_s[2] != 0;
#ifdef I2L_GROUP_STAMPS
    long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long st_last = (long long)wall_clock64();
#define I2L_STAMP16(i) do { const long long n_ = (long long)wall_clock64(); st_acc[i] += n_ - st_last; st_last = n_; } while (0)
#else
#define I2L_STAMP16(i) do { } while (0)
#endif
    for (; !failed; ++t) {
        // ---- A. gates(t) = h(t-1) . WhhT on the matrix cores; on the way every wave polls the 256 candidate granules of
        //         step t-1 -- lane (row l & 15, members 4 (l >> 4) .. +3) -- and merges them into the 16 tokens
        f32x4_t acc[3];                                     // hi | mid | lo partial products
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const u64_t* cand_src = xg + (size_t)((t - 1) & 1) * G16Q * G16GRAN + (size_t)(4 * lhi) * G16GRAN + G16GRAN_C + lcol;
        const unsigned c_epoch = (unsigned)t & 0xFFFFu;
        bool have = t == 0;
        int tk[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) tk[r] = 0;
        u64_t gv[4] = {0, 0, 0, 0};
        auto issue = [&]() {
#pragma unroll
            for (int i = 0; i < 4; ++i) gv[i] = load_granule(cand_src + (size_t)i * G16GRAN);
        };
        auto check = [&]() {
            bool ok = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) ok = ok && (unsigned)(gv[i] >> 48) == c_epoch;
            if (!__all(ok)) return;
            u64_t best = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                best = umax64(best, am_key(__uint_as_float((unsigned)gv[i]), (int)((unsigned)(gv[i] >> 32) & 0xFFFFu)));
            best = umax64(best, (u64_t)__shfl_xor((unsigned long long)best, 16));
            best = umax64(best, (u64_t)__shfl_xor((unsigned long long)best, 32));
            const int bi = am_idx(best);                    // every lane: the token of row l & 15
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                tk[r] = __builtin_amdgcn_readlane(bi, r);
                tk[r] = tk[r] < V ? tk[r] : 0;
            }
            have = true;
            if (t < T) {
                mytok = __shfl(bi, cell_row);
                mytok = mytok < V ? mytok : 0;
                pvec = *reinterpret_cast<const float4*>(w.P + (size_t)mytok * G + 4 * unit);
            }
        };
        if (t > 0 && t < T) {
            const u32x4_t* hq = reinterpret_cast<const u32x4_t*>(hp + (size_t)((t - 1) & 1) * 3 * G16_HP_PIECE) + lhi * 16 + lcol;
            issue();
            Frag16 fa[2][3];                                // A fragments (rows l & 15, k = 32 ks + 8 (l >> 4) .. +7), one k-step ahead
#pragma unroll
            for (int c = 0; c < 3; ++c) fa[0][c].q = hq[(c * 32) * 16];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                if (ks + 1 < 8) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) fa[(ks + 1) & 1][c].q = hq[(c * 32 + 4 * (ks + 1)) * 16];
                }
                if (ks == 6) { check(); if (!have) issue(); }
                __builtin_amdgcn_sched_barrier(0);
                const bf16x8_t a0 = fa[ks & 1][0].v, a1 = fa[ks & 1][1].v, a2 = fa[ks & 1][2].v;
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wg[ks * 3 + 0], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wg[ks * 3 + 1], acc[1], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wg[ks * 3 + 0], acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wg[ks * 3 + 2], acc[2], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wg[ks * 3 + 1], acc[2], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, wg[ks * 3 + 0], acc[2], 0, 0, 0);
            }
            if (!have) check();
        }
        I2L_STAMP16(0);
        // ---- B. wait for the tokens if they are not there yet (uniform exit on a time-out: see decode_group_kernel)
        bool bail = false;
        if (!have) {
            long long t_start = 0;
            unsigned spins = 0;
            for (;;) {
                issue();
                check();
                if (have) break;
                __builtin_amdgcn_s_sleep(1);
                if ((++spins & 255u) == 0) {
                    const long long now = (long long)wall_clock64();
                    if (t_start == 0) t_start = now;
                    else if (now - t_start > p.opts.limit_step) { bail = true; break; }
                }
            }
            if (bail) cnt_s[2] = 1;
        }
        if (t > 0 && !bail) {
            bool all_fin = true;
#pragma unroll
            for (int r = 0; r < G16Q; ++r) {
                const bool was_fin = (fin >> r) & 1u;
                if (r == m && tid == 0 && ids_row) ids_row[t - 1] = (p.stop == I2L_STOP_STICKY && was_fin) ? -1 : tk[r];
                if (tk[r] == p.end_id) fin |= 1u << r;
                all_fin = all_fin && ((fin >> r) & 1u);
            }
            if (t == T || (p.stop == I2L_STOP_STICKY && all_fin)) break;
        }
        I2L_STAMP16(1);
        // ---- C. 4 x 4 transposition inside lane quads, cell, publish h(t) as its three bf16 pieces
        const unsigned epoch = ((unsigned)t + 1u) & 0xFFFFu;
        const int par = t & 1;
        u64_t* slot = xg + (size_t)par * G16Q * G16GRAN;
        unsigned short* hcur = hp + (size_t)par * 3 * G16_HP_PIECE;
        if (!bail) {
            const bool b0 = lq & 1, b1 = lq & 2;
            // D registers: z[i] = gate (l & 3) of unit uq, row 4 (l >> 4) + i.  small terms first
            float z[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = (acc[2][i] + acc[1][i]) + acc[0][i];
            // stage 1 (lane ^ 1): even lanes send z[1], z[3]; odd lanes send z[0], z[2]
            const float r0 = dpp_f<DPP_XOR1>(b0 ? z[0] : z[1]), r1 = dpp_f<DPP_XOR1>(b0 ? z[2] : z[3]);
            const float e0 = b0 ? r0 : z[0], e1 = b0 ? z[1] : r0, e2 = b0 ? r1 : z[2], e3 = b0 ? z[3] : r1;
            // stage 2 (lane ^ 2): lanes 0, 1 send e2, e3; lanes 2, 3 send e0, e1
            const float s0 = dpp_f<DPP_XOR2>(b1 ? e0 : e2), s1 = dpp_f<DPP_XOR2>(b1 ? e1 : e3);
            const float gi = b1 ? s0 : e0, gf = b1 ? s1 : e1, gc = b1 ? e2 : s0, go = b1 ? e3 : s1;   // gates of (unit, row cell_row)
            const float xi = (gi + genc.x) + pvec.x, xf = (gf + genc.y) + pvec.y;
            const float xc = (gc + genc.z) + pvec.z, xo = (go + genc.w) + pvec.w;
            const float ig = sigmoidf_(xi), fg = sigmoidf_(xf), gg = tanhf_(xc), og = sigmoidf_(xo);
            c_own = fg * c_own + ig * gg;
            h_own = og * tanhf_(c_own);
            unsigned short q0, q1, q2;
            split3(h_own, q0, q1, q2);
            const int ul = 4 * wave + uq;                   // unit inside the member: k block ul >> 3, element ul & 7
            const u64_t gran = ((u64_t)epoch << 48) | ((u64_t)q0 << 32) | ((u64_t)q1 << 16) | (u64_t)q2;
            store_granule(slot + (size_t)m * G16GRAN + ((ul >> 3) * 16 + cell_row) * 8 + (ul & 7), gran, local);
            const int o = ((2 * m + (ul >> 3)) * 16 + cell_row) * 8 + (ul & 7);
            hcur[o] = q0;
            hcur[G16_HP_PIECE + o] = q1;
            hcur[2 * G16_HP_PIECE + o] = q2;
        }
        I2L_STAMP16(2);
        // ---- D. the other fifteen sixteenths of h(t): task = (peer, k block, row) = 8 granules = 64 bytes; a thread's two
        //         tasks (tid, tid + 256 < 480) are polled TOGETHER
        if (!bail) {
            const int ta = tid, tb = tid + G16NT < 15 * 32 ? tid + G16NT : tid;         // threads 224 .. 255: one task (twice)
            const int qa_ = ta >> 5, qa = qa_ + (qa_ >= m ? 1 : 0), qb_ = tb >> 5, qb = qb_ + (qb_ >= m ? 1 : 0);
            const u64_t* sa = slot + (size_t)qa * G16GRAN + (((ta >> 4) & 1) * 16 + (ta & 15)) * 8;
            const u64_t* sb = slot + (size_t)qb * G16GRAN + (((tb >> 4) & 1) * 16 + (tb & 15)) * 8;
            u32x4_t g[8];
            long long t_start = 0;
            unsigned spins = 0;
            for (;;) {
                load_run64x2(sa, sb, g);
                bool ok = true;
#pragma unroll
                for (int i = 0; i < 8; ++i) ok = ok && (g[i].y >> 16) == epoch && (g[i].w >> 16) == epoch;
                if (ok) break;
                __builtin_amdgcn_s_sleep(1);
                if ((++spins & 255u) == 0) {
                    const long long now = (long long)wall_clock64();
                    if (t_start == 0) t_start = now;
                    else if (now - t_start > p.opts.limit_step) { cnt_s[2] = 1; break; }
                }
            }
            unpack_run(g, reinterpret_cast<u32x4_t*>(hcur) + (2 * qa + ((ta >> 4) & 1)) * 16 + (ta & 15));
            unpack_run(g + 4, reinterpret_cast<u32x4_t*>(hcur) + (2 * qb + ((tb >> 4) & 1)) * 16 + (tb & 15));
        }
        I2L_STAMP16(3);
        __syncthreads();                                    // THE barrier of the step: h(t) complete in hcur
        if (cnt_s[2] != 0) { failed = true; break; }
        I2L_STAMP16(4);

        // ---- E. logits(t): each wave one column tile over half of k; waves 2, 3 pass their partial sums to waves 0, 1
        {
            f32x4_t la[3] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
            const u32x4_t* hq = reinterpret_cast<const u32x4_t*>(hcur) + lhi * 16 + lcol;
            Frag16 fa[4][3];                                // all four k-steps' fragments requested at once (12 reads in flight)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int c = 0; c < 3; ++c) fa[ks][c].q = hq[(c * 32 + 4 * (4 * lhalf + ks)) * 16];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8_t a0 = fa[ks][0].v, a1 = fa[ks][1].v, a2 = fa[ks][2].v;
                la[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wl[ks * 3 + 0], la[0], 0, 0, 0);
                la[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wl[ks * 3 + 1], la[1], 0, 0, 0);
                la[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wl[ks * 3 + 0], la[1], 0, 0, 0);
                la[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, wl[ks * 3 + 2], la[2], 0, 0, 0);
                la[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, wl[ks * 3 + 1], la[2], 0, 0, 0);
                la[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, wl[ks * 3 + 0], la[2], 0, 0, 0);
            }
            f32x4_t part;
#pragma unroll
            for (int i = 0; i < 4; ++i) part[i] = (la[2][i] + la[1][i]) + la[0][i];
            if (lhalf == 1) {                               // waves 2, 3: LDS write, then the flag (LDS keeps a wave's order)
                lpart[ltile * 64 + lane] = part;
                if (lane == 0) __hip_atomic_store(cnt_s + 4 + ltile, (int)epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                I2L_STAMP16(5);
            } else {                                        // waves 0, 1: the other half, bias, arg max, candidates (exchange 2)
                while (__hip_atomic_load(cnt_s + 4 + ltile, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != (int)epoch)
                    __builtin_amdgcn_s_sleep(0);
                const f32x4_t other = lpart[ltile * 64 + lane];
                I2L_STAMP16(5);
                const int l_v = 32 * m + 16 * ltile + lcol; // this lane's vocabulary column; register i = row 4 (l >> 4) + i
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float lv = (part[i] + other[i]) + l_bias;
                    if (p.use_temp) lv = lv / p.temperature;
                    // arg max over the 16 lanes (= columns) of a row in 32-bit steps: the value's order-preserving integer image
                    // (am_key's high word) by DPP max, then the FIRST lane that holds it (lowest column wins a tie, as am_key)
                    unsigned vk = __float_as_uint(lv + 0.0f);
                    vk ^= (vk >> 31) ? 0xFFFFFFFFu : 0x80000000u;
                    unsigned mx = vk;
                    mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_ROR8, 0xF, 0xF, true));
                    mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_ROR4, 0xF, 0xF, true));
                    mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_XOR2, 0xF, 0xF, true));
                    mx = max(mx, (unsigned)__builtin_amdgcn_mov_dpp((int)mx, DPP_XOR1, 0xF, 0xF, true));
                    const unsigned long long hit = __ballot(vk == mx);
                    const int first = __ffs((unsigned)(hit >> (16 * lhi)) & 0xFFFFu) - 1;
                    const u64_t key = ((u64_t)mx << 32) | (u64_t)(0xFFFFFFFFu - (unsigned)(l_v - lcol + first));
                    if (lcol == 0) atomicMax(reinterpret_cast<unsigned long long*>(redk + par * 16 + 4 * lhi + i), (unsigned long long)key);
                }
                int arrived = 0;
                if (lane == 0) arrived = atomicAdd(cnt_s + par, 1);
                arrived = __builtin_amdgcn_readfirstlane(arrived);
                if (arrived == 1) {                         // the later of the two publishes
                    if (lane < 16) {
                        const u64_t best = redk[par * 16 + lane];
                        store_granule(slot + (size_t)m * G16GRAN + G16GRAN_C + lane,
                                      granule((epoch << 16) | (unsigned)(am_idx(best) & 0xFFFF), am_val(best)), local);
                        redk[(par ^ 1) * 16 + lane] = 0;
                    }
                    if (lane == 0) cnt_s[par ^ 1] = 0;
                }
                I2L_STAMP16(6);
            }
        }
    }
#ifdef I2L_GROUP_STAMPS
    if (lane == 0 && (wave & 1) == 0 && blockIdx.x < 16)
        for (int i = 0; i < 8; ++i) p.status[8 + blockIdx.x * 16 + (wave >> 1) * 8 + i] = (unsigned)st_acc[i];
#endif
#undef I2L_STAMP16
    if (failed) {
        if (lane == 0) atomicOr(p.status, 1u);
        if (ids_row) for (int tt = tid; tt < T; tt += G16NT) ids_row[tt] = -3;
        return;
    }
    if (ids_row) for (int tt = t + tid; tt < T; tt += G16NT) ids_row[tt] = -1;
}
