// Step-batched greedy decode on the MATRIX CORES for decoders the grouped kernels do not take (the shipped 2 x 512 one):
// one decoder step of the whole batch is L + 2 short launches and the launch boundary is the only barrier (included by
// decode.hip inside its anonymous namespace, after decode_group16.inc.h).  Reference decoder.py:247-250,277-280 (LSTM
// gates, Linear(H -> V)), seq2seq.py:210-221 / predictor.py:283-347 (the arg max loop).
//
//   lstm_step_mfma_kernel<TB>   one launch per layer: gates[B x 4H] = (P[tok] + Genc | biasP) + x . WihT + h . WhhT and the
//                               cell in the epilogue.  A workgroup owns TB batch rows x 64 gate columns (16 hidden units,
//                               all four gates) and reads only its own 64-column slab of the weights.
//   logits_mfma_kernel<TB>      logits[B x Vp] = h_top . WoutT + boutP into the scratch, same tiles.
//   select_batched_kernel<Rule> one wave per row (select_row): the row kernel's selection rule under the rule's pick
//                               policy (plain, or decode_constrained.inc.h's), ids, next token, finished rows.
//
// Products are split-bf16 (bf16_split.inc.h): both operands are split into three bf16 pieces while they are staged into
// LDS in the matrix cores' operand layout, six partial products v_mfma_f32_16x16x32_bf16, fp32 accumulation, the small
// terms added first.  The gate columns lie along the MFMA's M and the batch rows along its N: D[m = 4 (l >> 4) + i][n =
// l & 15] gives lane l the four gates (i) of one hidden unit for one row, so the cell needs no cross-lane traffic.
//
// h is double-buffered by step parity (other workgroups of the same launch still read the old h); c is updated in place
// (each element is read and written by one thread).  Under I2L_STOP_STICKY the selection kernel counts the unfinished rows
// in one device word; every kernel of a later step reads it first and returns when it is 0.  No polls, no cooperative
// launch, no exchange: nothing here can time out.

#include "mfma_slab.inc.h"      // DB_* tile constants, DbLds, db_slab, batched_tile_rows

struct BatchedParams {
    StepWeights w;
    int B, T;
    int genc_div;        // row r reads Genc row r / genc_div: 1, the beam width (beam_batched.inc.h: K rows per image) or
                         // the samples of an image (i2l_sample_decode_multi), which then share tok0[r / genc_div] too
    const int32_t* forced;
    float* h;            // [2][L][B][H]
    float* c;            // [L][B][H]
    float* lg;           // [B][Vp] logits of the current step
    int* tok;            // [B] token selected by the previous step
    int* fin;            // [B] row has produced END
    unsigned* live;      // rows not finished (only I2L_STOP_STICKY counts it down)
    int32_t* ids;
    float* logits_out;
    float temperature;
    int use_temp, select, stop, end_id;
};

// Layer `layer` of step t for the whole batch.  grid (H / 16, cdiv(B, TB)).
template <int TB>
__global__ __launch_bounds__(DB_NT) void lstm_step_mfma_kernel(BatchedParams p, int layer, int t) {
    __shared__ u32x4_t ws[DbLds<TB>::WS];
    __shared__ u32x4_t xs[DbLds<TB>::XS];
    if (*p.live == 0) return;
    const StepWeights& w = p.w;
    const int H = w.H, L = w.L, B = p.B, par = t & 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col0 = blockIdx.x * DB_COLS, row0 = blockIdx.y * TB;
    const size_t G = 4 * (size_t)H, LBH = (size_t)L * B * H;
    f32x4_t acc[TB / 16][3];
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[nt][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const float* h_old = p.h + (size_t)par * LBH + (size_t)layer * B * H;
    float* h_new = p.h + (size_t)(par ^ 1) * LBH + (size_t)layer * B * H;
    if (layer > 0)      // the layer below, already at step t
        db_slab<TB>(acc, w.WihT[layer], G, col0, p.h + (size_t)(par ^ 1) * LBH + (size_t)(layer - 1) * B * H, H, row0, B, H,
                    ws, xs, tid);
    db_slab<TB>(acc, w.WhhT[layer], G, col0, h_old, H, row0, B, H, ws, xs, tid);

    const int unit = (col0 >> 2) + 4 * wave + (lane >> 4);       // this lane's D rows are the gates i, f, g, o of `unit`
    float* c_l = p.c + (size_t)layer * B * H;
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt) {
        const int row = row0 + 16 * nt + (lane & 15);
        if (row >= B) continue;
        float4 add;
        if (layer == 0) {
            int tk = p.forced ? p.forced[(size_t)row * p.T + t] : p.tok[row];
            tk = min(max(tk, 0), w.V - 1);
            const float4 a = *reinterpret_cast<const float4*>(w.P + (size_t)tk * G + 4 * unit);
            const float4 e = *reinterpret_cast<const float4*>(w.Genc + (size_t)(row / p.genc_div) * G + 4 * unit);
            add = make_float4(a.x + e.x, a.y + e.y, a.z + e.z, a.w + e.w);
        } else {
            add = *reinterpret_cast<const float4*>(w.biasP[layer] + 4 * unit);
        }
        const f32x4_t z = db_fold(acc[nt]);
        const float ig = sigmoidf_(z[0] + add.x), fg = sigmoidf_(z[1] + add.y);
        const float gg = tanhf_(z[2] + add.z), og = sigmoidf_(z[3] + add.w);
        const size_t ci = (size_t)row * H + unit;
        const float cn = fg * c_l[ci] + ig * gg;
        c_l[ci] = cn;
        h_new[ci] = og * tanhf_(cn);
    }
}

// logits of step t (after its LSTM launches): lg[b][v] = boutP[v] + sum_k h_top[b][k] WoutT[k][v].  grid (Vp / 64, cdiv(B, TB)).
template <int TB>
__global__ __launch_bounds__(DB_NT) void logits_mfma_kernel(BatchedParams p, int t) {
    __shared__ u32x4_t ws[DbLds<TB>::WS];
    __shared__ u32x4_t xs[DbLds<TB>::XS];
    if (*p.live == 0) return;
    const StepWeights& w = p.w;
    const int H = w.H, L = w.L, B = p.B, par = t & 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col0 = blockIdx.x * DB_COLS, row0 = blockIdx.y * TB;
    f32x4_t acc[TB / 16][3];
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[nt][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const float* h_top = p.h + ((size_t)(par ^ 1) * L + (L - 1)) * B * H;
    db_slab<TB>(acc, w.WoutT, (size_t)w.Vp, col0, h_top, H, row0, B, H, ws, xs, tid);
    const int col = col0 + 16 * wave + 4 * (lane >> 4);
    const float4 bb = *reinterpret_cast<const float4*>(w.boutP + col);   // -inf in the padding columns
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt) {
        const int row = row0 + 16 * nt + (lane & 15);
        if (row >= B) continue;
        const f32x4_t z = db_fold(acc[nt]);
        *reinterpret_cast<float4*>(p.lg + (size_t)row * w.Vp + col) = make_float4(z[0] + bb.x, z[1] + bb.y, z[2] + bb.z, z[3] + bb.w);
    }
}

// The token selected for `row` at step t, by one thread: ids (-1 once the row has finished under the sticky stop), the
// next step's token, the finished mark and the count of unfinished rows.
__device__ __forceinline__ void commit_token_batched(const BatchedParams& p, int row, int t, int sel) {
    const int was_fin = p.fin[row];
    if (p.ids) p.ids[(size_t)row * p.T + t] = (p.stop == I2L_STOP_STICKY && was_fin) ? -1 : sel;
    p.tok[row] = sel;
    if (sel == p.end_id && !was_fin) {
        p.fin[row] = 1;
        if (p.stop == I2L_STOP_STICKY) atomicSub(p.live, 1u);
    }
}

// THE PICK POLICY of the selection kernels (the arg max here, the sampling of sample_batched.inc.h).  A kernel template
// takes a rule as a launch argument -- NoRule, or decode_constrained.inc.h's ConstrainRule or ArgumentRule -- and
// rule.row(...) gives each thread the policy of its row at this step:
//   allows(v, c), operator()(v)   may column v be picked (c = cls(v), its class byte)
//   mask()                        where the row's allowed set is written, or null
//   winner_cls(c, v)              in every lane of the wave: the c of the lane that owns column v (v & 63)
//   finish_argmax, finish_sample  by ONE thread: the token to commit from what the selection returned, and the policy's
//                                 own state, if it keeps any
// AllowAll is the plain model: every column, no class byte, no state.  It must cost nothing -- each member is a constant
// that folds, so a plain instantiation is the kernel as one would write it without a policy, register for register.
struct AllowAll {
    __device__ __forceinline__ uint8_t cls(int) const { return 0; }
    __device__ __forceinline__ bool allows(int, uint8_t) const { return true; }
    __device__ __forceinline__ bool operator()(int) const { return true; }
    __device__ __forceinline__ uint8_t* mask() const { return nullptr; }
    __device__ __forceinline__ int winner_cls(int, int) const { return 0; }
    __device__ __forceinline__ int finish_argmax(int V, int pick, int) const { return pick < V ? pick : 0; }
    __device__ __forceinline__ int finish_sample(int, int pick) const { return pick; }
};
struct NoRule {
    __device__ __forceinline__ AllowAll row(int, int, int, int) const { return {}; }
};

// One row by one wave.  The rule is decode_kernel's ("output projection + token selection" in decode.hip, the first
// copy) over the allowed columns of x[0, V): raw logits out (lo, V floats or null), division by the temperature when it
// is not 1, first-index arg max, and for I2L_SELECT_SOFTMAX the probabilities evaluated literally (exp(x - max) / sum in
// fp32, first index wins).  Every lane returns the arg max and in *pick_cls its class byte -- the winner is the local
// best of the lane that owns its column, which hands the class over, so that nothing is loaded between the selection
// and the commit -- or 0x7fffffff and -1 if no allowed column holds a logit above -inf.
template <class Pick>
__device__ __forceinline__ int select_row(const float* __restrict__ x, int V, float temperature, int use_temp, int select,
                                          const Pick& al, float* __restrict__ lo, int lane, int* pick_cls) {
    uint8_t* mask = al.mask();
    float best = -INFINITY;
    int besti = 0x7fffffff, bestc = 0;
    for (int v = lane; v < V; v += 64) {
        float a = x[v];
        const uint8_t c = al.cls(v);
        const bool ok = al.allows(v, c);
        if (lo) lo[v] = a;
        if (mask) mask[v] = ok ? 1 : 0;
        if (use_temp) a = a / temperature;
        if (ok && a > best) { best = a; besti = v; bestc = c; }
    }
    wave_argmax(best, besti);
    if (select == I2L_SELECT_SOFTMAX && besti < V) {
        float s = 0.f;
        for (int v = lane; v < V; v += 64) {
            const float a = use_temp ? x[v] / temperature : x[v];
            if (al(v)) s += expf(a - best);
        }
        s = wave_sum(s);
        float pbest = -1.f;
        int pbesti = 0x7fffffff;
        for (int v = lane; v < V; v += 64) {
            const float a = use_temp ? x[v] / temperature : x[v];
            const float pr = expf(a - best) / s;
            const uint8_t c = al.cls(v);
            if (al.allows(v, c) && pr > pbest) { pbest = pr; pbesti = v; bestc = c; }
        }
        wave_argmax(pbest, pbesti);
        besti = pbesti;
    }
    const int c = al.winner_cls(bestc, besti);
    *pick_cls = besti < V ? c : -1;
    return besti;
}

// Token selection of step t, one wave per row, under NoRule or ConstrainRule.  grid cdiv(B, DB_NT / 64).
template <class Rule>
__global__ __launch_bounds__(DB_NT) void select_batched_kernel(BatchedParams p, Rule r, int t) {
    if (*p.live == 0) return;
    const int V = p.w.V, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6);
    if (row >= p.B) return;
    const auto al = r.row(row, V, p.end_id, p.T - t - 1);
    float* lo = p.logits_out ? p.logits_out + ((size_t)row * p.T + t) * V : nullptr;
    int pick_cls;
    const int pick = select_row(p.lg + (size_t)row * p.w.Vp, V, p.temperature, p.use_temp, p.select, al, lo, lane, &pick_cls);
    if (lane == 0) commit_token_batched(p, row, t, al.finish_argmax(V, pick, pick_cls));
}

// state in, tokens, finished marks, the live-row count and ids = -1 (steps an early end never runs)
__global__ __launch_bounds__(DB_NT) void init_batched_kernel(BatchedParams p, const int32_t* __restrict__ tok0,
                                                             const float* __restrict__ h0, const float* __restrict__ c0) {
    const size_t LBH = (size_t)p.w.L * p.B * p.w.H, BT = (size_t)p.B * p.T;
    const size_t i0 = (size_t)blockIdx.x * DB_NT + threadIdx.x, stride = (size_t)gridDim.x * DB_NT;
    for (size_t i = i0; i < LBH; i += stride) {
        p.h[i] = h0 ? h0[i] : 0.f;
        p.c[i] = c0 ? c0[i] : 0.f;
    }
    if (p.ids)
        for (size_t i = i0; i < BT; i += stride) p.ids[i] = -1;
    for (size_t i = i0; i < (size_t)p.B; i += stride) { p.tok[i] = tok0[i / p.genc_div]; p.fin[i] = 0; }
    if (i0 == 0) *p.live = (unsigned)p.B;
}

// state after the last step (parity T & 1)
__global__ __launch_bounds__(DB_NT) void state_out_batched_kernel(BatchedParams p, float* __restrict__ h_out,
                                                                  float* __restrict__ c_out) {
    const size_t LBH = (size_t)p.w.L * p.B * p.w.H;
    const float* h = p.h + (size_t)(p.T & 1) * LBH;
    for (size_t i = (size_t)blockIdx.x * DB_NT + threadIdx.x; i < LBH; i += (size_t)gridDim.x * DB_NT) {
        if (h_out) h_out[i] = h[i];
        if (c_out) c_out[i] = p.c[i];
    }
}

struct BatchedLayout {
    size_t h, c, lg, tok, fin, live, total;
};

BatchedLayout batched_layout(int rows, int Vp, int H, int L) {
    BatchedLayout o{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t r = off; off += i2l_align(bytes); return r; };
    const size_t LBH = (size_t)L * rows * H;
    o.h = take(2 * LBH * sizeof(float));
    o.c = take(LBH * sizeof(float));
    o.lg = take((size_t)rows * Vp * sizeof(float));
    o.tok = take((size_t)rows * sizeof(int));
    o.fin = take((size_t)rows * sizeof(int));
    o.live = take(sizeof(unsigned));
    o.total = off;
    return o;
}

inline bool batched_dims_ok(int rows, int V, int H, int L) {
    return rows > 0 && V > 0 && H > 0 && H % 64 == 0 && H <= 2048 && L > 0 && L <= MAXL;
}
