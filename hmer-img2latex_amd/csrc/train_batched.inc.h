// Step-batched training recurrences on the MATRIX CORES (I2L_FLAG_TRAIN_BATCHED; included by train_decoder.hip inside its
// anonymous namespace): the forward recurrence and the BPTT of the teacher-forced decoder as plain launches per (step,
// layer) over the whole batch, the launch boundary the only barrier, all state in global memory (no LDS-resident state, so
// no limit on H from it).  Reference decoder.py:100-195 (nn.LSTM under teacher forcing, inter-layer dropout :81).
//
//   lstm_train_step_fwd_kernel<TB>       gates[B x 4H] = (GX[bt] | biasP) + x_below . WihT + h(t-1) . WhhT and the cell in
//                                        the epilogue; lstm_step_mfma_kernel's tiles (TB rows x 64 gate columns of the
//                                        gate-interleaved [K][4H] images); writes the tape of lstm_train_fwd_kernel: ACT,
//                                        C, Hout, Hprev, and (L > 1, p > 0) the inter-layer-dropped copy of h for the
//                                        layer above.
//   lstm_train_step_bwd_prod_kernel<TB>  partial sums of dh: TB rows x 64 hidden columns x one K chunk of
//                                        DG[l](t+1) . W_hh[l] (slices 0 .. nA-1) and DG[l+1](t) . W_ih[l+1] (nA .. nA+nB-1).
//   lstm_train_step_bwd_cell_kernel      adds the slices in slice order (fixed: no atomics), the mask on the second
//                                        product only, dHtop at the top layer, then lstm_train_bwd_kernel's cell backward
//                                        element by element: DG[l][bt] in standard gate order, dc_next = dc * f.
//
// The K split of the backward.  dh is B x H, a quarter of the forward's columns, over K = 4H (8H below the top layer):
// with the forward's tiling a launch would be H/64 column tiles of four to eight times the forward's serial K loop.  The
// products are split over WORKGROUPS instead (grid z = product x chunk, TBB chunks of 4H / TBB rows each: H rows, the
// forward's recurrent chain, when the scratch has room for 2 x 4 slices, else 2H) and a second, elementwise pass sums them.
// db_slab stays as it is -- one staging and summation order for inference and training -- at the price of one more short
// launch per (step, layer) and a round trip of nA + nB slices of B x H floats through L2.
//
// Scratch of the backward: GX, which only the forward reads ([B*T][4H] floats = 4T slices of B x H): dc_next [L][B][H] at
// its head when T > 1 (T = 1 has no earlier step to hand dc to), the slices behind it.  T >= 3: L + 8 <= 12 slices; T = 2:
// L + 4 <= 8; T = 1: 2 <= 4 (only the second product exists).  Scratch of the forward: the dropped copy of Hout[l] lives in
// DG[l] ([B*T][4H], written only by the backward, which rebuilds every mask from the hash and never reads the copy).
// Neither C nor ACT is written by the backward: it can be called again on the same tape.
#include "mfma_slab.inc.h"

constexpr int TB_MAX_H = 2048;       // the step-batched decode's bound (batched_dims_ok)

inline bool train_batched_dims_ok(int V, int E, int H, int L) {
    return V > 0 && E > 0 && E % 4 == 0 && H > 0 && H % 64 == 0 && H <= TB_MAX_H && L > 0 && L <= MAXL;
}
// K chunks per backward product (see the scratch budget above)
inline int train_batched_k_chunks(int T) { return T >= 3 ? 4 : 2; }

// Layer `layer` of step t for the whole batch.  grid (H / 16, cdiv(B, TB)).  x_below: [B*T][H] input from the layer below
// (its dropped copy, or Hout[layer - 1] itself when no mask is live), NULL for layer 0; drop_out: where the dropped copy of
// this layer's output goes, NULL when nothing reads one.
template <int TB>
__global__ __launch_bounds__(DB_NT) void lstm_train_step_fwd_kernel(TrainBuf p, const float* __restrict__ x_below,
                                                                    float* __restrict__ drop_out, int layer, int t) {
    __shared__ u32x4_t ws[DbLds<TB>::WS];
    __shared__ u32x4_t xs[DbLds<TB>::XS];
    const int H = p.H, B = p.B, T = p.T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col0 = blockIdx.x * DB_COLS, row0 = blockIdx.y * TB;
    const size_t G = 4 * (size_t)H;
    f32x4_t acc[TB / 16][3];
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[nt][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (layer > 0)      // the layer below, already at step t
        db_slab<TB>(acc, p.WihT[layer], G, col0, x_below + (size_t)t * H, T * H, row0, B, H, ws, xs, tid);
    if (t > 0)
        db_slab<TB>(acc, p.WhhT[layer], G, col0, p.Hout[layer] + (size_t)(t - 1) * H, T * H, row0, B, H, ws, xs, tid);

    const int unit = (col0 >> 2) + 4 * wave + (lane >> 4);       // this lane's D rows are the gates i, f, g, o of `unit`
    const float inv_keep = p.p > 0.f ? 1.f / (1.f - p.p) : 1.f;
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt) {
        const int row = row0 + 16 * nt + (lane & 15);
        if (row >= B) continue;
        const size_t bt = (size_t)row * T + t;
        const float4 add = layer == 0 ? *reinterpret_cast<const float4*>(p.GX + bt * G + 4 * unit)
                                      : *reinterpret_cast<const float4*>(p.biasP[layer] + 4 * unit);
        const f32x4_t z = db_fold(acc[nt]);
        const float ig = sigmoidf_(z[0] + add.x), fg = sigmoidf_(z[1] + add.y);
        const float gg = tanhf_(z[2] + add.z), og = sigmoidf_(z[3] + add.w);
        const size_t ci = bt * H + unit;
        const float cp = t > 0 ? p.C[layer][ci - H] : 0.f;
        const float cn = fg * cp + ig * gg;
        const float hn = og * tanhf_(cn);
        *reinterpret_cast<float4*>(p.ACT[layer] + bt * G + 4 * unit) = make_float4(ig, fg, gg, og);
        p.C[layer][ci] = cn;
        p.Hout[layer][ci] = hn;
        if (t == 0) p.Hprev[layer][ci] = 0.f;
        if (t + 1 < T) p.Hprev[layer][ci + H] = hn;
        if (drop_out)       // nn.LSTM inter-layer dropout (decoder.py:81): the row kernel's hash, stream and element index
            drop_out[ci] = hn * keep_scale(p.seed, DS_LAYER0 + layer, ci, p.p, inv_keep);
    }
}

// Slice blockIdx.z of dh(layer, t): product first + z / ks (0: DG[layer](t+1) . W_hh[layer], 1: DG[layer+1](t) .
// W_ih[layer+1]), K chunk z % ks of 4H / ks rows.  grid (H / 64, cdiv(B, TB), slices).  part: [slices][B][H].
template <int TB>
__global__ __launch_bounds__(DB_NT) void lstm_train_step_bwd_prod_kernel(BwdBuf p, float* __restrict__ part, int layer,
                                                                         int t, int first, int ks) {
    __shared__ u32x4_t ws[DbLds<TB>::WS];
    __shared__ u32x4_t xs[DbLds<TB>::XS];
    const int H = p.H, B = p.B, T = p.T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col0 = blockIdx.x * DB_COLS, row0 = blockIdx.y * TB;
    const int slice = blockIdx.z, prod = first + slice / ks, chunk = slice % ks;
    const size_t G = 4 * (size_t)H;
    const int kc = (int)(G / ks);                                 // multiple of DB_KC: H % 64 == 0, ks = 2 or 4
    f32x4_t acc[TB / 16][3];
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[nt][c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // W: the original (4H, H) matrix, K = 4H, ldw = H; X: gate gradients in standard gate order, row stride T * 4H
    const float* W = (prod == 0 ? p.Whh[layer] : p.Wih[layer + 1]) + (size_t)chunk * kc * H;
    const float* X = (prod == 0 ? p.DG[layer] + (size_t)(t + 1) * G : p.DG[layer + 1] + (size_t)t * G) + (size_t)chunk * kc;
    db_slab<TB>(acc, W, (size_t)H, col0, X, (int)(T * G), row0, B, kc, ws, xs, tid);
    const int col = col0 + 16 * wave + 4 * (lane >> 4);          // this lane's D rows are four consecutive hidden columns
#pragma unroll
    for (int nt = 0; nt < TB / 16; ++nt) {
        const int row = row0 + 16 * nt + (lane & 15);
        if (row >= B) continue;
        const f32x4_t z = db_fold(acc[nt]);
        *reinterpret_cast<float4*>(part + ((size_t)slice * B + row) * H + col) = make_float4(z[0], z[1], z[2], z[3]);
    }
}

// dh(layer, t) from the slices, then the cell backward of lstm_train_bwd_kernel.  One thread per (row, hidden unit).
// dc_next: [L][B][H], read when t + 1 < T, written when t > 0.
__global__ __launch_bounds__(256) void lstm_train_step_bwd_cell_kernel(BwdBuf p, const float* __restrict__ part,
                                                                       float* __restrict__ dc_next, int layer, int t,
                                                                       int nA, int nB) {
    const int H = p.H, B = p.B, T = p.T;
    const size_t BH = (size_t)B * H, G = 4 * (size_t)H;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= BH) return;
    const int row = (int)(idx / H), j = (int)(idx - (size_t)row * H);
    const size_t bt = (size_t)row * T + t;
    float dh = 0.f;
    for (int s = 0; s < nA; ++s) dh += part[(size_t)s * BH + idx];
    if (layer == p.L - 1) {
        dh += p.dHtop[bt * H + j];
    } else {
        float low = 0.f;
        for (int s = 0; s < nB; ++s) low += part[(size_t)(nA + s) * BH + idx];
        const float inv_keep = p.p > 0.f ? 1.f / (1.f - p.p) : 1.f;
        dh += low * keep_scale(p.seed, DS_LAYER0 + layer, bt * H + j, p.p, inv_keep);
    }
    const float4 a = *reinterpret_cast<const float4*>(p.ACT[layer] + bt * G + 4 * j);
    const float c = p.C[layer][bt * H + j];
    const float cp = t > 0 ? p.C[layer][(bt - 1) * H + j] : 0.f;
    const size_t si = (size_t)layer * BH + idx;
    const float tc = tanhf_(c);
    const float d_o = dh * tc * a.w * (1.f - a.w);
    const float dc = dh * a.w * (1.f - tc * tc) + (t + 1 < T ? dc_next[si] : 0.f);
    const float d_i = dc * a.z * a.x * (1.f - a.x);
    const float d_f = dc * cp * a.y * (1.f - a.y);
    const float d_g = dc * a.x * (1.f - a.z * a.z);
    if (t > 0) dc_next[si] = dc * a.y;
    float* o = p.DG[layer] + bt * G;
    o[j] = d_i; o[H + j] = d_f; o[2 * H + j] = d_g; o[3 * H + j] = d_o;
}

// Forward recurrence: T x L launches on s.  drop[l]: a [B*T][H] region that is dead during the forward (DG[l]).
int train_batched_forward(const TrainBuf& p, float* const* drop, hipStream_t s) {
    const int H = p.H, B = p.B, L = p.L;
    const int tb = batched_tile_rows(H / 16, B);
    const dim3 grid(H / 16, i2l_cdiv(B, tb));
    const bool masked = L > 1 && p.p > 0.f;
    for (int t = 0; t < p.T; ++t)
        for (int l = 0; l < L; ++l) {
            const float* below = l == 0 ? nullptr : (masked ? drop[l - 1] : p.Hout[l - 1]);
            float* out = masked && l + 1 < L ? drop[l] : nullptr;
            if (tb == 16) hipLaunchKernelGGL(lstm_train_step_fwd_kernel<16>, grid, dim3(DB_NT), 0, s, p, below, out, l, t);
            else if (tb == 32) hipLaunchKernelGGL(lstm_train_step_fwd_kernel<32>, grid, dim3(DB_NT), 0, s, p, below, out, l, t);
            else hipLaunchKernelGGL(lstm_train_step_fwd_kernel<64>, grid, dim3(DB_NT), 0, s, p, below, out, l, t);
            I2L_CHECK_LAUNCH();
        }
    return I2L_OK;
}

// BPTT: per (t, l), top down, the slices of dh and the cell pass.  scratch: a region of at least 4T x [B][H] floats that the
// backward does not read otherwise (GX).
int train_batched_backward(const BwdBuf& p, float* scratch, hipStream_t s) {
    const int H = p.H, B = p.B, L = p.L, T = p.T;
    const size_t BH = (size_t)B * H;
    const int ks = train_batched_k_chunks(T);
    float* dc_next = scratch;
    float* part = scratch + (T > 1 ? (size_t)L * BH : 0);
    const int cell_grid = (int)((BH + 255) / 256);
    for (int t = T - 1; t >= 0; --t)
        for (int l = L - 1; l >= 0; --l) {
            const int nA = t + 1 < T ? ks : 0, nB = l + 1 < L ? ks : 0;
            if (nA + nB > 0) {
                const int tb = batched_tile_rows((H / 64) * (nA + nB), B);
                const dim3 grid(H / 64, i2l_cdiv(B, tb), nA + nB);
                const int first = nA ? 0 : 1;
                if (tb == 16)
                    hipLaunchKernelGGL(lstm_train_step_bwd_prod_kernel<16>, grid, dim3(DB_NT), 0, s, p, part, l, t, first, ks);
                else if (tb == 32)
                    hipLaunchKernelGGL(lstm_train_step_bwd_prod_kernel<32>, grid, dim3(DB_NT), 0, s, p, part, l, t, first, ks);
                else
                    hipLaunchKernelGGL(lstm_train_step_bwd_prod_kernel<64>, grid, dim3(DB_NT), 0, s, p, part, l, t, first, ks);
                I2L_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(lstm_train_step_bwd_cell_kernel, dim3(cell_grid), dim3(256), 0, s, p, (const float*)part,
                               dc_next, l, t, nA, nB);
            I2L_CHECK_LAUNCH();
        }
    return I2L_OK;
}
