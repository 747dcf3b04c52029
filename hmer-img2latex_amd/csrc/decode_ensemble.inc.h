// Ensemble decode on the step-batched loop (included by decode.hip inside an anonymous namespace, before launch_batched,
// which is the loop for one decoder and for several): M decoders of one vocabulary read the SAME tokens, each runs its
// own recurrences and logits on its own state, one kernel combines their rows (ensemble_rules.inc.h) and the existing
// selection kernels pick from the combined row.  (This package: the reference decodes with one model.)
//
//   step t:  for every member  launch_batched_step            its L LSTM launches and its logits launch, unchanged kernels
//            ensemble_combine_kernel<M>                       the members' [B][Vp] rows -> the ensemble's [B][Vp] row
//            launch_batched_select                            select_batched_kernel / sample_batched_kernel under NoRule,
//                                                             ConstrainRule or ArgumentRule, on a BatchedParams whose lg
//                                                             is the combined buffer
// so a step is sum(L_m) + M + 2 launches: one more (the combine) and M - 1 fewer (the selections) than M separate
// decodes.  tok, fin, live and ids are shared: every member's LSTM kernel reads the token the ONE selection committed,
// and every kernel of a later step returns on the one live word under I2L_STOP_STICKY.  With M == 1 the combine is
// skipped and the selection reads the member's own lg: a single-decoder entry's launches.  This file holds the combine
// kernel, the ensemble's scratch layout and the check of its members.
//
// ensemble_combine_kernel: one wave per row (select_batched_kernel's grid and block).  The row is at most 8 x 2048
// floats that the logits launches have just written, so the kernel is bound by the latency of its loads, not by their
// volume.  A lane holds a CHUNK of the row in registers -- ENS_CHUNK columns, lane-strided, of every member -- and the
// M x ENS_CHUNK loads of a chunk are issued together: one round trip to memory per chunk, not one per column.  Pass 1
// walks the chunks and accumulates every member's (max, sum exp) online, then reduces them over the wave; pass 2 walks
// them backwards and writes y[0, V), so that the last chunk of pass 1 is still in registers: a row of V <= 512 columns
// (the shipped vocabulary) is read ONCE.  Measured at 256 rows x 500 columns: 9.0 us a launch with two column-by-column
// passes (four round trips each at two columns in flight), see profiles/ensemble_decode_cost.txt for this form.
// Columns [V, Vp) of the combined buffer are never written: no selection kernel reads them.  The member pointers,
// strides and weights are launch arguments.

#include "ensemble_rules.inc.h"

struct EnsembleRows {
    const float* lg[ENS_MAX];    // member m's [B][ld[m]] logits of the current step
    int ld[ENS_MAX];
    float w[ENS_MAX], logw[ENS_MAX];
    float* out;                  // [B][ld_out]
    int ld_out, B, V, rule;
    const unsigned* live;
};

constexpr int ENS_CHUNK = 8;     // columns of a member a lane holds: 64 * ENS_CHUNK = 512 columns of the row per chunk

// chunk `c` of the members' rows: a[m][i] = x_m[512 c + 64 i + lane], -inf beyond V (ens_accumulate passes over it)
template <int M>
__device__ __forceinline__ void ens_load_chunk(float (&a)[M][ENS_CHUNK], const float* const (&x)[M], int c, int V, int lane) {
#pragma unroll
    for (int i = 0; i < ENS_CHUNK; ++i) {
        const int v = (c * ENS_CHUNK + i) * 64 + lane;
#pragma unroll
        for (int m = 0; m < M; ++m) a[m][i] = v < V ? x[m][v] : -INFINITY;
    }
}

template <int M>
__global__ __launch_bounds__(DB_NT) void ensemble_combine_kernel(EnsembleRows e) {
    if (*e.live == 0) return;
    const int V = e.V, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6);
    if (row >= e.B) return;
    const float* x[M];
    float a[M][ENS_CHUNK], mx[M], s[M], top[M], log_s[M];
#pragma unroll
    for (int m = 0; m < M; ++m) { x[m] = e.lg[m] + (size_t)row * e.ld[m]; mx[m] = -INFINITY; s[m] = 0.f; }
    const int chunks = (V + 64 * ENS_CHUNK - 1) / (64 * ENS_CHUNK);
    for (int c = 0; c < chunks; ++c) {
        ens_load_chunk<M>(a, x, c, V, lane);
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int i = 0; i < ENS_CHUNK; ++i) ens_accumulate(mx[m], s[m], a[m][i]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        top[m] = wave_max(mx[m]);
        log_s[m] = logf(wave_sum(ens_rescale(mx[m], s[m], top[m])));
    }
    float* y = e.out + (size_t)row * e.ld_out;
    for (int c = chunks - 1; c >= 0; --c) {
        if (c != chunks - 1) ens_load_chunk<M>(a, x, c, V, lane);      // the last chunk is still in registers
#pragma unroll
        for (int i = 0; i < ENS_CHUNK; ++i) {
            const int v = (c * ENS_CHUNK + i) * 64 + lane;
            float lp[M];
#pragma unroll
            for (int m = 0; m < M; ++m) lp[m] = ens_logprob(a[m][i], top[m], log_s[m]);
            if (v < V) y[v] = ens_combine<M>(lp, e.w, e.logw, e.rule);
        }
    }
}

struct EnsembleLayout {
    size_t member[ENS_MAX];      // each a batched_layout of that member's H and L
    size_t combined;             // [rows][Vp]
    size_t total;
};

EnsembleLayout ensemble_layout(const i2l_ensemble_member* members, int n, int rows, int Vp) {
    EnsembleLayout o{};
    size_t off = 0;
    for (int m = 0; m < n; ++m) {
        o.member[m] = off;
        off += batched_layout(rows, Vp, members[m].w->hidden, members[m].w->layers).total;
    }
    o.combined = off;
    off += i2l_align((size_t)rows * Vp * sizeof(float));
    o.total = off;
    return o;
}

// n in 1 .. I2L_MAX_ENSEMBLE, every member complete, accepted by the step-batched kernels and of one vocabulary
int check_members(const i2l_ensemble_member* members, int n) {
    if (!members || n < 1) return I2L_ERR_ARG;
    if (n > I2L_MAX_ENSEMBLE) return I2L_ERR_UNSUPPORTED;
    for (int m = 0; m < n; ++m) {
        int rc = check_weights(members[m].w);
        if (rc != I2L_OK) return rc;
        if (!members[m].workspace) return I2L_ERR_ARG;
    }
    for (int m = 1; m < n; ++m)
        if (members[m].w->vocab != members[0].w->vocab) return I2L_ERR_ARG;
    return I2L_OK;
}
