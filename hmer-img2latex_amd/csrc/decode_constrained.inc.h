// Bracket-constrained selection for the step-batched decode (included by decode.hip inside its anonymous namespace,
// after sample_batched.inc.h): a greedy or sampled formula whose groups nest and which ends on END within `steps`.
// The rules are bracket_rules.inc.h's; here they are a mask inside the selection launch and 16 bytes of state per row.
//
//   select_constrained_kernel   select_batched_kernel's twin, one wave per row: the class byte is read beside the
//                               logit, the allowed predicate is evaluated from the row's state (loaded once), the
//                               first-index arg max runs over the allowed columns only.
//   sample_constrained_kernel   sample_batched_kernel's twin, one workgroup per row: sample_row with the predicate, so
//                               that a disallowed column enters the softmax as -INFINITY.
//   pick_constrained_*_kernel   the same two row functions over a caller's logits (i2l_constrained_pick_logits).
//
// After the pick ONE thread commits the token (commit_token_batched) and advances the state.  The launches stay on the
// serial chain of every step exactly where the plain ones were: no exchange, no poll, no host round trip, and the LSTM
// and logits launches are untouched.  If the selection returns no allowed column (a malformed table, or no allowed
// logit above -inf) the pick is br_fallback's: the first allowed column, else end_id.

struct ConstrainRule {
    const uint8_t* cls;      // [V] class bytes
    BracketState* state;     // [rows]
};

// the allowed predicate of one row at one step; the state is a copy taken before any thread advances it
struct BracketAllow {
    const uint8_t* cls;
    BracketState st;
    int end_id, rem;
    __device__ __forceinline__ bool allows(int v, uint8_t c) const { return br_allowed(st, v == end_id, c, rem); }
    __device__ __forceinline__ bool operator()(int v) const { return allows(v, cls[v]); }
};

// By one thread: a pick the selection could not make, the new state.  pick_cls >= 0: the class byte of a pick the caller
// took from the allowed columns, so that nothing is loaded between the selection and the commit; -1: look `pick` up.
__device__ __forceinline__ int constrained_finish(const BracketAllow& al, int V, int pick, int pick_cls, BracketState* state) {
    if (pick_cls < 0) {
        if (pick < 0 || pick >= V || !al(pick)) pick = br_fallback(al.st, al.cls, V, al.end_id, al.rem);
        pick_cls = al.cls[pick];
    }
    BracketState st = al.st;
    br_advance(st, pick == al.end_id, (uint8_t)pick_cls);
    *state = st;
    return pick;
}

// One row by one wave: select_batched_kernel's rule over the allowed columns of x[0, V).  lo (V floats or null) receives
// the raw logits, mask (V bytes or null) the allowed set.  Every lane returns the arg max and in *pick_cls its class byte
// -- the winner is the local best of the lane that owns its column, v & 63, which hands the class over by a shuffle --
// or 0x7fffffff and -1 if there is none.
__device__ __forceinline__ int select_row_constrained(const float* __restrict__ x, int V, float temperature, int use_temp,
                                                      int select, const BracketAllow& al, float* __restrict__ lo,
                                                      uint8_t* __restrict__ mask, int lane, int* pick_cls) {
    float best = -INFINITY;
    int besti = 0x7fffffff, bestc = 0;
    for (int v = lane; v < V; v += 64) {
        float a = x[v];
        const uint8_t c = al.cls[v];
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
            const uint8_t c = al.cls[v];
            if (al.allows(v, c) && pr > pbest) { pbest = pr; pbesti = v; bestc = c; }
        }
        wave_argmax(pbest, pbesti);
        besti = pbesti;
    }
    const int c = __shfl(bestc, besti & 63, 64);
    *pick_cls = besti < V ? c : -1;
    return besti;
}

// Token selection of step t under the constraint, one wave per row; grid as select_batched_kernel.
__global__ __launch_bounds__(DB_NT) void select_constrained_kernel(BatchedParams p, ConstrainRule c, int t) {
    if (*p.live == 0) return;
    const int V = p.w.V, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6);
    if (row >= p.B) return;
    const BracketAllow al{c.cls, c.state[row], p.end_id, p.T - t - 1};
    float* lo = p.logits_out ? p.logits_out + ((size_t)row * p.T + t) * V : nullptr;
    int pick_cls;
    const int pick = select_row_constrained(p.lg + (size_t)row * p.w.Vp, V, p.temperature, p.use_temp, p.select, al, lo,
                                            nullptr, lane, &pick_cls);
    if (lane == 0) commit_token_batched(p, row, t, constrained_finish(al, V, pick, pick_cls, c.state + row));
}

// Token selection of step t by sampling under the constraint, one workgroup per row.
__global__ __launch_bounds__(NT) void sample_constrained_kernel(BatchedParams p, SampleRule r, ConstrainRule c, int t) {
    __shared__ SampleLds s;
    if (*p.live == 0) return;
    const int V = p.w.V, row = blockIdx.x, tid = threadIdx.x;
    const BracketAllow al{c.cls, c.state[row], p.end_id, p.T - t - 1};
    float* po = r.probs ? r.probs + ((size_t)row * p.T + t) * V : nullptr;
    const int pick = sample_row(p.lg + (size_t)row * p.w.Vp, V, p.temperature, p.use_temp, r.top_k, r.top_p,
                                uniform01(r.seed, (unsigned)row, (unsigned)t), po, s, tid, al);
    // every thread took its copy of the state before the first barrier of sample_row; thread 0 stores behind the last one
    if (tid == 0) commit_token_batched(p, row, t, constrained_finish(al, V, pick, -1, c.state + row));
}

// i2l_constrained_pick_logits, arg max: the rule applied once to (rows, ld) logits of the caller, one wave per row.
__global__ __launch_bounds__(DB_NT) void pick_constrained_select_kernel(const float* __restrict__ logits, int ld, int rows,
                                                                        int V, float temperature, int use_temp, int select,
                                                                        ConstrainRule c, int end_id, int rem,
                                                                        int32_t* __restrict__ ids,
                                                                        uint8_t* __restrict__ allowed) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const BracketAllow al{c.cls, c.state[row], end_id, rem};
    int pick_cls;
    const int pick = select_row_constrained(logits + (size_t)row * ld, V, temperature, use_temp, select, al, nullptr,
                                            allowed ? allowed + (size_t)row * V : nullptr, lane, &pick_cls);
    if (lane == 0) ids[row] = constrained_finish(al, V, pick, pick_cls, c.state + row);
}

// i2l_constrained_pick_logits, sampling: one workgroup per row.
__global__ __launch_bounds__(NT) void pick_constrained_sample_kernel(const float* __restrict__ logits, int ld, int V,
                                                                     float temperature, int use_temp, SampleRule r,
                                                                     unsigned step, ConstrainRule c, int end_id, int rem,
                                                                     int32_t* __restrict__ ids,
                                                                     uint8_t* __restrict__ allowed) {
    __shared__ SampleLds s;
    const int row = blockIdx.x, tid = threadIdx.x;
    const BracketAllow al{c.cls, c.state[row], end_id, rem};
    if (allowed)
        for (int v = tid; v < V; v += NT) allowed[(size_t)row * V + v] = al(v) ? 1 : 0;
    float* po = r.probs ? r.probs + (size_t)row * V : nullptr;
    const int pick = sample_row(logits + (size_t)row * ld, V, temperature, use_temp, r.top_k, r.top_p,
                                uniform01(r.seed, (unsigned)row, step), po, s, tid, al);
    if (tid == 0) ids[row] = constrained_finish(al, V, pick, -1, c.state + row);
}
