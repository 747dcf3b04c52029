// Bracket-constrained selection for the step-batched decode (included by decode.hip inside its anonymous namespace,
// after sample_batched.inc.h): a greedy or sampled formula whose groups nest and which ends on END within `steps`.
// The rules are bracket_rules.inc.h's; here they are the bracket model of the selection kernels' pick policy
// (decode_batched.inc.h) -- a mask inside the selection launch and 16 bytes of state per row -- so the constrained
// launches are the plain kernel templates under ConstrainRule:
//
//   select_batched_kernel<ConstrainRule>   one wave per row: the class byte is read beside the logit, the allowed predicate
//                                          is evaluated from the row's state (loaded once), the first-index arg max runs
//                                          over the allowed columns only.
//   sample_batched_kernel<ConstrainRule>   one workgroup per row: sample_row with the predicate, so that a disallowed
//                                          column enters the softmax as -INFINITY.
//   pick_constrained_select_kernel,        the same two row functions over a caller's logits
//   sample_logits_kernel<ConstrainRule>    (i2l_constrained_pick_logits).
//
// After the pick ONE thread commits the token (commit_token_batched) and advances the state.  The launches stay on the
// serial chain of every step exactly where the plain ones are: no exchange, no poll, no host round trip, and the LSTM
// and logits launches are untouched.  If the selection returns no allowed column (a malformed table, or no allowed
// logit above -inf) the pick is br_fallback's: the first allowed column, else end_id.

// The pick policy of one row at one step; the state is a copy taken before any thread advances it.
struct BracketAllow {
    const uint8_t* cls_;
    BracketState st;
    int end_id, rem;
    BracketState* state;     // the row's, stored by finish
    uint8_t* mask_;          // the row's V bytes of the allowed set, or null
    __device__ __forceinline__ uint8_t cls(int v) const { return cls_[v]; }
    __device__ __forceinline__ bool allows(int v, uint8_t c) const { return br_allowed(st, v == end_id, c, rem); }
    __device__ __forceinline__ bool operator()(int v) const { return allows(v, cls_[v]); }
    __device__ __forceinline__ uint8_t* mask() const { return mask_; }
    __device__ __forceinline__ int winner_cls(int c, int v) const { return __shfl(c, v & 63, 64); }
    // By one thread: a pick the selection could not make, the new state.  pick_cls >= 0: the class byte of a pick the
    // caller took from the allowed columns; -1: look `pick` up.
    __device__ __forceinline__ int finish_argmax(int V, int pick, int pick_cls) const {
        if (pick_cls < 0) {
            if (pick < 0 || pick >= V || !(*this)(pick)) pick = br_fallback(st, cls_, V, end_id, rem);
            pick_cls = cls_[pick];
        }
        BracketState next = st;
        br_advance(next, pick == end_id, (uint8_t)pick_cls);
        *state = next;
        return pick;
    }
    __device__ __forceinline__ int finish_sample(int V, int pick) const { return finish_argmax(V, pick, -1); }
};

struct ConstrainRule {
    const uint8_t* cls;      // [V] class bytes
    BracketState* state;     // [rows]
    uint8_t* allowed;        // [rows][V] the allowed sets out, or null
    __device__ __forceinline__ BracketAllow row(int row, int V, int end_id, int rem) const {
        return {cls, state[row], end_id, rem, state + row, allowed ? allowed + (size_t)row * V : nullptr};
    }
};

// i2l_constrained_pick_logits, arg max: select_row applied once to (rows, ld) logits of the caller, one wave per row.
__global__ __launch_bounds__(DB_NT) void pick_constrained_select_kernel(const float* __restrict__ logits, int ld, int rows,
                                                                        int V, float temperature, int use_temp, int select,
                                                                        ConstrainRule c, int end_id, int rem,
                                                                        int32_t* __restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const BracketAllow al = c.row(row, V, end_id, rem);
    int pick_cls;
    const int pick = select_row(logits + (size_t)row * ld, V, temperature, use_temp, select, al, nullptr, lane, &pick_cls);
    if (lane == 0) ids[row] = al.finish_argmax(V, pick, pick_cls);
}
