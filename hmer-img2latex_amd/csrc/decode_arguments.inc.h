// Argument-complete selection for the step-batched decode (included by decode.hip inside its anonymous namespace, after
// decode_constrained.inc.h): a greedy or sampled formula whose groups nest, whose commands get every argument they
// demand, and which ends on END within `steps`.  The rules are argument_rules.inc.h's; here they are a second model of
// the selection kernels' pick policy (decode_batched.inc.h), beside the bracket one -- a mask inside the selection
// launch and 32 bytes of state per row -- so the launches are the plain kernel templates under ArgumentRule:
//
//   select_batched_kernel<ArgumentRule>, sample_batched_kernel<ArgumentRule>   the last launch of a step
//   pick_arguments_select_kernel, sample_logits_kernel<ArgumentRule>           the same two row functions over a
//                                                                              caller's logits (i2l_arguments_pick_logits)
//
// The row's scalars (depth, what is owed here, the innermost kind, the room left) are derived ONCE when the policy is
// built from the state; the per-column predicate is a byte decode and a few compares.  After the pick ONE thread commits
// the token and stores the advanced state, in plain C++.  No launch, exchange or poll is added to a step.

struct ArgumentAllow {
    const uint8_t* cls_;
    ArgumentState st;        // a copy taken before any thread advances it
    ArgumentRow r;
    int end_id;
    ArgumentState* state;    // the row's, stored by finish
    uint8_t* mask_;          // the row's V bytes of the allowed set, or null
    __device__ __forceinline__ uint8_t cls(int v) const { return cls_[v]; }
    __device__ __forceinline__ bool allows(int v, uint8_t c) const { return ar_allowed(r, v == end_id, c); }
    __device__ __forceinline__ bool operator()(int v) const { return allows(v, cls_[v]); }
    __device__ __forceinline__ uint8_t* mask() const { return mask_; }
    __device__ __forceinline__ int winner_cls(int c, int v) const { return __shfl(c, v & 63, 64); }
    // By one thread, as BracketAllow's: pick_cls >= 0 is the byte of a pick taken from the allowed columns, -1: look it up.
    __device__ __forceinline__ int finish_argmax(int V, int pick, int pick_cls) const {
        if (pick_cls < 0) {
            if (pick < 0 || pick >= V || !(*this)(pick)) pick = ar_fallback(r, cls_, V, end_id);
            pick_cls = cls_[pick];
        }
        ArgumentState next = st;
        ar_advance(next, pick == end_id, (uint8_t)pick_cls);
        *state = next;
        return pick;
    }
    __device__ __forceinline__ int finish_sample(int V, int pick) const { return finish_argmax(V, pick, -1); }
};

struct ArgumentRule {
    const uint8_t* cls;      // [V] table bytes
    ArgumentState* state;    // [rows]
    uint8_t* allowed;        // [rows][V] the allowed sets out, or null
    __device__ __forceinline__ ArgumentAllow row(int row, int V, int end_id, int rem) const {
        const ArgumentState st = state[row];
        return {cls, st, ar_row(st, rem), end_id, state + row, allowed ? allowed + (size_t)row * V : nullptr};
    }
};

// i2l_arguments_pick_logits, arg max: select_row applied once to (rows, ld) logits of the caller, one wave per row.
__global__ __launch_bounds__(DB_NT) void pick_arguments_select_kernel(const float* __restrict__ logits, int ld, int rows,
                                                                      int V, float temperature, int use_temp, int select,
                                                                      ArgumentRule c, int end_id, int rem,
                                                                      int32_t* __restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const ArgumentAllow al = c.row(row, V, end_id, rem);
    int pick_cls;
    const int pick = select_row(logits + (size_t)row * ld, V, temperature, use_temp, select, al, nullptr, lane, &pick_cls);
    if (lane == 0) ids[row] = al.finish_argmax(V, pick, pick_cls);
}
