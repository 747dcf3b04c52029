// Constrained selection for the step-batched decode (included by decode.hip inside its anonymous namespace, after
// sample_batched.inc.h and the rules headers): a greedy or sampled formula that keeps a rule set and ends on END within
// `steps`.  A rule set is a rule model (bracket_rules.inc.h: State, Row, row, allowed, advance) -- BracketModel: groups
// nest, 16 bytes of state per row; ArgumentModel (argument_rules.inc.h): and every command gets the arguments it
// demands, 32 bytes -- and ConstraintRule<Model> makes it a model of the selection kernels' pick policy
// (decode_batched.inc.h): a mask inside the selection launch and the row's state.  So the constrained launches are the
// plain kernel templates under Rule = ConstrainRule or ArgumentRule, and a new rule set is a model and an alias:
//
//   select_batched_kernel<Rule>   one wave per row: the class byte is read beside the logit, the allowed predicate is
//                                 evaluated from the row's scalars (derived ONCE when the policy is built from the
//                                 state), the first-index arg max runs over the allowed columns only.
//   sample_batched_kernel<Rule>   one workgroup per row: sample_row with the predicate, so that a disallowed column
//                                 enters the softmax as -INFINITY.
//   pick_select_kernel<Rule>,     the same two row functions over a caller's logits (i2l_constrained_pick_logits,
//   sample_logits_kernel<Rule>    i2l_arguments_pick_logits).
//
// After the pick ONE thread commits the token (commit_token_batched) and stores the advanced state, in plain C++.  The
// launches stay on the serial chain of every step exactly where the plain ones are: no exchange, no poll, no host round
// trip, and the LSTM and logits launches are untouched.  If the selection returns no allowed column (a malformed table,
// or no allowed logit above -inf) the pick is constraint_fallback's: the first allowed column, else end_id.

// The pick policy of one row at one step.
template <class Model>
struct ConstraintAllow {
    const uint8_t* cls_;
    typename Model::State st;        // a copy taken before any thread advances it
    typename Model::Row r;           // what the predicate needs of it
    int end_id;
    typename Model::State* state;    // the row's, stored by finish
    uint8_t* mask_;                  // the row's V bytes of the allowed set, or null
    __device__ __forceinline__ uint8_t cls(int v) const { return cls_[v]; }
    __device__ __forceinline__ bool allows(int v, uint8_t c) const { return Model::allowed(r, v == end_id, c); }
    __device__ __forceinline__ bool operator()(int v) const { return allows(v, cls_[v]); }
    __device__ __forceinline__ uint8_t* mask() const { return mask_; }
    __device__ __forceinline__ int winner_cls(int c, int v) const { return __shfl(c, v & 63, 64); }
    // By one thread: a pick the selection could not make, the new state.  pick_cls >= 0: the class byte of a pick the
    // caller took from the allowed columns; -1: look `pick` up.
    __device__ __forceinline__ int finish_argmax(int V, int pick, int pick_cls) const {
        if (pick_cls < 0) {
            if (pick < 0 || pick >= V || !(*this)(pick)) pick = constraint_fallback<Model>(r, cls_, V, end_id);
            pick_cls = cls_[pick];
        }
        typename Model::State next = st;
        Model::advance(next, pick == end_id, (uint8_t)pick_cls);
        *state = next;
        return pick;
    }
    __device__ __forceinline__ int finish_sample(int V, int pick) const { return finish_argmax(V, pick, -1); }
};

template <class Model>
struct ConstraintRule {
    const uint8_t* cls;              // [V] table bytes
    typename Model::State* state;    // [rows]
    uint8_t* allowed;                // [rows][V] the allowed sets out, or null
    __device__ __forceinline__ ConstraintAllow<Model> row(int row, int V, int end_id, int rem) const {
        const typename Model::State st = state[row];
        return {cls, st, Model::row(st, rem), end_id, state + row, allowed ? allowed + (size_t)row * V : nullptr};
    }
};
using ConstrainRule = ConstraintRule<BracketModel>;    // the beam step's too (beam_batched.inc.h)
using ArgumentRule = ConstraintRule<ArgumentModel>;    // the greedy and sampling decode's only

// The arg max of the pick-logits entries: select_row applied once to (rows, ld) logits of the caller, one wave per row.
template <class Rule>
__global__ __launch_bounds__(DB_NT) void pick_select_kernel(const float* __restrict__ logits, int ld, int rows, int V,
                                                            float temperature, int use_temp, int select, Rule c,
                                                            int end_id, int rem, int32_t* __restrict__ ids) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DB_NT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const auto al = c.row(row, V, end_id, rem);
    int pick_cls;
    const int pick = select_row(logits + (size_t)row * ld, V, temperature, use_temp, select, al, nullptr, lane, &pick_cls);
    if (lane == 0) ids[row] = al.finish_argmax(V, pick, pick_cls);
}
