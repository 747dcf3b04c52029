// Well-formed N-best beam search (included by decode.hip inside its anonymous namespace, after beam_nbest.inc.h): the
// search of i2l_beam_decode_nbest with the bracket constraint inside the step kernel.  The rules are
// beam_bracket_rules.inc.h's; the kernels are the n-best ones under ConstrainRule (decode_constrained.inc.h) in NoRule's
// place -- beam_topk_row ranks the columns a slot's bracket state allows and renormalises over them,
// beam_step_batched_kernel<K, true, ConstrainRule> hands the candidate counts to beam_rank and the parents' states on to
// the new slots.  The same launches per step as the plain search, the same early-end word, no poll and no exchange.
//
// What is specific to the constraint is here: 16 bytes of bracket state per slot behind the n-best scratch, their zero
// (the initial state); the dimensions are beam_nbest_dims_ok's.  With nbest = 1 and a null table it is the constrained
// single-best search.

__global__ __launch_bounds__(DB_NT) void beam_constrained_init_kernel(BracketState* __restrict__ state, size_t slots) {
    const size_t i = (size_t)blockIdx.x * DB_NT + threadIdx.x;
    if (i < slots) state[i] = BracketState{};
}

struct BeamConstrainedLayout {
    BeamNbestLayout n;
    size_t state, total;
};

BeamConstrainedLayout beam_constrained_layout(int images, int K, int N, int Vp, int H, int L, int steps) {
    BeamConstrainedLayout o{};
    o.n = beam_nbest_layout(images, K, N, Vp, H, L, steps);
    o.state = i2l_align(o.n.total);
    o.total = o.state + i2l_align((size_t)images * K * sizeof(BracketState));
    return o;
}
