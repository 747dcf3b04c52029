// Step-batched beam search on the MATRIX CORES for decoders the grouped beam kernel does not take (the shipped 2 x 512
// one): the K slots of every image are rows of ONE batched step, R = images * K rows, row r = slot r % K of image r / K
// (included by decode.hip inside its anonymous namespace, after decode_constrained.inc.h and beam_bracket_rules.inc.h).
// Reference seq2seq.py:234-298.
//
// Per step the host enqueues L launches of lstm_step_mfma_kernel<TB> and one of logits_mfma_kernel<TB> on the R rows
// (decode_batched.inc.h, unchanged but for the Genc row: a beam row reads the encoder half of its image, row / K), then
//
//   beam_step_batched_kernel<K>  one workgroup per image: phases (c) - (f) of beam_kernel<K> (decode.hip) and phase (a)
//                                of the NEXT step, with the search state in the scratch instead of LDS.
//
// Both kernels run the same code: phase (c) is beam_topk_row (decode.hip), the serial rules (a), (d), (f) and the result
// are beam_rules.inc.h's.  Only where the state lives differs: there the rows, scores and flags are LDS arrays of one
// workgroup that loops over the steps, here they are global arrays indexed per image and the step loop is the host's.
//
// State hazards.  The GEMM launches read h[par] and write h[par ^ 1]; the gather (e) moves h[par ^ 1] of a slot's parent
// into h[par] of the slot, so every step runs at parity 0.  c is updated in place by the GEMM launches, and the slots of
// one image read each other's rows in the gather, so c has two buffers: step t updates c[t & 1] and gathers it into
// c[(t + 1) & 1], which the next step's launches get.  Rows of unused or retired slots and of finished images still ride
// through the GEMMs on a clamped token; no row reads another row there and nothing reads their results.
//
// Early end: one device word counts the images still searching; every launch of a later step reads it first and returns
// when it is 0.  All steps are always enqueued.  No polls, no cooperative launch, no exchange: nothing can time out.

struct BeamBatchedParams {
    int images, T, V, Vp, H, L, start_id, end_id;
    int32_t* tokhist;    // [images][T][K]  token chosen for slot q at step t
    int32_t* parhist;    // [images][T][K]  slot (of step t-1) it extends
    float* h;            // [2][L][R][H]
    float* c;            // [2][L][R][H]
    const float* lg;     // [R][Vp]
    double* score;       // [R]
    int* last;           // [R] last token of each slot (the GEMM launches' tok)
    int* slot_live;      // [R]
    BeamImage* img;      // [images]
    unsigned* live;      // images still searching
    int32_t* seq_out;    // [images][T+1]
    int32_t* len_out;    // [images]
    double* score_out;   // [images] or null
    // the N-best search (beam_nbest.inc.h) keeps every completed beam instead of the best one; unused here
    int N;                   // rows per image
    const double* norm;      // [T + 1] length divisors, or null = all ones
    NbestEntry* list;        // [images][N], the first img[i].has_c in use, keys non-increasing
};

// The image's "completed" sink: the N-best search (beam_nbest.inc.h) keeps a list, the plain one the best entry.
template <bool NBEST>
__device__ __forceinline__ auto beam_sink(const BeamBatchedParams& p, int img) {
    if constexpr (NBEST) return BeamList{p.list + (size_t)img * p.N, p.N, p.norm};
    else return BeamBest{};
}

// zero state and the start of every image's search: slot 0 = START, (a) of step 0 (START == END: the empty sequence,
// which the N-best search's own init kernel puts into its list)
__global__ __launch_bounds__(DB_NT) void beam_init_batched_kernel(BeamBatchedParams p, int K) {
    const size_t R = (size_t)p.images * K, LRH2 = 2 * (size_t)p.L * R * p.H;
    const size_t i0 = (size_t)blockIdx.x * DB_NT + threadIdx.x, stride = (size_t)gridDim.x * DB_NT;
    for (size_t i = i0; i < LRH2; i += stride) { p.h[i] = 0.f; p.c[i] = 0.f; }
    for (size_t i = i0; i < (size_t)p.images; i += stride) {
        BeamImage im;
        beam_start(im, BeamBest{}, p.score + i * K, p.last + i * K, p.slot_live + i * K, K, p.start_id, p.end_id);
        p.img[i] = im;
    }
    if (i0 == 0) *p.live = p.start_id == p.end_id ? 0u : (unsigned)p.images;
}

// Ranking, gather and retirement of step t (after its logits launch).  grid images; c_cur: the buffer the step's LSTM
// launches updated, c_next: the one the next step's get.  NBEST: the kernel of i2l_beam_decode_nbest, the same step with
// the image's list as the sink.  Rule: the slots' pick policy (decode_batched.inc.h) -- NoRule, or ConstrainRule for the
// well-formed search (beam_constrained.inc.h), where slot r0 + q keeps 16 bytes of bracket state in rule.state: phase (c)
// ranks the columns the slot's state allows, (d) gets the slots' candidate counts, and after (d) new slot q takes its
// parent's state advanced by its token.  Everything of it is under `if constexpr`: with NoRule this is the kernel without.
template <int K, bool NBEST = false, class Rule = NoRule>
__global__ __launch_bounds__(DB_NT) void beam_step_batched_kernel(BeamBatchedParams p, float* __restrict__ c_cur,
                                                                  float* __restrict__ c_next, int t, Rule rule) {
    constexpr bool CON = std::is_same_v<Rule, ConstrainRule>;
    __shared__ double nscore[K];
    __shared__ float topv[K * K];                        // [K][K] log-probs, descending
    __shared__ int topi[K * K];
    __shared__ int npar[K], ntok[K], ctl[1];
    __shared__ double oscore[K];                         // the slots' scores and live flags as the step found them: the
    __shared__ int olive[K];                             // serial ranking of (d) reads them K * K times over
    __shared__ BracketState ostate[CON ? K : 1];         // and their bracket states: a parent's is read after (d)
    __shared__ int ncand[CON ? K : 1];                   // candidates of each live slot, 1 .. K
    if (*p.live == 0) return;
    const int img = blockIdx.x;
    BeamImage* im = p.img + img;
    if (im->done) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int V = p.V, Vp = p.Vp, H = p.H, L = p.L, T = p.T;
    const size_t R = (size_t)p.images * K, r0 = (size_t)img * K;
    int* slot_live = p.slot_live + r0;
    double* score = p.score + r0;
    int32_t* tokhist = p.tokhist + (size_t)img * T * K;
    int32_t* parhist = p.parhist + (size_t)img * T * K;

    if (tid < K) {
        oscore[tid] = score[tid]; olive[tid] = slot_live[tid];
        if constexpr (CON) ostate[tid] = rule.state[r0 + tid];
    }

    // (c) log_softmax and top-K, a wave per live slot; the policy's state is the slot's in global memory, loaded once
    for (int r = wave; r < K; r += DB_NT / 64)
        if (slot_live[r]) {                              // wave-uniform
            const auto al = rule.row((int)r0 + r, V, p.end_id, T - t - 1);
            [[maybe_unused]] const int n = beam_topk_row(p.lg + (r0 + r) * Vp, V, K, lane, al, topv + r * K, topi + r * K);
            if constexpr (CON)
                if (lane == 0) ncand[r] = bb_close_list(n, p.end_id, topv + r * K, topi + r * K);
        }
    __syncthreads();

    // (d) the ranking of the K x K candidates and the history rows
    if (tid == 0)
        ctl[0] = beam_rank(olive, oscore, topv, topi, K, CON ? ncand : nullptr, npar, ntok, nscore, tokhist + (size_t)t * K,
                           parhist + (size_t)t * K);
    __syncthreads();
    if constexpr (CON)
        if (tid < ctl[0]) rule.state[r0 + tid] = bb_inherit(ostate, npar[tid], ntok[tid], p.end_id, rule.cls);

    // (e) new slot q inherits the fresh state of its parent (hidden.clone(), :272): h[1] -> h[0], c_cur -> c_next
    {
        const int H4 = H >> 2;
        const size_t LRH = (size_t)L * R * H;
        const float4* hsrc = reinterpret_cast<const float4*>(p.h + LRH);
        float4* hdst = reinterpret_cast<float4*>(p.h);
        const float4* csrc = reinterpret_cast<const float4*>(c_cur);
        float4* cdst = reinterpret_cast<float4*>(c_next);
        for (int idx = tid; idx < L * K * H4; idx += DB_NT) {
            const int l = idx / (K * H4);
            const int rem = idx - l * (K * H4);
            const int q = rem / H4, j = rem - q * H4;
            const size_t src = ((size_t)l * R + r0 + npar[q]) * H4 + j;
            const size_t dst = ((size_t)l * R + r0 + q) * H4 + j;
            hdst[dst] = hsrc[src];
            cdst[dst] = csrc[src];
        }
    }

    // (f) the step's ending and (a) of step t + 1
    if (tid == 0) {
        BeamImage rec = *im;
        beam_step_end(rec, beam_sink<NBEST>(p, img), ctl[0], ntok, nscore, score, p.last + r0, slot_live, K, p.end_id, t, T);
        *im = rec;
        if (rec.done) atomicSub(p.live, 1u);
    }
}

// result: max(completed) (first on ties) else beams[0]; strip START, cut at END, pad with -1.  One thread per image.
__global__ __launch_bounds__(DB_NT) void beam_final_batched_kernel(BeamBatchedParams p, int K) {
    const int img = blockIdx.x * DB_NT + threadIdx.x;
    if (img >= p.images) return;
    const size_t hist = (size_t)img * p.T * K;
    double sc;
    p.len_out[img] = beam_best_result(p.img[img], p.score + (size_t)img * K, p.tokhist + hist, p.parhist + hist, K, p.end_id,
                                      p.T, p.seq_out + (size_t)img * (p.T + 1), &sc);
    if (p.score_out) p.score_out[img] = sc;
}

struct BeamBatchedLayout {
    size_t hist, h, c, lg, score, last, slot_live, img, live, total;
};

BeamBatchedLayout beam_batched_layout(int images, int K, int Vp, int H, int L, int steps) {
    BeamBatchedLayout o{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t r = off; off += i2l_align(bytes); return r; };
    const size_t R = (size_t)images * K, LRH = (size_t)L * R * H;
    o.hist = take(2 * (size_t)images * steps * K * sizeof(int32_t));
    o.h = take(2 * LRH * sizeof(float));
    o.c = take(2 * LRH * sizeof(float));
    o.lg = take(R * Vp * sizeof(float));
    o.score = take(R * sizeof(double));
    o.last = take(R * sizeof(int));
    o.slot_live = take(R * sizeof(int));
    o.img = take((size_t)images * sizeof(BeamImage));
    o.live = take(sizeof(unsigned));
    o.total = off;
    return o;
}

// vocab <= 2048: the top-K scan's taken-mask is 32 bits per lane
inline bool beam_batched_dims_ok(int images, int beam, int V, int H, int L, int steps) {
    return images > 0 && steps > 0 && beam >= 1 && beam <= I2L_MAX_BEAM && beam <= V && V <= 2048 &&
           (long)images * beam <= 0x7fffffffL / 4 && batched_dims_ok(images * beam, V, H, L);
}
