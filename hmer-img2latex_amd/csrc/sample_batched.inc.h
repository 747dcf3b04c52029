// Top-k / top-p sampling for the step-batched decode (included by decode.hip inside its anonymous namespace, after
// decode_batched.inc.h).  Reference predictor.py:295-331; the rule is decode_kernel<R, 0, 0, true>'s, restated so that
// no column walks the whole vocabulary:
//
//   sample_row            one 256-thread workgroup, one row: softmax(x / T) in fp32, the top-k mask from a RADIX SELECTION
//                         of the k-th largest probability (four 8-bit digits of the bit pattern, a 256-bin count each),
//                         the top-p mask from a BITONIC SORT of (bit pattern, index) keys and a scan of the sorted
//                         masses, the draw from a scan of the final distribution in index order.
//   sample_batched_kernel<Rule>  the last launch of a step of i2l_sample_decode_batched, in select_batched_kernel's place;
//                         <Rule, true> also keeps the row's sequence score (i2l_sample_decode_multi).
//   sample_logits_kernel<Rule>   the same row function over a caller's logits (i2l_sample_logits).
// Rule is NoRule or ConstrainRule: the pick policy of decode_batched.inc.h, which sample_row takes as `allow`.
//
// Probabilities are >= 0, so their bit patterns order as the values do.  A key is (pattern << 32) | ~index: descending
// keys are descending values with the lower index first among equal ones, and no two keys are equal.  Every sum is a
// fixed tree (per-thread run, wave scan or butterfly, the four waves in order); the only atomics count integers in LDS.
// So a call is bitwise reproducible.  One workgroup per row, not one wave: at V = 500 a wave would hold 8 keys per lane
// and walk 45 compare-exchange rounds of 4 pairs each, the workgroup walks them with one pair per thread -- and this
// launch is on the serial chain of every step, where its latency counts, not its throughput.

constexpr int SB_MAXV = 8 * NT;          // 2048: i2l_sample_decode's limit

// the sampling arguments of every entry (i2l_sample_decode, i2l_sample_decode_batched, i2l_sample_logits); the
// comparisons are written so that a NaN is refused
inline bool sample_args_ok(float temperature, int top_k, float top_p) {
    return !(!(temperature > 0.f) || top_k < 0 || !(top_p >= 0.f) || (top_k == 0 && top_p == 0.f));
}

struct SampleRule {
    int top_k;
    float top_p;
    unsigned long long seed;
    float* probs;        // (B, T, V) or null
    double* score;       // [B] sequence log-probability (sample_batched_kernel<Rule, true> only), or null
};

struct SampleLds {
    unsigned long long key[SB_MAXV];     // sort keys
    float q[SB_MAXV];                    // scaled logits, then the distribution
    unsigned hist[NT];                   // digit counts of the radix selection
    float redv[NT / 64];
    int redi[NT / 64];
    unsigned sel[2];                     // selected digit, rank left inside it
};

// Exclusive scan over the workgroup in thread order; *total gets the sum.  Fixed order: the wave's lanes by doubling
// steps, then the waves one after the other.  Two __syncthreads().
__device__ __forceinline__ float block_scan_excl(float v, float* red, int tid, float* total) {
    const int lane = tid & 63, wave = tid >> 6;
    float incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    float base = 0.f, run = 0.f;
#pragma unroll
    for (int wv = 0; wv < NT / 64; ++wv) {
        if (wv == wave) base = run;
        run += red[wv];
    }
    __syncthreads();
    *total = run;
    return base + excl;
}

__device__ __forceinline__ unsigned block_scan_incl_u32(unsigned v, unsigned* red, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    if (lane == 63) red[wave] = v;
    __syncthreads();
    unsigned base = 0;
#pragma unroll
    for (int wv = 0; wv < NT / 64; ++wv)
        if (wv < wave) base += red[wv];
    __syncthreads();
    return base + v;
}

// smallest of the workgroup's values (every thread gets it); two __syncthreads()
__device__ __forceinline__ int block_min(int v, int* red, int tid) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    int m = red[0];
#pragma unroll
    for (int wv = 1; wv < NT / 64; ++wv) m = min(m, red[wv]);
    __syncthreads();
    return m;
}

// The kk-th largest (1 <= kk <= V) of q[0, V), q >= 0: most significant digit first, the digit's bin is the one in which
// the count of larger values passes kk.  Thread tid looks after bin 255 - tid, so that a scan in thread order runs from
// the largest digit down.
__device__ __forceinline__ float radix_kth(SampleLds& s, int V, int kk, int tid) {
    unsigned prefix = 0, mask = 0, need = (unsigned)kk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        s.hist[tid] = 0;
        __syncthreads();
        for (int v = tid; v < V; v += NT) {
            const unsigned b = __float_as_uint(s.q[v]);
            if ((b & mask) == prefix) atomicAdd(&s.hist[(b >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned bin = 255u - (unsigned)tid, c = s.hist[bin];
        const unsigned incl = block_scan_incl_u32(c, reinterpret_cast<unsigned*>(s.redi), tid);   // values in bins >= bin
        if (incl - c < need && need <= incl) { s.sel[0] = bin; s.sel[1] = need - (incl - c); }     // one thread
        __syncthreads();
        prefix |= s.sel[0] << shift;
        mask |= 255u << shift;
        need = s.sel[1];
    }
    return __uint_as_float(prefix);
}

// s.key[0, N) into descending order, N a power of two >= NT.  One compare-exchange per pair and round.  (Rounds of
// distance <= 64 stay inside one wave's 128 keys and could do without the workgroup barrier; measured at the shipped
// shape that gains nothing -- 19.0 against 18.7 us a launch -- so every round ends in the plain barrier.)
__device__ __forceinline__ void bitonic_desc(unsigned long long* key, int N, int tid) {
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (N >> 1); i += NT) {
                const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), b = a | j;
                const unsigned long long ka = key[a], kb = key[b];
                if ((ka < kb) == ((a & k) == 0)) { key[a] = kb; key[b] = ka; }
            }
            __syncthreads();
        }
    }
}

// One row: x[0, V) raw logits, u the row's uniform of this step.  Every thread returns the pick; po (V floats or null)
// receives the final distribution.  V <= SB_MAXV, blockDim.x == NT.  A column v with !allow(v) enters as -INFINITY: its
// probability is exactly 0 and the others renormalise (decode_constrained.inc.h); the result is 0x7fffffff or a
// disallowed column only when no allowed column holds a finite logit.  lse (two floats of the caller's, or null) receives
// the maximum and the sum of exp(. - maximum) of the scaled logits over the allowed columns, as the softmax took them.
template <class Allow>
__device__ __forceinline__ int sample_row(const float* __restrict__ x, int V, float temperature, int use_temp, int top_k,
                                          float top_p, float u, float* __restrict__ po, SampleLds& s, int tid,
                                          const Allow& allow, float* lse = nullptr) {
    float best[1] = {-INFINITY};
    int besti[1] = {0x7fffffff};
    for (int v = tid; v < V; v += NT) {
        float a = x[v];
        if (use_temp) a = a / temperature;
        if (!allow(v)) a = -INFINITY;
        s.q[v] = a;
        if (a > best[0]) { best[0] = a; besti[0] = v; }
    }
    block_argmax<1>(best, besti, s.redv, s.redi, tid);
    float sm = 0.f;
    for (int v = tid; v < V; v += NT) sm += expf(s.q[v] - best[0]);
    sm = block_sum(sm, s.redv, tid);
    if (lse) { lse[0] = best[0]; lse[1] = sm; }
    for (int v = tid; v < V; v += NT) s.q[v] = expf(s.q[v] - best[0]) / sm;
    __syncthreads();
    if (top_k > 0) {
        const float kth = radix_kth(s, V, min(top_k, V), tid);
        float s2 = 0.f;
        for (int v = tid; v < V; v += NT) { const float q = s.q[v] < kth ? 0.f : s.q[v]; s.q[v] = q; s2 += q; }
        s2 = block_sum(s2, s.redv, tid);
        if (s2 > 0.f) for (int v = tid; v < V; v += NT) s.q[v] = s.q[v] / s2;
        __syncthreads();
    }
    if (top_p > 0.f) {
        int N = NT;
        while (N < V) N <<= 1;
        for (int v = tid; v < N; v += NT)       // padding: value 0 behind every column
            s.key[v] = ((unsigned long long)(v < V ? __float_as_uint(s.q[v]) : 0u) << 32) | (unsigned)~v;
        __syncthreads();
        bitonic_desc(s.key, N, tid);
        const int CH = N / NT;                  // thread tid owns sorted places [tid * CH, (tid + 1) * CH)
        float part = 0.f;
        for (int j = tid * CH; j < (tid + 1) * CH; ++j) part += __uint_as_float((unsigned)(s.key[j] >> 32));
        float total;
        float before = block_scan_excl(part, s.redv, tid, &total);   // mass sorted ahead of the place
        for (int j = tid * CH; j < (tid + 1) * CH; ++j) {
            const unsigned long long kj = s.key[j];
            const int v = (int)~(unsigned)kj;
            const float pv = __uint_as_float((unsigned)(kj >> 32));
            if (v < V) s.q[v] = before > top_p ? 0.f : pv;           // the first place has nothing ahead of it: it stays
            before += pv;
        }
        __syncthreads();
        float s2 = 0.f;
        for (int v = tid; v < V; v += NT) s2 += s.q[v];
        s2 = block_sum(s2, s.redv, tid);
        if (s2 > 0.f) for (int v = tid; v < V; v += NT) s.q[v] = s.q[v] / s2;
        __syncthreads();
    }
    if (po)
        for (int v = tid; v < V; v += NT) po[v] = s.q[v];
    // inverse CDF over index order: thread tid owns the columns [tid * CH, (tid + 1) * CH)
    const int CH = (V + NT - 1) / NT, v0 = min(V, tid * CH), v1 = min(V, (tid + 1) * CH);
    float part = 0.f;
    for (int v = v0; v < v1; ++v) part += s.q[v];
    float total;
    float run = block_scan_excl(part, s.redv, tid, &total);
    const float target = u * total;
    int pick = 0x7fffffff;
    for (int v = v0; v < v1; ++v) {
        const float q = s.q[v];
        run += q;
        if (q > 0.f && run > target && pick == 0x7fffffff) pick = v;
    }
    pick = block_min(pick, s.redi, tid);        // the cdf does not fall: the first crossing is the smallest one
    return pick < V ? pick : besti[0];          // rounding corner: fall back to the arg max
}

// Token selection of step t by sampling, one workgroup per row, under NoRule or ConstrainRule.  ids, next token, finished
// rows and the live-row count as select_batched_kernel.
//
// Score (i2l_sample_decode_multi): a row that has not finished adds the log-probability of the token it commits to
// r.score[row] -- beam_topk_row's convention and formula, (x[pick] - m) - logf(sum expf(x - m)) in fp32 over the RAW
// logits of the columns the policy allows, so that a sample and a beam hypothesis of the same tokens carry comparable
// scores.  No temperature, no truncation; a pick the policy does not allow is the constraint's fallback and adds 0.
// At temperature 1 m and the sum are the ones sample_row's softmax has just taken (the same terms, summed by its tree);
// otherwise wave 0 takes them from the raw logits in beam_topk_row's lane order.  Thread 0 reads the row's finished
// mark and its score before sample_row, so that only the store is left behind the pick.  A template parameter, so that
// <Rule, false> is the kernel as it was.
template <class Rule, bool Score = false>
__global__ __launch_bounds__(NT) void sample_batched_kernel(BatchedParams p, SampleRule r, Rule c, int t) {
    __shared__ SampleLds s;
    if (*p.live == 0) return;
    const int V = p.w.V, row = blockIdx.x, tid = threadIdx.x;
    const auto al = c.row(row, V, p.end_id, p.T - t - 1);
    float* po = r.probs ? r.probs + ((size_t)row * p.T + t) * V : nullptr;
    [[maybe_unused]] int scoring = 0;
    [[maybe_unused]] double acc = 0.0;
    [[maybe_unused]] float lse[2] = {0.f, 1.f};
    if constexpr (Score) {
        scoring = !p.fin[row];                  // thread 0 commits behind the pick, so this is still the last step's
        if (tid == 0) acc = r.score[row];
    }
    const int pick = sample_row(p.lg + (size_t)row * p.w.Vp, V, p.temperature, p.use_temp, r.top_k, r.top_p,
                                uniform01(r.seed, (unsigned)row, (unsigned)t), po, s, tid, al, Score ? lse : nullptr);
    if constexpr (Score) {
        if (scoring && tid < 64) {              // wave 0
            const float* x = p.lg + (size_t)row * p.w.Vp;
            if (p.use_temp) {
                float m = -INFINITY;
                for (int v = tid; v < V; v += 64)
                    if (al(v)) m = fmaxf(m, x[v]);
                m = wave_max(m);
                float sum = 0.f;
                for (int v = tid; v < V; v += 64)
                    if (al(v)) sum += expf(x[v] - m);
                lse[0] = m;
                lse[1] = wave_sum(sum);
            }
            if (tid == 0 && pick >= 0 && pick < V && al(pick)) r.score[row] = acc + (double)((x[pick] - lse[0]) - logf(lse[1]));
        }
    }
    // every thread took its copy of the policy before the first barrier of sample_row; thread 0 stores behind the last one
    if (tid == 0) commit_token_batched(p, row, t, al.finish_sample(V, pick));
}

// i2l_sample_logits, and under ConstrainRule the sampling branch of i2l_constrained_pick_logits: the rule applied once
// to (rows, ld) logits of the caller, one workgroup per row.  end_id and rem are the constraint's (NoRule reads neither).
template <class Rule>
__global__ __launch_bounds__(NT) void sample_logits_kernel(const float* __restrict__ logits, int ld, int V, float temperature,
                                                           int use_temp, SampleRule r, unsigned step, Rule c, int end_id,
                                                           int rem, int32_t* __restrict__ ids) {
    __shared__ SampleLds s;
    const int row = blockIdx.x, tid = threadIdx.x;
    const auto al = c.row(row, V, end_id, rem);
    if (uint8_t* mask = al.mask())
        for (int v = tid; v < V; v += NT) mask[v] = al(v) ? 1 : 0;
    float* po = r.probs ? r.probs + (size_t)row * V : nullptr;
    const int pick = sample_row(logits + (size_t)row * ld, V, temperature, use_temp, r.top_k, r.top_p,
                                uniform01(r.seed, (unsigned)row, step), po, s, tid, al);
    if (tid == 0) ids[row] = al.finish_sample(V, pick);
}
