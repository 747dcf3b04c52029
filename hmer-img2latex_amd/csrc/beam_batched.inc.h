// Step-batched beam search on the MATRIX CORES for decoders the grouped beam kernel does not take (the shipped 2 x 512
// one): the K slots of every image are rows of ONE batched step, R = images * K rows, row r = slot r % K of image r / K
// (included by decode.hip inside its anonymous namespace, after decode_batched.inc.h).  Reference seq2seq.py:234-298.
//
// Per step the host enqueues L launches of lstm_step_mfma_kernel<TB> and one of logits_mfma_kernel<TB> on the R rows
// (decode_batched.inc.h, unchanged but for the Genc row: a beam row reads the encoder half of its image, row / K), then
//
//   beam_step_batched_kernel<K>  one workgroup per image: phases (c), (d), (e) of beam_kernel<K> (decode.hip) and phase
//                                (a) of the NEXT step, with the search state in the scratch instead of LDS.
//
// The ranking rule of (c) / (d) is restated here from beam_kernel<K>, not shared with it: there the rows, scores and
// flags are LDS arrays of one workgroup that loops over the steps, here they are global arrays indexed per image and the
// step loop is the host's; the arithmetic and its order are the same.
//
// State hazards.  The GEMM launches read h[par] and write h[par ^ 1]; the gather (e) moves h[par ^ 1] of a slot's parent
// into h[par] of the slot, so every step runs at parity 0.  c is updated in place by the GEMM launches, and the slots of
// one image read each other's rows in the gather, so c has two buffers: step t updates c[t & 1] and gathers it into
// c[(t + 1) & 1], which the next step's launches get.  Rows of unused or retired slots and of finished images still ride
// through the GEMMs on a clamped token; no row reads another row there and nothing reads their results.
//
// Early end: one device word counts the images still searching; every launch of a later step reads it first and returns
// when it is 0.  All steps are always enqueued.  No polls, no cooperative launch, no exchange: nothing can time out.

struct BeamImage {       // per image: `completed` reduced to its best entry, the beam count, the end of the search
    double best_c;
    int has_c, best_t, best_q;   // (the N-best search keeps a list instead and counts its entries in has_c)
    int nb;              // beams in the slots 0 .. nb - 1
    int t_last;          // last history row written
    int done;
};

struct NbestEntry;        // beam_nbest.inc.h

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

// (a) of step `t` for one image: slots whose last token is END retire into the best-completed record, in slot order,
// strict > (seq2seq.py:258-260); the live flags; returns the live count.  One thread.
__device__ __forceinline__ int bb_retire(BeamImage& im, const int* last_q, const double* score_q, int* slot_live, int K,
                                         int end_id, int t) {
    int nl = 0;
    for (int q = 0; q < K; ++q) {
        int lv = 0;
        if (q < im.nb) {
            if (last_q[q] == end_id) {
                if (!im.has_c || score_q[q] > im.best_c) { im.has_c = 1; im.best_c = score_q[q]; im.best_t = t - 1; im.best_q = q; }
            } else { lv = 1; ++nl; }
        }
        slot_live[q] = lv;
    }
    return nl;
}

// zero state, slot 0 = START with score 0.0 and one beam, (a) of step 0 (START == END: the empty sequence)
__global__ __launch_bounds__(DB_NT) void beam_init_batched_kernel(BeamBatchedParams p, int K) {
    const size_t R = (size_t)p.images * K, LRH2 = 2 * (size_t)p.L * R * p.H;
    const size_t i0 = (size_t)blockIdx.x * DB_NT + threadIdx.x, stride = (size_t)gridDim.x * DB_NT;
    for (size_t i = i0; i < LRH2; i += stride) { p.h[i] = 0.f; p.c[i] = 0.f; }
    // (a) of step 0: the one beam [START] retires at once when START == END, and `if not candidates: break` (:276-277)
    const int ended = p.start_id == p.end_id;
    for (size_t i = i0; i < R; i += stride) {
        p.score[i] = 0.0;
        p.last[i] = p.start_id;
        p.slot_live[i] = (i % K == 0 && !ended) ? 1 : 0;
    }
    for (size_t i = i0; i < (size_t)p.images; i += stride) {
        BeamImage im{};
        im.nb = 1; im.best_t = -1; im.t_last = -1;
        im.has_c = ended; im.done = ended;
        p.img[i] = im;
    }
    if (i0 == 0) *p.live = ended ? 0u : (unsigned)p.images;
}

// The ending of a step of the N-best search (beam_nbest.inc.h): retiring beams go into the image's list.  One thread.
template <int K>
__device__ __forceinline__ void nb_step_end(const BeamBatchedParams& p, BeamImage& rec, const int* ntok, const double* nscore,
                                            int* slot_live, bool all_end, int img, int t);

// Ranking, gather and retirement of step t (after its logits launch).  grid images; c_cur: the buffer the step's LSTM
// launches updated, c_next: the one the next step's get.  NBEST: the same step with nb_step_end in place of the
// best-completed record (the kernel of i2l_beam_decode_nbest).
template <int K, bool NBEST = false>
__global__ __launch_bounds__(DB_NT) void beam_step_batched_kernel(BeamBatchedParams p, float* __restrict__ c_cur,
                                                                  float* __restrict__ c_next, int t) {
    __shared__ double nscore[K];
    __shared__ float topv[K * K];                        // [K][K] log-probs, descending
    __shared__ int topi[K * K];
    __shared__ int npar[K], ntok[K], ctl[1];
    __shared__ double oscore[K];                         // the slots' scores and live flags as the step found them: the
    __shared__ int olive[K];                             // serial ranking of (d) reads them K * K times over
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

    if (tid < K) { oscore[tid] = score[tid]; olive[tid] = slot_live[tid]; }

    // (c) log_softmax (fp32, :266) and top-K (:267: descending, lower index first on ties); wave per row
    for (int r = wave; r < K; r += DB_NT / 64) {
        if (!slot_live[r]) continue;                     // wave-uniform
        const float* x = p.lg + (r0 + r) * Vp;
        float m = -INFINITY;
        for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
        m = wave_max(m);
        float s = 0.f;
        for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
        s = wave_sum(s);
        const float lse = logf(s);
        unsigned taken = 0;                              // bit i: element lane + 64*i already selected (V <= 2048)
        for (int j = 0; j < K; ++j) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            for (int v = lane, i = 0; v < V; v += 64, ++i)
                if (!((taken >> i) & 1u) && x[v] > bv) { bv = x[v]; bi = v; }
            wave_argmax(bv, bi);
            if (bi < V && (bi & 63) == lane) taken |= 1u << (bi >> 6);
            if (lane == 0) { topv[r * K + j] = (bv - m) - lse; topi[r * K + j] = bi < V ? bi : 0; }
        }
    }
    __syncthreads();

    // (d) candidates in (slot, rank) order, fp64 scores, stable descending selection of K (:268-280)
    if (tid == 0) {
        int nlive = 0;
        for (int q = 0; q < K; ++q) nlive += olive[q];
        const int ncand = nlive * K;
        const int nnew = ncand < K ? ncand : K;
        unsigned long long used = 0ull;                  // K*K <= 64 candidate flags
        for (int q = 0; q < nnew; ++q) {
            double bs = 0.0;
            int bc = -1;
            for (int s0 = 0; s0 < K; ++s0) {
                if (!olive[s0]) continue;
                for (int j = 0; j < K; ++j) {
                    const int c = s0 * K + j;
                    if ((used >> c) & 1ull) continue;
                    const double sc = oscore[s0] + (double)topv[c];
                    if (bc < 0 || sc > bs) { bs = sc; bc = c; }
                }
            }
            used |= 1ull << bc;
            npar[q] = bc / K;
            ntok[q] = topi[bc];
            nscore[q] = bs;
            tokhist[(size_t)t * K + q] = topi[bc];
            parhist[(size_t)t * K + q] = bc / K;
        }
        for (int q = nnew; q < K; ++q) { npar[q] = 0; ntok[q] = 0; nscore[q] = 0.0; }
        ctl[0] = nnew;
    }
    __syncthreads();

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

    // new scores and last tokens; all ended: completed.extend(beams); break (:282-284); else (a) of step t + 1
    if (tid == 0) {
        BeamImage rec = *im;
        const int nb = ctl[0];
        bool all_end = true;
        for (int q = 0; q < K; ++q) {
            score[q] = nscore[q];
            p.last[r0 + q] = ntok[q];
            if (q < nb && ntok[q] != p.end_id) all_end = false;
        }
        rec.nb = nb;
        rec.t_last = t;
        if constexpr (NBEST) {
            nb_step_end<K>(p, rec, ntok, nscore, slot_live, all_end, img, t);
        } else if (all_end) {
            for (int q = 0; q < nb; ++q)
                if (!rec.has_c || nscore[q] > rec.best_c) { rec.has_c = 1; rec.best_c = nscore[q]; rec.best_t = t; rec.best_q = q; }
            rec.done = 1;
        } else if (t + 1 < T) {
            if (bb_retire(rec, ntok, nscore, slot_live, K, p.end_id, t + 1) == 0) rec.done = 1;
        }
        *im = rec;
        if (rec.done) atomicSub(p.live, 1u);
    }
}

// result: max(completed) (first on ties) else beams[0]; strip START, cut at END, pad with -1 (:286-297).  One thread per image.
__global__ __launch_bounds__(DB_NT) void beam_final_batched_kernel(BeamBatchedParams p, int K) {
    const int img = blockIdx.x * DB_NT + threadIdx.x;
    if (img >= p.images) return;
    const BeamImage im = p.img[img];
    const int T = p.T;
    const int32_t* tokhist = p.tokhist + (size_t)img * T * K;
    const int32_t* parhist = p.parhist + (size_t)img * T * K;
    int tt = im.has_c ? im.best_t : im.t_last, q = im.has_c ? im.best_q : 0;
    const double sc = im.has_c ? im.best_c : p.score[(size_t)img * K];
    int32_t* out = p.seq_out + (size_t)img * (T + 1);
    const int n = tt + 1;                                // tokens after START
    for (int pos = tt; pos >= 0; --pos) {
        out[pos] = tokhist[(size_t)pos * K + q];
        q = parhist[(size_t)pos * K + q];
    }
    int len = n;
    for (int i = 0; i < n; ++i)
        if (out[i] == p.end_id) { len = i; break; }
    for (int i = len; i < T + 1; ++i) out[i] = -1;
    p.len_out[img] = len;
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
