// N-best step-batched beam search with length-normalised ranking (included by decode.hip inside its anonymous namespace,
// after beam_batched.inc.h).  The search is i2l_beam_decode_batched's: the same GEMM launches, the same phases (c), (d),
// (e) per step (beam_step_batched_kernel<K, true>: one source text, the ending apart), the same parity scheme and
// early-end word.  Only what happens to `completed` differs:
//
//   <K, false>   reduces `completed` to its best raw score (bb_retire, the all-ended branch)
//   <K, true>    nb_step_end: every retiring beam is inserted as (key, score, t, q) into a per-image list of at most N
//                entries in the scratch (BeamImage.has_c counts them), sorted by key = score / norm[n], n = the beam's
//                tokens after START, END included.
//
// A new entry goes in front of the first entry whose key is STRICTLY smaller and the last entry drops on overflow.  Beams
// retire in step order, then slot order, so this streaming insertion is the stable descending sort of the whole
// `completed` list cut to N.  With N = 1 and norm all ones it keeps max(completed), first on ties: bb_retire's rule.
//
// norm is the caller's table of T + 1 fp64 values (null: all ones); the kernel only divides, and fp64 division is
// correctly rounded, so the host computes the same keys.
//
// beam_nbest_final_kernel, one thread per (image, row): rows below the list's count are backtracked from their (t, q);
// an image that was still searching after the last step (neither `break` fired) fills further rows from its final slots
// in slot order -- all of them have n = T, and x / norm[T] is monotone in x, so slot order (raw score, descending,
// stable) is their stable key order.  Such a row is finished when its last token is END: the reference never retires a
// beam that ends at the very last step.

struct NbestEntry {
    double key, score;
    int t, q;            // history row and slot of the last token; t = -1: the empty sequence (START == END)
};

struct BeamNbestOut {
    int32_t* seq_out;        // [images][N][T + 1]
    int32_t* len_out;        // [images][N]
    double* score_out;       // [images][N]
    double* key_out;         // [images][N] or null
    int32_t* finished_out;   // [images][N] or null
    int32_t* count_out;      // [images]
};

__device__ __forceinline__ double nb_key(const double* norm, double score, int n) { return norm ? score / norm[n] : score; }

// one thread
__device__ __forceinline__ void nb_insert(NbestEntry* list, int& cnt, int N, double key, double score, int t, int q) {
    int pos = cnt;
    while (pos > 0 && list[pos - 1].key < key) --pos;
    if (pos >= N) return;
    const int last = cnt < N ? cnt : N - 1;
    for (int i = last; i > pos; --i) list[i] = list[i - 1];
    NbestEntry& e = list[pos];
    e.key = key; e.score = score; e.t = t; e.q = q;
    if (cnt < N) ++cnt;
}

// The ending of step t in beam_step_batched_kernel<K, true>, where the parent keeps the best completed beam: all ended
// -- completed.extend(beams); break (:282-284), n = t + 1 tokens; else (a) of step t + 1 as bb_retire, the retiring
// slots (n = t + 1 as well: their last token is step t's) going into the list in slot order.  One thread.
template <int K>
__device__ __forceinline__ void nb_step_end(const BeamBatchedParams& p, BeamImage& rec, const int* ntok, const double* nscore,
                                            int* slot_live, bool all_end, int img, int t) {
    NbestEntry* list = p.list + (size_t)img * p.N;
    int cnt = rec.has_c;                                 // here the number of list entries
    if (all_end) {
        for (int q = 0; q < rec.nb; ++q) nb_insert(list, cnt, p.N, nb_key(p.norm, nscore[q], t + 1), nscore[q], t, q);
        rec.done = 1;
    } else if (t + 1 < p.T) {
        int nl = 0;
        for (int q = 0; q < K; ++q) {
            int lv = 0;
            if (q < rec.nb) {
                if (ntok[q] == p.end_id) nb_insert(list, cnt, p.N, nb_key(p.norm, nscore[q], t + 1), nscore[q], t, q);
                else { lv = 1; ++nl; }
            }
            slot_live[q] = lv;
        }
        if (nl == 0) rec.done = 1;
    }
    rec.has_c = cnt;
}

// after beam_init_batched_kernel, which leaves has_c = 0 entries, or 1 for START == END, where [START] retires at once
// (n = 0): that entry
__global__ __launch_bounds__(DB_NT) void beam_nbest_init_kernel(BeamBatchedParams p) {
    const int img = blockIdx.x * DB_NT + threadIdx.x;
    if (img >= p.images || p.start_id != p.end_id) return;
    NbestEntry& e = p.list[(size_t)img * p.N];
    e.key = nb_key(p.norm, 0.0, 0); e.score = 0.0; e.t = -1; e.q = 0;
}

// rows of the result; grid covers images * N threads
__global__ __launch_bounds__(DB_NT) void beam_nbest_final_kernel(BeamBatchedParams p, BeamNbestOut o, int K) {
    const int N = p.N;
    const size_t id = (size_t)blockIdx.x * DB_NT + threadIdx.x;
    if (id >= (size_t)p.images * N) return;
    const int img = (int)(id / N), row = (int)(id - (size_t)img * N);
    const BeamImage im = p.img[img];
    const int T = p.T, cnt = im.has_c;
    const int left = im.done ? 0 : im.nb;                // the final beams of a loop that ran out of steps
    const int count = cnt + left < N ? cnt + left : N;
    if (row == 0) o.count_out[img] = count;
    int32_t* out = o.seq_out + id * (T + 1);
    int tt = -1, q = 0, fin = 0, len = -1;
    double sc = -INFINITY, key = -INFINITY;
    if (row < cnt) {
        const NbestEntry e = p.list[(size_t)img * N + row];
        tt = e.t; q = e.q; sc = e.score; key = e.key; fin = 1;
    } else if (row < count) {
        q = row - cnt;
        tt = im.t_last;
        sc = p.score[(size_t)img * K + q];
        key = nb_key(p.norm, sc, tt + 1);
        fin = p.last[(size_t)img * K + q] == p.end_id;
    }
    if (row < count) {
        const int32_t* tokhist = p.tokhist + (size_t)img * T * K;
        const int32_t* parhist = p.parhist + (size_t)img * T * K;
        const int n = tt + 1;                            // tokens after START
        for (int pos = tt; pos >= 0; --pos) {
            out[pos] = tokhist[(size_t)pos * K + q];
            q = parhist[(size_t)pos * K + q];
        }
        len = n;
        for (int i = 0; i < n; ++i)
            if (out[i] == p.end_id) { len = i; break; }
    }
    for (int i = len < 0 ? 0 : len; i < T + 1; ++i) out[i] = -1;
    o.len_out[id] = len;
    o.score_out[id] = sc;
    if (o.key_out) o.key_out[id] = key;
    if (o.finished_out) o.finished_out[id] = fin;
}

struct BeamNbestLayout {
    BeamBatchedLayout b;
    size_t list, total;
};

BeamNbestLayout beam_nbest_layout(int images, int K, int N, int Vp, int H, int L, int steps) {
    BeamNbestLayout o{};
    o.b = beam_batched_layout(images, K, Vp, H, L, steps);
    size_t off = o.b.total;                              // 256-aligned; the entries are packed, so every row counts
    o.list = off; off += (size_t)images * N * sizeof(NbestEntry);
    o.total = off;
    return o;
}

// nbest is independent of the beam width: `completed` grows by up to K entries per step
inline bool beam_nbest_dims_ok(int images, int beam, int nbest, int V, int H, int L, int steps) {
    return nbest >= 1 && nbest <= I2L_MAX_NBEST && beam_batched_dims_ok(images, beam, V, H, L, steps);
}
