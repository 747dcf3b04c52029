// N-best step-batched beam search with length-normalised ranking (included by decode.hip inside its anonymous namespace,
// after beam_batched.inc.h).  The search is i2l_beam_decode_batched's: the same GEMM launches, the same kernel text per
// step (beam_step_batched_kernel<K, true>), the same parity scheme and early-end word.  Only the "completed" sink of
// the rules differs (beam_rules.inc.h): BeamList in BeamBest's place, so every retiring beam is inserted as (key, score,
// t, q) into a per-image list of at most N entries in the scratch (BeamImage.has_c counts them), sorted by key = score /
// norm[n], n = the beam's tokens after START, END included.  With N = 1 and norm all ones that is BeamBest's rule.
//
// norm is the caller's table of T + 1 fp64 values (null: all ones); the rules only divide, and fp64 division is
// correctly rounded, so the host computes the same keys.
//
// What is specific to the list is here: its place in the scratch, the entry of the empty sequence, the rows of the result
// (beam_list_row, one thread per (image, row)) and the dimension check.

struct BeamNbestOut {
    int32_t* seq_out;        // [images][N][T + 1]
    int32_t* len_out;        // [images][N]
    double* score_out;       // [images][N]
    double* key_out;         // [images][N] or null
    int32_t* finished_out;   // [images][N] or null
    int32_t* count_out;      // [images]
};

// after beam_init_batched_kernel, which leaves has_c = 0 entries, or 1 for START == END, where [START] retires at once
// (n = 0): that entry
__global__ __launch_bounds__(DB_NT) void beam_nbest_init_kernel(BeamBatchedParams p) {
    const int img = blockIdx.x * DB_NT + threadIdx.x;
    if (img >= p.images || p.start_id != p.end_id) return;
    BeamImage none{};
    beam_sink<true>(p, img).put(none, 0.0, -1, 0);
}

// rows of the result; grid covers images * N threads.  Every output element is written.
__global__ __launch_bounds__(DB_NT) void beam_nbest_final_kernel(BeamBatchedParams p, BeamNbestOut o, int K) {
    const int N = p.N;
    const size_t id = (size_t)blockIdx.x * DB_NT + threadIdx.x;
    if (id >= (size_t)p.images * N) return;
    const int img = (int)(id / N), row = (int)(id - (size_t)img * N);
    const BeamImage im = p.img[img];
    const size_t hist = (size_t)img * p.T * K;
    if (row == 0) o.count_out[img] = beam_list_count(im, N);
    const NbestRow r = beam_list_row(im, beam_sink<true>(p, img), row, p.score + (size_t)img * K, p.last + (size_t)img * K,
                                     p.tokhist + hist, p.parhist + hist, K, p.end_id, p.T, o.seq_out + id * (p.T + 1));
    o.len_out[id] = r.len;
    o.score_out[id] = r.score;
    if (o.key_out) o.key_out[id] = r.key;
    if (o.finished_out) o.finished_out[id] = r.finished;
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
