// The beam search's serial rules (beam_rules.inc.h) as a stand-alone host program, so that exact score ties -- which real
// logits almost never produce -- can be fed to them, under the host sanitizers (-fsanitize=address,undefined) in a
// process of its own.  It holds no rule: the loop `for t: rank; step end`, then the results.
//
//   beam_rules_host_main CASES OUT
//
// CASES: "BEAM", int32 count, then per case int32 K, T, N, start_id, end_id, has_norm; float64 norm[T + 1] when
// has_norm; and per step t and slot s the K (float32 logp, int32 token) pairs phase (c) would have produced, descending:
// a "model" whose top K depends on (step, slot) alone.
// OUT per case: the best-completed search: int32 len, float64 score, int32 seq[T + 1]; then the N-best search: int32
// count and N rows of int32 len, int32 finished, float64 score, float64 key, int32 seq[T + 1].
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "beam_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Case {
    int K, T, start_id, end_id;
    std::vector<float> logp;      // [T][K][K]
    std::vector<int> token;       // [T][K][K]
};

// the slots and histories of one search
struct Search {
    BeamImage im;
    std::vector<double> score, nscore;
    std::vector<int> last, live, npar, ntok;
    std::vector<int32_t> tokhist, parhist;

    template <class Sink>
    Search(const Case& c, const Sink& completed)
        : score(c.K), nscore(c.K), last(c.K), live(c.K), npar(c.K), ntok(c.K), tokhist((size_t)c.T * c.K),
          parhist((size_t)c.T * c.K) {
        const int K = c.K;
        beam_start(im, completed, score.data(), last.data(), live.data(), K, c.start_id, c.end_id);
        for (int t = 0; t < c.T && !im.done; ++t) {
            const size_t at = (size_t)t * K * K;
            const int nnew = beam_rank(live.data(), score.data(), c.logp.data() + at, c.token.data() + at, K, nullptr, npar.data(),
                                       ntok.data(), nscore.data(), tokhist.data() + (size_t)t * K, parhist.data() + (size_t)t * K);
            beam_step_end(im, completed, nnew, ntok.data(), nscore.data(), score.data(), last.data(), live.data(), K,
                          c.end_id, t, c.T);
        }
    }
};

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "BEAM", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[6];
        if (!get(in, head, sizeof head)) return 2;
        Case c{head[0], head[1], head[3], head[4], {}, {}};
        const int K = c.K, T = c.T, N = head[2];
        if (K < 1 || K > 8 || T < 1 || T > 4096 || N < 1 || N > 4096) return 2;
        std::vector<double> norm(head[5] ? (size_t)T + 1 : 0);
        if (!get(in, norm.data(), norm.size() * sizeof(double))) return 2;
        const size_t pairs = (size_t)T * K * K;
        c.logp.resize(pairs);
        c.token.resize(pairs);
        for (size_t i = 0; i < pairs; ++i)
            if (!get(in, &c.logp[i], 4) || !get(in, &c.token[i], 4)) return 2;
        std::vector<int32_t> seq((size_t)T + 1);

        const Search best(c, BeamBest{});
        double score = 0.0;
        const int32_t len = beam_best_result(best.im, best.score.data(), best.tokhist.data(), best.parhist.data(), K, c.end_id,
                                             T, seq.data(), &score);
        fwrite(&len, 4, 1, out);
        fwrite(&score, 8, 1, out);
        fwrite(seq.data(), 4, seq.size(), out);

        std::vector<NbestEntry> list((size_t)N);
        const BeamList sink{list.data(), N, head[5] ? norm.data() : nullptr};
        const Search all(c, sink);
        const int32_t rows = beam_list_count(all.im, N);
        fwrite(&rows, 4, 1, out);
        for (int row = 0; row < N; ++row) {
            const NbestRow r = beam_list_row(all.im, sink, row, all.score.data(), all.last.data(), all.tokhist.data(),
                                             all.parhist.data(), K, c.end_id, T, seq.data());
            const int32_t lf[2] = {r.len, r.finished};
            const double sk[2] = {r.score, r.key};
            fwrite(lf, 4, 2, out);
            fwrite(sk, 8, 2, out);
            fwrite(seq.data(), 4, seq.size(), out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
