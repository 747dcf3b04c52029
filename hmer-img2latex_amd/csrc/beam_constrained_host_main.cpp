// The well-formed beam search's rules (beam_bracket_rules.inc.h on top of beam_rules.inc.h and bracket_rules.inc.h) as a
// stand-alone host program, so that a host test can run WHOLE constrained searches -- exact score ties, depth 32, slots
// with fewer than K candidates, broken tables -- under the host sanitizers (-fsanitize=address,undefined) in a process of
// its own.  It holds no rule: the loop `for t: candidates of every live slot; rank; inherit; step end`, then the rows.
//
//   beam_constrained_host_main CASES OUT
//
// CASES is one of two files.
//
// "BMCN", int32 count, then per case int32 V, K, T, N, start_id, end_id, has_norm; float64 norm[T + 1] when has_norm;
// uint8 cls[V]; float32 lp[T][V][V]: a "model" whose row of log-probs at step t depends on the slot's last token alone,
// taken as it is (no softmax: the renormalisation is the device's).
// OUT per case: per step run int32 t, int32 nnew, then per slot q < K int32 token, int32 parent, float64 score, int32
// candidates (0: not live) and the 16 bytes of its state after the step (zeros for q >= nnew); int32 -1; then int32 count
// and N rows of int32 len, int32 finished, float64 score, float64 key, int32 seq[T + 1].
//
// "BEAM": the case file of beam_rules_host_main.  Every N-best search is run twice, beam_rank with null counts and with
// counts all K, and OUT holds both results per case in beam_rules_host_main's N-best layout: they must be the same bytes.
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "beam_bracket_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static void put_rows(FILE* out, const BeamImage& im, const BeamList& sink, const std::vector<double>& score,
                     const std::vector<int>& last, const std::vector<int32_t>& tokhist, const std::vector<int32_t>& parhist,
                     int K, int end_id, int T) {
    std::vector<int32_t> seq((size_t)T + 1);
    const int32_t rows = beam_list_count(im, sink.N);
    fwrite(&rows, 4, 1, out);
    for (int row = 0; row < sink.N; ++row) {
        const NbestRow r = beam_list_row(im, sink, row, score.data(), last.data(), tokhist.data(), parhist.data(), K, end_id,
                                         T, seq.data());
        const int32_t lf[2] = {r.len, r.finished};
        const double sk[2] = {r.score, r.key};
        fwrite(lf, 4, 2, out);
        fwrite(sk, 8, 2, out);
        fwrite(seq.data(), 4, seq.size(), out);
    }
}

// one well-formed search, traced step by step
static bool constrained_case(FILE* in, FILE* out) {
    int32_t head[7];
    if (!get(in, head, sizeof head)) return false;
    const int V = head[0], K = head[1], T = head[2], N = head[3], start_id = head[4], end_id = head[5];
    if (V < 1 || V > 4096 || K < 1 || K > 8 || T < 1 || T > 4096 || N < 1 || N > 4096 || end_id < 0 || end_id >= V ||
        start_id < 0 || start_id >= V)
        return false;
    std::vector<double> norm(head[6] ? (size_t)T + 1 : 0);
    std::vector<uint8_t> cls((size_t)V);
    std::vector<float> lp((size_t)T * V * V);
    if (!get(in, norm.data(), norm.size() * sizeof(double)) || !get(in, cls.data(), cls.size()) ||
        !get(in, lp.data(), lp.size() * sizeof(float)))
        return false;

    std::vector<NbestEntry> list((size_t)N);
    const BeamList sink{list.data(), N, head[6] ? norm.data() : nullptr};
    BeamImage im;
    std::vector<double> score(K), nscore(K);
    std::vector<int> last(K), live(K), npar(K), ntok(K), ncand(K), topi((size_t)K * K);
    std::vector<float> topv((size_t)K * K);
    std::vector<int32_t> tokhist((size_t)T * K), parhist((size_t)T * K);
    std::vector<BracketState> state(K), parents(K);

    beam_start(im, sink, score.data(), last.data(), live.data(), K, start_id, end_id);
    for (int t = 0; t < T && !im.done; ++t) {
        parents = state;                                     // the copy taken before any slot is overwritten
        for (int s = 0; s < K; ++s) {
            ncand[s] = 0;
            if (live[s])
                ncand[s] = bb_candidates(parents[s], lp.data() + ((size_t)t * V + last[s]) * V, cls.data(), V, K, end_id, T, t,
                                         topv.data() + (size_t)s * K, topi.data() + (size_t)s * K);
        }
        const int32_t nnew = beam_rank(live.data(), score.data(), topv.data(), topi.data(), K, ncand.data(), npar.data(),
                                       ntok.data(), nscore.data(), tokhist.data() + (size_t)t * K, parhist.data() + (size_t)t * K);
        for (int q = 0; q < K; ++q)
            state[q] = q < nnew ? bb_inherit(parents.data(), npar[q], ntok[q], end_id, cls.data()) : BracketState{};
        const int32_t t32 = t;
        fwrite(&t32, 4, 1, out);
        fwrite(&nnew, 4, 1, out);
        for (int q = 0; q < K; ++q) {
            const int32_t tp[2] = {ntok[q], npar[q]};
            const int32_t nc = ncand[q];
            fwrite(tp, 4, 2, out);
            fwrite(&nscore[q], 8, 1, out);
            fwrite(&nc, 4, 1, out);
            fwrite(&state[q], sizeof(BracketState), 1, out);
        }
        beam_step_end(im, sink, nnew, ntok.data(), nscore.data(), score.data(), last.data(), live.data(), K, end_id, t, T);
    }
    const int32_t stop = -1;
    fwrite(&stop, 4, 1, out);
    put_rows(out, im, sink, score, last, tokhist, parhist, K, end_id, T);
    return true;
}

// one case of beam_rules_host_main: the N-best search under null counts, then under counts all K
static bool plain_case(FILE* in, FILE* out) {
    int32_t head[6];
    if (!get(in, head, sizeof head)) return false;
    const int K = head[0], T = head[1], N = head[2], start_id = head[3], end_id = head[4];
    if (K < 1 || K > 8 || T < 1 || T > 4096 || N < 1 || N > 4096) return false;
    std::vector<double> norm(head[5] ? (size_t)T + 1 : 0);
    if (!get(in, norm.data(), norm.size() * sizeof(double))) return false;
    const size_t pairs = (size_t)T * K * K;
    std::vector<float> logp(pairs);
    std::vector<int> token(pairs);
    for (size_t i = 0; i < pairs; ++i)
        if (!get(in, &logp[i], 4) || !get(in, &token[i], 4)) return false;
    const std::vector<int> all_k((size_t)K, K);
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<NbestEntry> list((size_t)N);
        const BeamList sink{list.data(), N, head[5] ? norm.data() : nullptr};
        BeamImage im;
        std::vector<double> score(K), nscore(K);
        std::vector<int> last(K), live(K), npar(K), ntok(K);
        std::vector<int32_t> tokhist((size_t)T * K), parhist((size_t)T * K);
        beam_start(im, sink, score.data(), last.data(), live.data(), K, start_id, end_id);
        for (int t = 0; t < T && !im.done; ++t) {
            const size_t at = (size_t)t * K * K;
            const int nnew = beam_rank(live.data(), score.data(), logp.data() + at, token.data() + at, K,
                                       pass ? all_k.data() : nullptr, npar.data(), ntok.data(), nscore.data(),
                                       tokhist.data() + (size_t)t * K, parhist.data() + (size_t)t * K);
            beam_step_end(im, sink, nnew, ntok.data(), nscore.data(), score.data(), last.data(), live.data(), K, end_id, t, T);
        }
        put_rows(out, im, sink, score, last, tokhist, parhist, K, end_id, T);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || !get(in, &count, 4) || count < 0) return 2;
    const bool constrained = memcmp(magic, "BMCN", 4) == 0;
    if (!constrained && memcmp(magic, "BEAM", 4) != 0) return 2;
    for (int32_t k = 0; k < count; ++k)
        if (!(constrained ? constrained_case(in, out) : plain_case(in, out))) return 2;
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
