// The consensus decode's rules (sample_rank_rules.inc.h) as a stand-alone host program, so that crafted token rows and
// exact score and risk ties can be fed to them under the host sanitizers (-fsanitize=address,undefined) in a process
// of its own.  It holds no rule: cut every sample, fill the distance table, sum the risks, take the keys, order.
//
//   sample_rank_host_main CASES OUT
//
// CASES: "SRNK", int32 count, then per case (one image) int32 samples, steps, end_id, rank, has_norm; float64
// norm[steps + 1] when has_norm; int32 ids[samples][steps]; float64 score[samples].
// OUT per case: int32 len[samples], finished[samples], risk[samples]; float64 key[samples]; int32 order[samples];
// int32 dist[samples][samples].
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "sample_rank_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "SRNK", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[5];
        if (!get(in, head, sizeof head)) return 2;
        const int S = head[0], T = head[1], end_id = head[2], rank = head[3];
        if (S < 1 || S > SR_MAX_SAMPLES || T < 1 || T > SR_MAX_STEPS) return 2;
        if (rank != SR_RANK_CONSENSUS && rank != SR_RANK_LOGPROB) return 2;
        std::vector<double> norm(head[4] ? (size_t)T + 1 : 0), score((size_t)S), key((size_t)S);
        std::vector<int32_t> ids((size_t)S * T), len((size_t)S), fin((size_t)S), order((size_t)S), dist((size_t)S * S);
        std::vector<int> risk((size_t)S), n((size_t)S);
        if (!get(in, norm.data(), norm.size() * sizeof(double)) || !get(in, ids.data(), ids.size() * 4) ||
            !get(in, score.data(), score.size() * sizeof(double)))
            return 2;
        for (int s = 0; s < S; ++s) {
            const SrCut c = sr_cut(ids.data() + (size_t)s * T, T, end_id);
            n[s] = c.n; len[s] = c.len; fin[s] = c.finished;
        }
        for (int i = 0; i < S; ++i) {
            risk[i] = 0;
            for (int j = 0; j < S; ++j) {
                std::vector<int> row((size_t)n[j] + 1);
                const int d = sr_distance(ids.data() + (size_t)i * T, n[i], ids.data() + (size_t)j * T, n[j], row.data());
                dist[(size_t)i * S + j] = d;
                risk[i] += d;
            }
        }
        for (int s = 0; s < S; ++s) key[s] = sr_key(rank, risk[s], score[s], len[s], head[4] ? norm.data() : nullptr);
        sr_order(rank, S, risk.data(), score.data(), key.data(), order.data());
        std::vector<int32_t> risk32(risk.begin(), risk.end());
        fwrite(len.data(), 4, len.size(), out);
        fwrite(fin.data(), 4, fin.size(), out);
        fwrite(risk32.data(), 4, risk32.size(), out);
        fwrite(key.data(), 8, key.size(), out);
        fwrite(order.data(), 4, order.size(), out);
        fwrite(dist.data(), 4, dist.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
