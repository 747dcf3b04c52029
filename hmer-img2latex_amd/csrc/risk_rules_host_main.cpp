// The rules of minimum-risk fine-tuning (risk_rules.inc.h) as a stand-alone host program, so that crafted draws -- an
// empty one, one without END, one equal to the gold formula, an empty gold formula, draws that are all equal -- can be fed
// to them under the host sanitizers (-fsanitize=address,undefined) in a process of its own.  It holds no rule: cut the
// gold row and every draw, take the distances by the textbook table (sr_distance; the device takes Myers' bit vectors,
// both are exact), the rewards, the advantages, the coefficients, and assemble the rows.
//
//   risk_rules_host_main CASES OUT
//
// CASES: "RISK", int32 count, then per case (one image) int32 samples, steps, start_id, end_id, pad_id; float32 alpha,
// label_smoothing; int32 formulas[steps + 1]; int32 draws[samples][steps].
// OUT per case: int32 rows[samples + 1][steps + 1]; float32 coef[samples + 1], smooth[samples + 1]; int32
// part[samples + 1]; int32 dist[samples], len[samples]; float32 reward[samples], advantage[samples].
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "risk_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "RISK", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[5];
        float mix[2];
        if (!get(in, head, sizeof head) || !get(in, mix, sizeof mix)) return 2;
        const int S = head[0], T = head[1], start_id = head[2], end_id = head[3], pad_id = head[4];
        if (rk_check(1, S, T, mix[0], mix[1]) != 0) return 2;
        std::vector<int32_t> formulas((size_t)T + 1), draws((size_t)S * T), rows((size_t)(S + 1) * (T + 1));
        std::vector<int32_t> part((size_t)S + 1), dist((size_t)S), len((size_t)S);
        std::vector<float> coef((size_t)S + 1), smooth((size_t)S + 1), reward((size_t)S), advantage((size_t)S);
        std::vector<double> r((size_t)S);
        if (!get(in, formulas.data(), formulas.size() * 4) || !get(in, draws.data(), draws.size() * 4)) return 2;
        const int32_t* gold = formulas.data() + 1;
        const int C = rk_gold_len(gold, T, end_id, pad_id);
        for (int t = 0; t <= T; ++t) rows[(size_t)t] = formulas[(size_t)t];
        coef[0] = rk_coef_gold(mix[0]); smooth[0] = mix[1]; part[0] = RK_PART_GOLD;
        for (int n = 0; n < S; ++n) {
            const int32_t* draw = draws.data() + (size_t)n * T;
            const int first_end = sr_first_end(draw, T, end_id);
            const int R = sr_cut_at(first_end, T).n;
            std::vector<int> table((size_t)C + 1);
            dist[(size_t)n] = sr_distance(draw, R, gold, C, table.data());
            len[(size_t)n] = R;
            r[(size_t)n] = rk_reward(dist[(size_t)n], R, C);
            reward[(size_t)n] = (float)r[(size_t)n];
            for (int t = 0; t <= T; ++t)
                rows[(size_t)(n + 1) * (T + 1) + t] = rk_draw_row_token(draw, t, first_end, start_id, pad_id);
        }
        for (int n = 0; n < S; ++n) {
            const double a = rk_advantage(r.data(), n, S);
            advantage[(size_t)n] = (float)a;
            coef[(size_t)n + 1] = rk_coef_draw(mix[0], a);
            smooth[(size_t)n + 1] = 0.f;
            part[(size_t)n + 1] = RK_PART_DRAW;
        }
        fwrite(rows.data(), 4, rows.size(), out);
        fwrite(coef.data(), 4, coef.size(), out);
        fwrite(smooth.data(), 4, smooth.size(), out);
        fwrite(part.data(), 4, part.size(), out);
        fwrite(dist.data(), 4, dist.size(), out);
        fwrite(len.data(), 4, len.size(), out);
        fwrite(reward.data(), 4, reward.size(), out);
        fwrite(advantage.data(), 4, advantage.size(), out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
