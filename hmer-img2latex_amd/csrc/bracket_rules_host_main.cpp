// The bracket constraint's rules (bracket_rules.inc.h) as a stand-alone host program, so that a host test can walk them
// step by step -- depth 32, budgets that run out, broken tables -- under the host sanitizers
// (-fsanitize=address,undefined) in a process of its own.  It holds no rule: the loop `for t: mask; first-index arg max
// of the allowed logits; advance`.
//
//   bracket_rules_host_main CASES OUT
//
// CASES: "BRKT", int32 count, then per case int32 V, steps, end_id; uint8 cls[V]; float32 logits[steps][V].
// OUT per case and step: uint8 allowed[V], int32 pick, then the 16 bytes of the state after the pick.
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bracket_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "BRKT", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[3];
        if (!get(in, head, sizeof head)) return 2;
        const int V = head[0], steps = head[1], end_id = head[2];
        if (V < 1 || V > 4096 || steps < 1 || steps > 4096 || end_id < 0 || end_id >= V) return 2;
        std::vector<uint8_t> cls((size_t)V), allowed((size_t)V);
        std::vector<float> x((size_t)V);
        if (!get(in, cls.data(), cls.size())) return 2;
        BracketState st{};
        for (int t = 0; t < steps; ++t) {
            if (!get(in, x.data(), x.size() * sizeof(float))) return 2;
            const int rem = steps - t - 1;
            float best = -INFINITY;
            int pick = -1;
            for (int v = 0; v < V; ++v) {
                allowed[(size_t)v] = br_allowed(st, v == end_id, cls[(size_t)v], rem) ? 1 : 0;
                if (allowed[(size_t)v] && x[(size_t)v] > best) { best = x[(size_t)v]; pick = v; }
            }
            if (pick < 0) pick = br_fallback(st, cls.data(), V, end_id, rem);
            br_advance(st, pick == end_id, cls[(size_t)pick]);
            const int32_t p32 = pick;
            fwrite(allowed.data(), 1, allowed.size(), out);
            fwrite(&p32, 4, 1, out);
            fwrite(&st, sizeof st, 1, out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
