// The case-walking loop of the rule sets' stand-alone host programs (bracket_rules_host_main.cpp,
// argument_rules_host_main.cpp), written once over a rule model (bracket_rules.inc.h).  It holds no rule: the loop
// `for t: mask; first-index arg max of the allowed logits; advance`.
//
// CASES: the program's 4-byte magic, int32 count, then per case int32 V, steps, end_id; uint8 cls[V];
// float32 logits[steps][V].
// OUT per case and step: uint8 allowed[V], int32 pick, then the bytes of the model's state after the pick.
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#pragma once
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bracket_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

// the program's exit status
template <class Model>
int walk_cases(const char* cases, const char* result, const char* want_magic) {
    FILE* in = fopen(cases, "rb");
    FILE* out = fopen(result, "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, want_magic, 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[3];
        if (!get(in, head, sizeof head)) return 2;
        const int V = head[0], steps = head[1], end_id = head[2];
        if (V < 1 || V > 4096 || steps < 1 || steps > 4096 || end_id < 0 || end_id >= V) return 2;
        std::vector<uint8_t> cls((size_t)V), allowed((size_t)V);
        std::vector<float> x((size_t)V);
        if (!get(in, cls.data(), cls.size())) return 2;
        typename Model::State st{};
        for (int t = 0; t < steps; ++t) {
            if (!get(in, x.data(), x.size() * sizeof(float))) return 2;
            const typename Model::Row r = Model::row(st, steps - t - 1);
            float best = -INFINITY;
            int pick = -1;
            for (int v = 0; v < V; ++v) {
                allowed[(size_t)v] = Model::allowed(r, v == end_id, cls[(size_t)v]) ? 1 : 0;
                if (allowed[(size_t)v] && x[(size_t)v] > best) { best = x[(size_t)v]; pick = v; }
            }
            if (pick < 0) pick = constraint_fallback<Model>(r, cls.data(), V, end_id);
            Model::advance(st, pick == end_id, cls[(size_t)pick]);
            const int32_t p32 = pick;
            fwrite(allowed.data(), 1, allowed.size(), out);
            fwrite(&p32, 4, 1, out);
            fwrite(&st, sizeof st, 1, out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
