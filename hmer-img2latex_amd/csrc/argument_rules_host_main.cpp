// The argument rules (argument_rules.inc.h) as a stand-alone host program, so that a host test can walk them step by
// step -- arguments owed at depth 31, budgets that run out inside an argument, broken tables -- and enumerate every
// sequence they allow, under the host sanitizers (-fsanitize=address,undefined) in a process of its own.  It holds no
// rule: the loop `for t: mask; first-index arg max of the allowed logits; advance`, and a depth-first walk of the masks.
//
//   argument_rules_host_main CASES OUT
//   argument_rules_host_main --enumerate TABLE OUT
//
// CASES: "ARGS", int32 count, then per case int32 V, steps, end_id; uint8 cls[V]; float32 logits[steps][V].
// OUT per case and step: uint8 allowed[V], int32 pick, then the 32 bytes of the state after the pick.
// TABLE: "ARGE", int32 V, steps, end_id; uint8 cls[V].
// OUT: per sequence that reaches END within `steps`, int32 n and its n ids (END last), in lexicographic order of the
// ids; then int32 -1 and three int64: the states visited before an END, those among them with NO column allowed, and
// the sequences that used all `steps` without END.
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "argument_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

struct Walk {
    const std::vector<uint8_t>& cls;
    int V, steps, end_id;
    FILE* out;
    std::vector<int32_t> ids;
    int64_t visited = 0, empty = 0, unfinished = 0;
    void go(const ArgumentState& st, int t) {
        if (t == steps) { ++unfinished; return; }
        ++visited;
        const ArgumentRow r = ar_row(st, steps - t - 1);
        bool any = false;
        for (int v = 0; v < V; ++v) {
            if (!ar_allowed(r, v == end_id, cls[(size_t)v])) continue;
            any = true;
            ids.push_back(v);
            if (v == end_id) {
                const int32_t n = (int32_t)ids.size();
                fwrite(&n, 4, 1, out);
                fwrite(ids.data(), 4, ids.size(), out);
            } else {
                ArgumentState next = st;
                ar_advance(next, false, cls[(size_t)v]);
                go(next, t + 1);
            }
            ids.pop_back();
        }
        if (!any) ++empty;
    }
};

static int enumerate(const char* table, const char* result) {
    FILE* in = fopen(table, "rb");
    FILE* out = fopen(result, "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t head[3];
    if (!get(in, magic, 4) || memcmp(magic, "ARGE", 4) != 0 || !get(in, head, sizeof head)) return 2;
    const int V = head[0], steps = head[1], end_id = head[2];
    if (V < 1 || V > 64 || steps < 1 || steps > 16 || end_id < 0 || end_id >= V) return 2;
    std::vector<uint8_t> cls((size_t)V);
    if (!get(in, cls.data(), cls.size())) return 2;
    Walk w{cls, V, steps, end_id, out};
    w.go(ArgumentState{}, 0);
    const int32_t stop = -1;
    const int64_t tail[3] = {w.visited, w.empty, w.unfinished};
    fwrite(&stop, 4, 1, out);
    fwrite(tail, sizeof tail, 1, out);
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 4 && strcmp(argv[1], "--enumerate") == 0) return enumerate(argv[2], argv[3]);
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "ARGS", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[3];
        if (!get(in, head, sizeof head)) return 2;
        const int V = head[0], steps = head[1], end_id = head[2];
        if (V < 1 || V > 4096 || steps < 1 || steps > 4096 || end_id < 0 || end_id >= V) return 2;
        std::vector<uint8_t> cls((size_t)V), allowed((size_t)V);
        std::vector<float> x((size_t)V);
        if (!get(in, cls.data(), cls.size())) return 2;
        ArgumentState st{};
        for (int t = 0; t < steps; ++t) {
            if (!get(in, x.data(), x.size() * sizeof(float))) return 2;
            const ArgumentRow r = ar_row(st, steps - t - 1);
            float best = -INFINITY;
            int pick = -1;
            for (int v = 0; v < V; ++v) {
                allowed[(size_t)v] = ar_allowed(r, v == end_id, cls[(size_t)v]) ? 1 : 0;
                if (allowed[(size_t)v] && x[(size_t)v] > best) { best = x[(size_t)v]; pick = v; }
            }
            if (pick < 0) pick = ar_fallback(r, cls.data(), V, end_id);
            ar_advance(st, pick == end_id, cls[(size_t)pick]);
            const int32_t p32 = pick;
            fwrite(allowed.data(), 1, allowed.size(), out);
            fwrite(&p32, 4, 1, out);
            fwrite(&st, sizeof st, 1, out);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
