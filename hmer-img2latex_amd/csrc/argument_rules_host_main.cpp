// The argument rules (argument_rules.inc.h) as a stand-alone host program, so that a host test can walk them step by
// step -- arguments owed at depth 31, budgets that run out inside an argument, broken tables -- and enumerate every
// sequence they allow, under the host sanitizers (-fsanitize=address,undefined) in a process of its own.  It holds no
// rule: rules_walk_host.inc.h's walk of the cases, and a depth-first walk of the masks.
//
//   argument_rules_host_main CASES OUT
//   argument_rules_host_main --enumerate TABLE OUT
//
// CASES ("ARGS") and OUT (32 bytes of state per step) are rules_walk_host.inc.h's.
// TABLE: "ARGE", int32 V, steps, end_id; uint8 cls[V].
// OUT: per sequence that reaches END within `steps`, int32 n and its n ids (END last), in lexicographic order of the
// ids; then int32 -1 and three int64: the states visited before an END, those among them with NO column allowed, and
// the sequences that used all `steps` without END.
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include "argument_rules.inc.h"
#include "rules_walk_host.inc.h"

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
    return argc == 3 ? walk_cases<ArgumentModel>(argv[1], argv[2], "ARGS") : 2;
}
