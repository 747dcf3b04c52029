// The error analysis' rules (edit_align_rules.inc.h) as a stand-alone host program, so that every pair of short
// sequences and crafted tie cases can be fed to them under the host sanitizers (-fsanitize=address,undefined) in a
// process of its own.  It holds no rule: fill the table, walk it; fill the bit vectors, walk them.
//
//   edit_align_host_main CASES OUT
//
// CASES: "EALN", int32 count, then per case int32 m, n, V; int32 r[m] (the target); int32 p[n] (the prediction).
// OUT per case, twice -- from the full table, then from the bit vectors of the device's column pass:
//   int32 len, ops[4]; uint8 script[len] (forward order); uint32 C[(V + 1) * (V + 1)].
// Every buffer is allocated at its exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "edit_align_rules.inc.h"

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static void put(FILE* out, int len, const int32_t* ops, const std::vector<uint8_t>& rev, const std::vector<uint32_t>& C) {
    const int32_t head[5] = {len, ops[0], ops[1], ops[2], ops[3]};
    fwrite(head, 4, 5, out);
    std::vector<uint8_t> script((size_t)len);
    for (int k = 0; k < len; ++k) script[k] = rev[len - 1 - k];
    fwrite(script.data(), 1, script.size(), out);
    fwrite(C.data(), 4, C.size(), out);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "EALN", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[3];
        if (!get(in, head, sizeof head)) return 2;
        const int m = head[0], n = head[1], V = head[2];
        if (m < 0 || m > EA_MAX_STRIDE || n < 0 || n > EA_MAX_STRIDE || V < 1 || V > EA_MAX_VOCAB) return 2;
        std::vector<int32_t> r((size_t)m), p((size_t)n);
        if (!get(in, r.data(), r.size() * 4) || !get(in, p.data(), p.size() * 4)) return 2;
        const size_t cells = ((size_t)V + 1) * ((size_t)V + 1);
        int32_t ops[4];
        {
            std::vector<int> D(((size_t)m + 1) * ((size_t)n + 1));
            std::vector<uint8_t> rev((size_t)m + n);
            std::vector<uint32_t> C(cells, 0u);
            ea_table(r.data(), m, p.data(), n, D.data());
            const int len = ea_walk(r.data(), m, p.data(), n, EaTableCells{D.data(), (size_t)n + 1}, V, rev.data(), ops, C.data());
            put(out, len, ops, rev, C);
        }
        {
            const int W = (m + 63) / 64;
            std::vector<ea_u64> vec((size_t)n * W * 2), pv((size_t)W), mv((size_t)W);
            std::vector<uint8_t> rev((size_t)m + n);
            std::vector<uint32_t> C(cells, 0u);
            ea_fill_columns(r.data(), m, p.data(), n, W, vec.data(), pv.data(), mv.data());
            const int len = ea_walk(r.data(), m, p.data(), n, EaBitCells{vec.data(), W}, V, rev.data(), ops, C.data());
            put(out, len, ops, rev, C);
        }
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
