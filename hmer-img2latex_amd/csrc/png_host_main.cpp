// The shared PNG decode core (png_core.inc.h) as a stand-alone host program, so that the code which interprets
// untrusted bits can run under the host sanitizers (-fsanitize=address,undefined) in a process of its own.
//
//   png_host_main CASES OUT
//
// CASES: "PNGC", int32 count, then per case int32 width, height, colour_type, pal_n, int64 z_len, the zlib stream and
// 3 * pal_n palette bytes.  OUT: per case int32 status, int64 size, and `size` bytes: the unfiltered image
// (height * width * bpp, no filter bytes) when the status is 0, nothing otherwise.  Every buffer is allocated at its
// exact size, so a read or write outside it is a sanitizer report.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "png_core.inc.h"

struct HostSink {
    uint8_t* out;
    bool leader() const { return true; }
    void sync() const {}
    void literal(int64_t pos, uint8_t v) const { out[pos] = v; }
    void match(int64_t pos, int dist, int len) const {
        for (int i = 0; i < len; ++i) out[pos + i] = out[pos - dist + i % dist];
    }
    void stored(int64_t pos, const uint8_t* src, int len) const {
        for (int i = 0; i < len; ++i) out[pos + i] = src[i];
    }
};

static bool get(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    char magic[4];
    int32_t count = 0;
    if (!get(in, magic, 4) || memcmp(magic, "PNGC", 4) != 0 || !get(in, &count, 4) || count < 0) return 2;
    for (int32_t k = 0; k < count; ++k) {
        int32_t head[4];
        int64_t z_len = 0;
        if (!get(in, head, sizeof head) || !get(in, &z_len, 8)) return 2;
        const int w = head[0], h = head[1], ct = head[2], pal_n = head[3], bpp = png_bpp(ct);
        if (w < 1 || h < 1 || bpp == 0 || pal_n < 0 || pal_n > 256 || z_len < 0 || z_len > (1 << 28)) return 2;
        const int64_t expect = (int64_t)h * (1 + (int64_t)w * bpp);
        if (expect > ((int64_t)1 << 27)) return 2;
        std::vector<uint8_t> z((size_t)z_len), pal((size_t)pal_n * 3), f((size_t)expect);
        if (!get(in, z.data(), z.size()) || !get(in, pal.data(), pal.size())) return 2;
        PngTables* t = new PngTables;
        HostSink sink{f.data()};
        uint32_t want = 0;
        int32_t rc = png_inflate(z.data(), z_len, expect, *t, sink, &want);
        delete t;
        if (rc == PNG_OK) {
            uint64_t sa = 0, sb = 0;
            png_adler_partial(f.data(), expect, 0, 1, &sa, &sb);
            if (png_adler_finish(sa, sb, expect) != want) rc = PNG_E_ADLER;
        }
        if (rc == PNG_OK) rc = png_unfilter_scalar(f.data(), w, h, bpp);
        if (rc == PNG_OK && ct == 3)
            for (int y = 0; y < h && rc == PNG_OK; ++y)
                for (int x = 0; x < w; ++x)
                    if (f[(size_t)y * (1 + w) + 1 + x] >= pal_n) {
                        rc = PNG_E_PALETTE;
                        break;
                    }
        const int64_t size = rc == PNG_OK ? (int64_t)h * w * bpp : 0;
        fwrite(&rc, 4, 1, out);
        fwrite(&size, 8, 1, out);
        if (rc == PNG_OK)
            for (int y = 0; y < h; ++y) fwrite(f.data() + (size_t)y * (1 + (size_t)w * bpp) + 1, 1, (size_t)w * bpp, out);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 2;
}
