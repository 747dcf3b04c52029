// The part of the PNG decoder that interprets untrusted bits, shared between png.hip (the device kernel, one wave per
// image) and a stand-alone host program (png_host_main.cpp, built with sanitizers): the bit reader, the zlib header
// check, code-length and table construction, symbol decode, the match bounds logic, the Adler-32 sums and the filter
// arithmetic.  Plain C++, no HIP: PNG_HD is `__host__ __device__` under hipcc and empty elsewhere.
//
// Who writes the output is the caller's business: png_inflate() is a template over a Sink with
//   bool leader()                                  one caller per image writes the tables (lane 0 of the wave; true on the host)
//   void sync()                                    the Sink's earlier writes are visible to its later reads
//   void literal(int64 pos, uint8 v)               out[pos] = v
//   void match(int64 pos, int dist, int len)       out[pos + i] = out[pos - dist + i % dist], i < len (a periodic copy)
//   void stored(int64 pos, const uint8* src, int len)
// and calls them only with pos + len <= expect and dist <= pos: the bounds are decided here, once, for both builds.
// On the device every lane of the wave runs this code with the same values (loads of one address are a broadcast), so
// control flow stays wave-uniform and the Sink's copies can use all 64 lanes.
//
// Every loop below is bounded by the input or the output length: a symbol costs at least one bit, a block at least
// three, a stored block moves LEN bytes of both, and the first bit that is not there ends the decode (PNG_E_TRUNCATED).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

// status words (0 = decoded)
enum {
    PNG_OK = 0,
    PNG_E_HEADER = 1,         // zlib header: CM != 8, window > 32 K, preset dictionary, FCHECK
    PNG_E_TRUNCATED = 2,      // the stream ends inside a block or in front of its checksum
    PNG_E_BLOCK_TYPE = 3,     // BTYPE 3
    PNG_E_STORED_LEN = 4,     // LEN != ~NLEN
    PNG_E_CODE_LENGTHS = 5,   // over-subscribed or incomplete lengths, a bad repeat, HLIT / HDIST too large, no end code
    PNG_E_SYMBOL = 6,         // a code that no symbol has, literal/length symbol 286 / 287, distance code 30 / 31
    PNG_E_DISTANCE = 7,       // a distance beyond the start of the output or beyond the header's window
    PNG_E_TOO_MANY = 8,       // more output than height * (1 + width * bpp)
    PNG_E_TOO_FEW = 9,        // less
    PNG_E_TRAILING = 10,      // compressed bytes behind the checksum
    PNG_E_ADLER = 11,
    PNG_E_FILTER = 12,        // a filter byte above 4
    PNG_E_PALETTE = 13        // a palette index at or beyond the PLTE entry count
};

constexpr int PNG_FAST_BITS = 9;
constexpr int PNG_MAX_SYMS = 288;
constexpr uint32_t PNG_ADLER_MOD = 65521u;

struct PngHuff {
    uint16_t fast[1 << PNG_FAST_BITS];   // (symbol << 4) | length for codes of up to 9 bits, indexed by the next 9 stream bits; 0 = longer / none
    uint16_t count[16];                  // codes per length
    uint16_t symbol[PNG_MAX_SYMS];       // symbols in canonical order
};

struct PngTables {                       // one per image in flight (LDS on the device)
    PngHuff lit, dist;
    uint8_t lens[PNG_MAX_SYMS + 32];     // code lengths being read: up to 286 + 30
};

struct PngBits {
    const uint8_t* p;
    int64_t pos, end;                    // next byte to load, one past the last
    uint64_t buf;
    int cnt;                             // valid bits in buf
};

// at least 33 valid bits afterwards unless the input ends first; never reads at or beyond `end`
PNG_HD void png_refill(PngBits& b) {
    if (b.cnt > 32) return;
    if (b.pos + 4 <= b.end) {
        const uint8_t* q = b.p + b.pos;
        const uint32_t w = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        b.buf |= (uint64_t)w << b.cnt;
        b.cnt += 32;
        b.pos += 4;
    } else {
        while (b.pos < b.end && b.cnt <= 56) {                       // at most three bytes
            b.buf |= (uint64_t)b.p[b.pos++] << b.cnt;
            b.cnt += 8;
        }
    }
}

// n <= 16 bits, or -1 when the stream does not hold them
PNG_HD int png_take(PngBits& b, int n) {
    png_refill(b);
    if (b.cnt < n) return -1;
    const int v = (int)(b.buf & ((1u << n) - 1u));
    b.buf >>= n;
    b.cnt -= n;
    return v;
}

// Canonical Huffman tables from lens[0 .. n).  complete_only: an incomplete set is an error (the code-length code);
// otherwise zlib's rule: incomplete is accepted only with no code at all or one code of one bit (inflate_table).
template <class Sink>
PNG_HD int png_build(PngHuff& h, const uint8_t* lens, int n, bool complete_only, Sink& sink) {
    uint16_t count[16], offs[16], next[16];
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int s = 0; s < n; ++s) ++count[lens[s] & 15];
    int left = 1, codes = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)count[l];
        if (left < 0) return PNG_E_CODE_LENGTHS;                    // over-subscribed
        codes += count[l];
    }
    if (left > 0 && (complete_only || !(codes == 0 || (codes == 1 && count[1] == 1)))) return PNG_E_CODE_LENGTHS;
    offs[1] = 0;
    next[1] = 0;
    for (int l = 1; l < 15; ++l) {
        offs[l + 1] = (uint16_t)(offs[l] + count[l]);
        next[l + 1] = (uint16_t)((next[l] + count[l]) << 1);
    }
    sink.sync();
    if (sink.leader()) {
        for (int i = 0; i < (1 << PNG_FAST_BITS); ++i) h.fast[i] = 0;
        h.count[0] = 0;
        for (int l = 1; l < 16; ++l) h.count[l] = count[l];
        for (int s = 0; s < n; ++s) {
            const int l = lens[s] & 15;
            if (l == 0) continue;
            h.symbol[offs[l]++] = (uint16_t)s;                       // offs[l] stays below codes <= n <= 288
            const uint32_t code = next[l]++;
            if (l <= PNG_FAST_BITS) {
                uint32_t rev = 0;
                for (int k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);
                for (uint32_t i = rev; i < (1u << PNG_FAST_BITS); i += 1u << l) h.fast[i] = (uint16_t)((s << 4) | l);
            }
        }
    }
    sink.sync();
    return PNG_OK;
}

// one symbol, or -PNG_E_TRUNCATED / -PNG_E_SYMBOL
PNG_HD int png_symbol(PngBits& b, const PngHuff& h) {
    png_refill(b);
    const uint16_t e = h.fast[b.buf & ((1u << PNG_FAST_BITS) - 1u)];
    if (e) {
        const int l = e & 15;
        if (l > b.cnt) return -PNG_E_TRUNCATED;
        b.buf >>= l;
        b.cnt -= l;
        return e >> 4;
    }
    int code = 0, first = 0, index = 0;                              // bit by bit, canonical order (codes of 10 .. 15 bits)
    uint64_t bits = b.buf;
    for (int l = 1; l < 16; ++l) {
        if (l > b.cnt) return -PNG_E_TRUNCATED;
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = h.count[l];
        if (code - c < first) {
            b.buf >>= l;
            b.cnt -= l;
            return h.symbol[index + (code - first)];                 // index + code - first < the number of codes
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -PNG_E_SYMBOL;
}

PNG_HD void png_fixed_lengths(uint8_t* lens) {
    for (int s = 0; s < 144; ++s) lens[s] = 8;
    for (int s = 144; s < 256; ++s) lens[s] = 9;
    for (int s = 256; s < 280; ++s) lens[s] = 7;
    for (int s = 280; s < 288; ++s) lens[s] = 8;
    for (int s = 288; s < 320; ++s) lens[s] = 5;                     // the 32 distance codes behind them
}

PNG_HD int png_length_base(int s) {    // s = symbol - 257, 0 .. 28
    const int extra = s < 8 ? 0 : (s == 28 ? 0 : (s - 4) >> 2);
    return s < 8 ? 3 + s : (s == 28 ? 258 : 3 + ((4 + (s & 3)) << extra));
}
PNG_HD int png_length_extra(int s) { return s < 8 ? 0 : (s == 28 ? 0 : (s - 4) >> 2); }
PNG_HD int png_dist_extra(int s) { return s < 4 ? 0 : (s - 2) >> 1; }           // s = 0 .. 29
PNG_HD int png_dist_base(int s) { return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << ((s - 2) >> 1)); }

// RFC 1950 / 1951: z[0 .. zlen) must inflate to exactly `expect` bytes, which the Sink receives, and end with its
// checksum and nothing else.  *adler_out = the stream's Adler-32 (the caller compares it with the output's).
template <class Sink>
PNG_HD int png_inflate(const uint8_t* z, int64_t zlen, int64_t expect, PngTables& t, Sink& sink, uint32_t* adler_out) {
    if (zlen < 2) return PNG_E_TRUNCATED;
    const uint32_t cmf = z[0], flg = z[1];
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u) || ((cmf << 8) | flg) % 31u != 0) return PNG_E_HEADER;
    const int64_t window = (int64_t)1 << ((cmf >> 4) + 8);
    PngBits b{z, 2, zlen, 0, 0};
    int64_t pos = 0;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (;;) {                                                       // a block per round: at least three bits each
        const int head = png_take(b, 3);
        if (head < 0) return PNG_E_TRUNCATED;
        const int type = head >> 1;
        if (type == 3) return PNG_E_BLOCK_TYPE;
        if (type == 0) {
            const int drop = b.cnt & 7;                              // to the byte boundary
            b.buf >>= drop;
            b.cnt -= drop;
            const int len = png_take(b, 16), nlen = png_take(b, 16);
            if (len < 0 || nlen < 0) return PNG_E_TRUNCATED;
            if ((len ^ nlen) != 0xffff) return PNG_E_STORED_LEN;
            const int64_t at = b.pos - (b.cnt >> 3);                 // the bit buffer holds whole bytes here
            if (at + len > zlen) return PNG_E_TRUNCATED;
            if (pos + len > expect) return PNG_E_TOO_MANY;
            sink.stored(pos, z + at, len);
            pos += len;
            b.pos = at + len;
            b.buf = 0;
            b.cnt = 0;
        } else {
            if (type == 1) {
                if (sink.leader()) png_fixed_lengths(t.lens);
                sink.sync();
                int rc = png_build(t.lit, t.lens, 288, false, sink);
                if (rc == PNG_OK) rc = png_build(t.dist, t.lens + 288, 32, false, sink);
                if (rc != PNG_OK) return rc;
            } else {
                const int hlit = png_take(b, 5), hdist = png_take(b, 5), hclen = png_take(b, 4);
                if (hlit < 0 || hdist < 0 || hclen < 0) return PNG_E_TRUNCATED;
                const int nlit = hlit + 257, ndist = hdist + 1, ncode = hclen + 4;
                if (nlit > 286 || ndist > 30) return PNG_E_CODE_LENGTHS;
                uint8_t cl[19];
                for (int i = 0; i < 19; ++i) cl[i] = 0;
                for (int i = 0; i < ncode; ++i) {
                    const int v = png_take(b, 3);
                    if (v < 0) return PNG_E_TRUNCATED;
                    cl[order[i]] = (uint8_t)v;
                }
                int rc = png_build(t.lit, cl, 19, true, sink);       // the code-length code borrows the literal table
                if (rc != PNG_OK) return rc;
                int have = 0, prev = 0;
                while (have < nlit + ndist) {                        // a symbol per round: at least one bit, at least one length
                    const int s = png_symbol(b, t.lit);
                    if (s < 0) return -s;
                    int rep = 1, val = s;
                    if (s >= 16) {
                        const int nb = s == 16 ? 2 : (s == 17 ? 3 : 7);
                        const int x = png_take(b, nb);
                        if (x < 0) return PNG_E_TRUNCATED;
                        if (s == 16 && have == 0) return PNG_E_CODE_LENGTHS;
                        val = s == 16 ? prev : 0;
                        rep = (s == 16 ? 3 : (s == 17 ? 3 : 11)) + x;
                    }
                    if (have + rep > nlit + ndist) return PNG_E_CODE_LENGTHS;
                    if (sink.leader())
                        for (int i = 0; i < rep; ++i) t.lens[have + i] = (uint8_t)val;
                    have += rep;
                    prev = val;
                }
                sink.sync();
                if (t.lens[256] == 0) return PNG_E_CODE_LENGTHS;     // no end-of-block code
                rc = png_build(t.lit, t.lens, nlit, false, sink);
                if (rc == PNG_OK) rc = png_build(t.dist, t.lens + nlit, ndist, false, sink);
                if (rc != PNG_OK) return rc;
            }
            for (;;) {                                               // a symbol per round: at least one bit
                const int s = png_symbol(b, t.lit);
                if (s < 0) return -s;
                if (s < 256) {
                    if (pos >= expect) return PNG_E_TOO_MANY;
                    sink.literal(pos, (uint8_t)s);
                    ++pos;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return PNG_E_SYMBOL;
                int len = png_length_base(s - 257);
                const int le = png_length_extra(s - 257);
                if (le) {
                    const int x = png_take(b, le);
                    if (x < 0) return PNG_E_TRUNCATED;
                    len += x;
                }
                const int d = png_symbol(b, t.dist);
                if (d < 0) return -d;
                if (d > 29) return PNG_E_SYMBOL;
                int dist = png_dist_base(d);
                const int de = png_dist_extra(d);
                if (de) {
                    const int x = png_take(b, de);
                    if (x < 0) return PNG_E_TRUNCATED;
                    dist += x;
                }
                if (dist > pos || dist > window) return PNG_E_DISTANCE;   // the source begins in front of the output
                if (pos + len > expect) return PNG_E_TOO_MANY;            // the copy would leave the page
                sink.match(pos, dist, len);
                pos += len;
            }
        }
        if (head & 1) break;
    }
    if (pos != expect) return PNG_E_TOO_FEW;
    const int64_t at = b.pos - (b.cnt >> 3);                         // the first whole byte not consumed
    if (at + 4 > zlen) return PNG_E_TRUNCATED;
    if (at + 4 < zlen) return PNG_E_TRAILING;
    *adler_out = ((uint32_t)z[at] << 24) | ((uint32_t)z[at + 1] << 16) | ((uint32_t)z[at + 2] << 8) | (uint32_t)z[at + 3];
    return PNG_OK;
}

// Adler-32 as two plain sums, so that any split of the bytes between callers adds up: over i = start, start + stride, ...
// below n,  *sa += d[i],  *sb += (n - i) * d[i]  (n <= 2^27: no uint64 overflow).  png_adler_finish() of the totals is
// the checksum.
PNG_HD void png_adler_partial(const uint8_t* d, int64_t n, int64_t start, int64_t stride, uint64_t* sa, uint64_t* sb) {
    uint64_t a = 0, b = 0;
    for (int64_t i = start; i < n; i += stride) {
        a += d[i];
        b += (uint64_t)(n - i) * d[i];
    }
    *sa += a;
    *sb += b;
}
PNG_HD uint32_t png_adler_finish(uint64_t sa, uint64_t sb, int64_t n) {
    const uint32_t a = (uint32_t)((1u + sa) % PNG_ADLER_MOD);
    const uint32_t b = (uint32_t)(((uint64_t)n + sb) % PNG_ADLER_MOD);
    return (b << 16) | a;
}

// PNG spec 9.2: the reconstruction of one byte.  x: the filtered byte, a: left, b: above, c: above left (0 where absent)
PNG_HD uint8_t png_paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint8_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}
PNG_HD uint8_t png_recon(int filter, int x, int a, int b, int c) {
    switch (filter) {
        case 1: return (uint8_t)(x + a);
        case 2: return (uint8_t)(x + b);
        case 3: return (uint8_t)(x + ((a + b) >> 1));
        case 4: return (uint8_t)(x + png_paeth(a, b, c));
        default: return (uint8_t)x;
    }
}

// Pillow's L of an RGB pixel (Convert.c L24)
PNG_HD uint8_t png_luma(int r, int g, int b) { return (uint8_t)((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16); }

PNG_HD int png_bpp(int colour_type) {   // bytes per pixel at bit depth 8; 0 = not a colour type
    return colour_type == 0 ? 1 : colour_type == 2 ? 3 : colour_type == 3 ? 1 : colour_type == 4 ? 2 : colour_type == 6 ? 4 : 0;
}

// The rows of an image one byte after the other (the host program's unfilter, and the rule the device's row kernels
// are written against): f holds h rows of 1 + w * bpp bytes, reconstructed in place.  Returns PNG_E_FILTER for a filter
// byte above 4.
PNG_HD int png_unfilter_scalar(uint8_t* f, int w, int h, int bpp) {
    const int64_t rb = (int64_t)w * bpp, stride = rb + 1;
    for (int y = 0; y < h; ++y) {
        uint8_t* cur = f + y * stride + 1;
        const uint8_t* prev = cur - stride;                          // read only when y > 0
        const int ft = cur[-1];
        if (ft > 4) return PNG_E_FILTER;
        if (ft == 0) continue;
        for (int64_t i = 0; i < rb; ++i) {
            const int a = i >= bpp ? cur[i - bpp] : 0, b = y > 0 ? prev[i] : 0, c = (i >= bpp && y > 0) ? prev[i - bpp] : 0;
            cur[i] = png_recon(ft, cur[i], a, b, c);
        }
    }
    return PNG_OK;
}
