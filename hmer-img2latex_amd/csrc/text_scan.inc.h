// What tokenize.hip and vocab_fit.hip share: Python's str.split() on packed UTF-8, a wave per row, lane = byte.
// The whitespace classifier, the FNV-1a step, the 64-byte chunk scan that finds the token starts, and the walk of one
// token by the lane on its first byte.  Included inside each file's unnamed namespace.
#pragma once

constexpr uint32_t FNV_SEED = 2166136261u;

__host__ __device__ inline uint32_t fnv_step(uint32_t h, uint32_t b) { return (h ^ b) * 16777619u; }
__host__ __device__ inline uint32_t first_slot(uint32_t h, uint32_t mask) { return (h ^ (h >> 16)) & mask; }

// Bytes of the whitespace character that BEGINS with c0 c1 c2 (0: none does).  U+0009-000D, 001C-0020; C2 85, C2 A0;
// E1 9A 80; E2 80 80..8A, E2 80 A8, E2 80 A9, E2 80 AF; E2 81 9F; E3 80 80.
__host__ __device__ inline int ws_len(unsigned c0, unsigned c1, unsigned c2) {
    if ((c0 >= 0x09u && c0 <= 0x0du) || (c0 >= 0x1cu && c0 <= 0x20u)) return 1;
    if (c0 == 0xc2u) return (c1 == 0x85u || c1 == 0xa0u) ? 2 : 0;
    if (c0 == 0xe1u) return (c1 == 0x9au && c2 == 0x80u) ? 3 : 0;
    if (c0 == 0xe2u) {
        if (c1 == 0x80u) return ((c2 >= 0x80u && c2 <= 0x8au) || c2 == 0xa8u || c2 == 0xa9u || c2 == 0xafu) ? 3 : 0;
        return (c1 == 0x81u && c2 == 0x9fu) ? 3 : 0;
    }
    if (c0 == 0xe3u) return (c1 == 0x80u && c2 == 0x80u) ? 3 : 0;
    return 0;
}

// One row's scan state, carried from 64-byte chunk to chunk.  step() is called by all 64 lanes of the wave.
struct ChunkScan {
    int carry1 = 0, carry2 = 0;                 // ws_len of the previous chunk's last / second-last byte
    bool prev_ws = true;                        // the byte before this chunk is whitespace (or the row's start)
    unsigned c0, c1, c2;                        // this lane's byte and the two behind it (0 beyond the row's end e)
    unsigned long long starts;                  // ballot of the lanes on a token's first byte

    // Classifies the bytes base .. base + 63 of a row that ends at e: every lane from the bytes p, p + 1, p + 2; a pattern
    // of 2 or 3 bytes marks its later bytes through its neighbours' lanes, the last two lanes of a chunk hand theirs to
    // the next chunk.  True on the lane of a token's first byte.
    __device__ inline bool step(const uint8_t* __restrict__ text, long long base, long long e, int lane) {
        const long long p = base + lane;
        c0 = p < e ? text[p] : 0u;
        c1 = p + 1 < e ? text[p + 1] : 0u;
        c2 = p + 2 < e ? text[p + 2] : 0u;
        const int L = p < e ? ws_len(c0, c1, c2) : 0;
        int L1 = __shfl_up(L, 1, 64), L2 = __shfl_up(L, 2, 64);
        if (lane == 0) { L1 = carry1; L2 = carry2; }
        if (lane == 1) L2 = carry1;
        const bool ws = L > 0 || L1 >= 2 || L2 == 3 || p >= e;      // beyond the row: no token either
        const unsigned long long wsm = __ballot(ws);
        const bool before_ws = lane == 0 ? prev_ws : ((wsm >> (lane - 1)) & 1ull) != 0;
        const bool tok_start = !ws && before_ws;
        starts = __ballot(tok_start);
        carry1 = __shfl(L, 63, 64);
        carry2 = __shfl(L, 62, 64);
        prev_ws = ((wsm >> 63) & 1ull) != 0;
        return tok_start;
    }
    // tokens of this chunk in front of this lane's byte
    __device__ inline int before(int lane) const { return __popcll(starts & ((1ull << lane) - 1ull)); }
};

// The token whose first byte is text[p] (a0 a1 a2 = that byte and the two behind it): it ends in front of the next
// whitespace character (its bytes are in none, so that character BEGINS there) or at the row's end e.  Returns its
// length and its FNV-1a hash; the walk stops one byte past `limit`, wherever the token ends.
__device__ inline long long token_walk(const uint8_t* __restrict__ text, long long p, long long e, unsigned a0, unsigned a1,
                                       unsigned a2, long long limit, uint32_t& hash) {
    uint32_t h = FNV_SEED;
    long long len = 0, q = p;
    for (;;) {
        h = fnv_step(h, a0);
        ++len;
        ++q;
        if (q >= e || len > limit) break;
        a0 = a1;
        a1 = a2;
        a2 = q + 2 < e ? text[q + 2] : 0u;
        if (ws_len(a0, a1, a2) > 0) break;
    }
    hash = h;
    return len;
}
