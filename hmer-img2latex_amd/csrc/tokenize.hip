// Packed UTF-8 text -> padded token id rows on the device: LaTeXTokenizer.encode / encode_batch (reference
// img2latex/data/tokenizer.py:143-164,196-232) and the data set's "START formula END" rule (data/dataset.py:333-335,
// collator :59-66).  Token rule = Python's str.split() without an argument: tokens are the maximal runs of bytes that
// belong to no whitespace character, whitespace being the 29 code points of str.isspace(), matched by their UTF-8 byte
// patterns (ws_len; exact at any byte position of well-formed UTF-8, which is self-synchronising).  Id rule = the
// table entry whose bytes EQUAL the token's bytes, else unk_id (tokenizer.py:162).
//
// One launch, one wave per row, lane = byte: per 64 bytes every lane classifies its byte from the bytes p, p + 1, p + 2
// (neighbouring lanes read neighbouring bytes; a pattern of 2 or 3 bytes marks its later bytes through its neighbours'
// lanes, the last two lanes of a chunk hand theirs to the next chunk), a ballot of the token starts plus the count of
// the chunks before gives every token its ordinal = its output column, and the lane of a token's first byte walks the
// token (FNV-1a, stopping one byte past the longest key: such a token is in no table), probes the open-addressing table
// and compares the bytes of a slot whose hash and length agree.  Tokens past `width` are counted, not looked up.  The
// wave then writes START / END and pads the row.  The classifier, the chunk scan and the walk are text_scan.inc.h,
// shared with vocab_fit.hip.
#include "common.h"

#include <string.h>

namespace {

#include "text_scan.inc.h"

constexpr int TT = 256;                         // threads per workgroup: four rows
constexpr uint32_t TABLE_MAGIC = 0x314e4b54u;   // "TKN1"
constexpr int HDR_WORDS = 8;                    // magic, slots, longest key, keys, byte offset of the key bytes, total bytes, 0, 0

struct Slot {                                   // 16 bytes; len < 0: empty
    uint32_t hash;
    int32_t start;                              // first byte of the key, relative to the key bytes
    int32_t len;
    int32_t id;
};

__host__ __device__ inline size_t slots_for(size_t n) {
    size_t s = 2;
    while (s < 2 * n) s <<= 1;                  // load factor <= 1/2
    return s;
}

__global__ __launch_bounds__(TT) void tokenize_kernel(const uint8_t* __restrict__ text, long long text_bytes,
                                                      const int32_t* __restrict__ row_off, int rows,
                                                      const int32_t* __restrict__ table, long long table_bytes, int unk_id,
                                                      int pad_id, int start_id, int end_id, int add_special, int width,
                                                      int32_t* __restrict__ out_ids, int out_stride,
                                                      int32_t* __restrict__ out_len, int32_t* __restrict__ out_count,
                                                      int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (TT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    int flags = 0;
    long long s = row_off[row], e = row_off[row + 1];
    if (s < 0 || e < s || e > text_bytes) {                          // unusable offsets: an empty row, nothing is read
        s = e = 0;
        flags |= 2;
    }
    // the table image describes itself; one that does not add up is never probed
    const long long n_slots = table[1], max_key = table[2], key_base = table[4], total = table[5];
    const bool table_ok = (uint32_t)table[0] == TABLE_MAGIC && n_slots >= 2 && (n_slots & (n_slots - 1)) == 0 &&
                          key_base == (long long)HDR_WORDS * 4 + n_slots * (long long)sizeof(Slot) && key_base <= total &&
                          total == table_bytes && max_key >= 0;
    if (!table_ok) flags |= 4;
    const uint4* slots = reinterpret_cast<const uint4*>(table + HDR_WORDS);
    const uint8_t* keys = reinterpret_cast<const uint8_t*>(table) + key_base;
    const long long key_bytes = total - key_base;
    const uint32_t mask = (uint32_t)(n_slots - 1);
    int32_t* out = out_ids + (size_t)row * out_stride;

    int n_tok = 0;                                                   // tokens of the chunks before
    ChunkScan scan;
    for (long long base = s; base < e; base += 64) {
        const long long p = base + lane;
        const bool tok_start = scan.step(text, base, e, lane);
        const long long col = (long long)n_tok + scan.before(lane) + add_special;
        if (tok_start && col < width) {
            // one byte past the longest key the token is UNK wherever it ends
            uint32_t h;
            const long long len = token_walk(text, p, e, scan.c0, scan.c1, scan.c2, max_key, h);
            int id = unk_id;
            if (table_ok && len <= max_key) {
                uint32_t sl = first_slot(h, mask);
                for (long long probe = 0; probe < n_slots; ++probe) {
                    const uint4 S = slots[sl];
                    const long long k_start = (int32_t)S.y, k_len = (int32_t)S.z;
                    if (k_len < 0) break;                            // an empty slot ends the probe
                    if (S.x == h && k_len == len && k_start >= 0 && k_start + k_len <= key_bytes) {
                        long long k = 0;
                        while (k < len && keys[k_start + k] == text[p + k]) ++k;
                        if (k == len) {
                            id = (int32_t)S.w;
                            break;
                        }
                    }
                    sl = (sl + 1) & mask;
                }
            }
            out[col] = id;
        }
        n_tok += __popcll(scan.starts);
    }
    const long long count = (long long)n_tok + (add_special ? 2 : 0);
    const int n = (int)(count < width ? count : width);
    if (lane == 0) {
        if (add_special) {
            out[0] = start_id;                                       // width >= 1
            if ((long long)n_tok + 1 < width) out[n_tok + 1] = end_id;   // an over-long row loses its END
        }
        out_len[row] = n;
        if (out_count) out_count[row] = (int32_t)count;
        if (count > width) flags |= 1;
        if (flags) atomicOr(status, flags);
    }
    for (int c = n + lane; c < width; c += 64) out[c] = pad_id;
}

uint32_t key_hash(const uint8_t* b, long long n) {
    uint32_t h = FNV_SEED;
    for (long long i = 0; i < n; ++i) h = fnv_step(h, b[i]);
    return h;
}

}  // namespace

extern "C" size_t i2l_tokenize_table_bytes(int n, int64_t key_bytes) {
    if (n < 0 || key_bytes < 0) return 0;
    const unsigned long long total = (unsigned long long)HDR_WORDS * 4 + (unsigned long long)slots_for((size_t)n) * sizeof(Slot) +
                                     (((unsigned long long)key_bytes + 3ull) & ~3ull);
    return total > 0x7fffffffull ? 0 : (size_t)total;               // the image's own offsets are int32
}

extern "C" int i2l_tokenize_table_build(const uint8_t* tok_bytes, const int32_t* tok_off, const int32_t* tok_id, int n,
                                        void* image, size_t image_bytes) {
    if (!tok_off || !image || n < 0 || (n > 0 && !tok_id)) return I2L_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (tok_off[i + 1] < tok_off[i]) return I2L_ERR_ARG;
    if (tok_off[0] < 0) return I2L_ERR_ARG;
    const long long key_bytes = (long long)tok_off[n] - tok_off[0];
    if (key_bytes > 0 && !tok_bytes) return I2L_ERR_ARG;
    const size_t total = i2l_tokenize_table_bytes(n, key_bytes);
    if (total == 0) return I2L_ERR_UNSUPPORTED;
    if (image_bytes < total) return I2L_ERR_WORKSPACE;
    const size_t n_slots = slots_for((size_t)n);
    const uint32_t mask = (uint32_t)(n_slots - 1);
    memset(image, 0, total);
    int32_t* hdr = static_cast<int32_t*>(image);
    Slot* slots = reinterpret_cast<Slot*>(hdr + HDR_WORDS);
    uint8_t* keys = reinterpret_cast<uint8_t*>(slots + n_slots);
    for (size_t i = 0; i < n_slots; ++i) slots[i].len = -1;
    if (key_bytes > 0) memcpy(keys, tok_bytes + tok_off[0], (size_t)key_bytes);
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        const int32_t start = tok_off[i] - tok_off[0], len = tok_off[i + 1] - tok_off[i];
        const uint32_t h = key_hash(keys + start, len);
        uint32_t sl = first_slot(h, mask);
        while (slots[sl].len >= 0) {                                 // load <= 1/2: an empty slot always comes
            if (slots[sl].hash == h && slots[sl].len == len && memcmp(keys + slots[sl].start, keys + start, (size_t)len) == 0)
                return I2L_ERR_ARG;                                  // the same key twice
            sl = (sl + 1) & mask;
        }
        slots[sl] = Slot{h, start, len, tok_id[i]};
        longest = len > longest ? len : longest;
    }
    hdr[0] = (int32_t)TABLE_MAGIC;
    hdr[1] = (int32_t)n_slots;
    hdr[2] = longest;
    hdr[3] = n;
    hdr[4] = (int32_t)(HDR_WORDS * 4 + n_slots * sizeof(Slot));
    hdr[5] = (int32_t)total;
    return I2L_OK;
}

extern "C" int i2l_tokenize(const uint8_t* text, int64_t text_bytes, const int32_t* row_off, int rows, const void* table,
                            size_t table_bytes, int unk_id, int pad_id, int start_id, int end_id, int add_special, int width,
                            int32_t* out_ids, int out_stride, int32_t* out_len, int32_t* out_count, int32_t* status,
                            i2l_stream_t stream) {
    if (width <= 0 || out_stride < width || text_bytes > 0x7fffffffLL) return I2L_ERR_UNSUPPORTED;
    if (rows < 0 || text_bytes < 0 || (add_special != 0 && add_special != 1)) return I2L_ERR_ARG;
    if (rows == 0) return I2L_OK;
    if (!row_off || !table || table_bytes < (size_t)HDR_WORDS * 4 || !out_ids || !out_len || !status || (text_bytes > 0 && !text))
        return I2L_ERR_ARG;
    hipStream_t s = i2l_s(stream);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return I2L_ERR_LAUNCH;
    hipLaunchKernelGGL(tokenize_kernel, dim3(i2l_cdiv(rows, TT / 64)), dim3(TT), 0, s, text, (long long)text_bytes, row_off,
                       rows, static_cast<const int32_t*>(table), (long long)table_bytes, unk_id, pad_id, start_id, end_id,
                       add_special, width, out_ids, out_stride, out_len, out_count, status);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
