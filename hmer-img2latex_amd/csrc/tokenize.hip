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
//
// i2l_tokenize_packed runs the same row body (row_tokens below) twice -- count, then write -- around a scan of the row
// counts, for rows that are never cut and never padded: the corpus of a data set, tokenized once into a CSR store.
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

// The table image as a kernel reads it.  The image describes itself; one that does not add up is never probed.
struct TableView {
    bool ok;
    const uint4* slots;
    const uint8_t* keys;
    long long n_slots, max_key, key_bytes;
    uint32_t mask;
};

__device__ inline TableView table_view(const int32_t* __restrict__ table, long long table_bytes) {
    TableView T;
    const long long key_base = table[4], total = table[5];
    T.n_slots = table[1];
    T.max_key = table[2];
    T.ok = (uint32_t)table[0] == TABLE_MAGIC && T.n_slots >= 2 && (T.n_slots & (T.n_slots - 1)) == 0 &&
           key_base == (long long)HDR_WORDS * 4 + T.n_slots * (long long)sizeof(Slot) && key_base <= total &&
           total == table_bytes && T.max_key >= 0;
    T.slots = reinterpret_cast<const uint4*>(table + HDR_WORDS);
    T.keys = reinterpret_cast<const uint8_t*>(table) + key_base;
    T.key_bytes = total - key_base;
    T.mask = (uint32_t)(T.n_slots - 1);
    return T;
}

// Row `row` of the text as [s, e); unusable offsets give an empty row (nothing is read) and the bad-offsets bit.
__device__ inline int row_span(const int32_t* __restrict__ row_off, int row, long long text_bytes, long long& s, long long& e) {
    s = row_off[row];
    e = row_off[row + 1];
    if (s < 0 || e < s || e > text_bytes) {
        s = e = 0;
        return 2;
    }
    return 0;
}

// The id of the token whose first byte is text[p], this lane's byte of `scan`: the walk, the probe and the compare.
__device__ inline int token_id(const uint8_t* __restrict__ text, long long p, long long e, const ChunkScan& scan,
                               const TableView& T, int unk_id) {
    // one byte past the longest key the token is UNK wherever it ends
    uint32_t h;
    const long long len = token_walk(text, p, e, scan.c0, scan.c1, scan.c2, T.max_key, h);
    int id = unk_id;
    if (T.ok && len <= T.max_key) {
        uint32_t sl = first_slot(h, T.mask);
        for (long long probe = 0; probe < T.n_slots; ++probe) {
            const uint4 S = T.slots[sl];
            const long long k_start = (int32_t)S.y, k_len = (int32_t)S.z;
            if (k_len < 0) break;                                    // an empty slot ends the probe
            if (S.x == h && k_len == len && k_start >= 0 && k_start + k_len <= T.key_bytes) {
                long long k = 0;
                while (k < len && T.keys[k_start + k] == text[p + k]) ++k;
                if (k == len) {
                    id = (int32_t)S.w;
                    break;
                }
            }
            sl = (sl + 1) & T.mask;
        }
    }
    return id;
}

// The row body that tokenize_kernel and the two passes of i2l_tokenize_packed share; called by all 64 lanes of the
// row's wave.  Walks the row [s, e) in 64-byte chunks; the lane on the first byte of token number t (0-based) calls
// emit(t, id) when t < limit -- tokens from `limit` on are counted, not looked up.  Returns the row's token count.
template <class Emit>
__device__ inline int row_tokens(const uint8_t* __restrict__ text, long long s, long long e, int lane, const TableView& T,
                                 int unk_id, long long limit, Emit emit) {
    int n_tok = 0;                                                   // tokens of the chunks before
    ChunkScan scan;
    for (long long base = s; base < e; base += 64) {
        const bool tok_start = scan.step(text, base, e, lane);
        const long long t = (long long)n_tok + scan.before(lane);
        if (tok_start && t < limit) emit(t, token_id(text, base + lane, e, scan, T, unk_id));
        n_tok += __popcll(scan.starts);
    }
    return n_tok;
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
    long long s, e;
    int flags = row_span(row_off, row, text_bytes, s, e);
    const TableView T = table_view(table, table_bytes);
    if (!T.ok) flags |= 4;
    int32_t* out = out_ids + (size_t)row * out_stride;
    const int n_tok = row_tokens(text, s, e, lane, T, unk_id, (long long)width - add_special,
                                 [&](long long t, int id) { out[t + add_special] = id; });
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

// ---- i2l_tokenize_packed: the same rows without the cut and the padding, packed without gaps (CSR)

constexpr int SCAN_T = 1024;            // threads of the scan workgroup

__global__ __launch_bounds__(TT) void packed_count_kernel(const uint8_t* __restrict__ text, long long text_bytes,
                                                          const int32_t* __restrict__ row_off, int rows,
                                                          const int32_t* __restrict__ table, long long table_bytes,
                                                          int add_special, int32_t* __restrict__ row_ids,
                                                          int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (TT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    long long s, e;
    int flags = row_span(row_off, row, text_bytes, s, e);
    const TableView T = table_view(table, table_bytes);
    if (!T.ok) flags |= 4;
    const int n_tok = row_tokens(text, s, e, lane, T, 0, 0, [](long long, int) {});     // limit 0: count only
    if (lane == 0) {
        row_ids[row] = n_tok + (add_special ? 2 : 0);                // <= 2^30 + 2: a token and its separator take 2 bytes
        if (flags) atomicOr(status, flags);
    }
}

__device__ __forceinline__ long long wave_inclusive_sum64(long long v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

// Exclusive scan of row_ids into out_off[0 .. rows], out_off[rows] = the total; status bit 0 iff it exceeds the capacity.
// One workgroup, chunks of SCAN_T rows with a running carry (detok_scan_kernel's scheme in 64 bits).
__global__ __launch_bounds__(SCAN_T) void packed_scan_kernel(const int32_t* __restrict__ row_ids, int rows, long long capacity,
                                                             int64_t* __restrict__ out_off, int32_t* __restrict__ status) {
    __shared__ long long wave_sum[SCAN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (int base = 0; base < rows; base += SCAN_T) {
        const int r = base + tid;                                    // rows <= 2^31 - 1 - SCAN_T (checked by the host)
        const long long v = r < rows ? row_ids[r] : 0;
        const long long incl = wave_inclusive_sum64(v, lane);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SCAN_T / 64; ++w) {
            const long long ws = wave_sum[w];
            before += w < wave ? ws : 0;
            all += ws;
        }
        if (r < rows) out_off[r] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        out_off[rows] = carry;
        if (carry > capacity) atomicOr(status, 1);
    }
}

__global__ __launch_bounds__(TT) void packed_write_kernel(const uint8_t* __restrict__ text, long long text_bytes,
                                                          const int32_t* __restrict__ row_off, int rows,
                                                          const int32_t* __restrict__ table, long long table_bytes, int unk_id,
                                                          int start_id, int end_id, int add_special,
                                                          const int64_t* __restrict__ out_off, int32_t* __restrict__ out_ids,
                                                          long long capacity) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (TT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    long long s, e;
    row_span(row_off, row, text_bytes, s, e);
    const TableView T = table_view(table, table_bytes);
    const long long at = out_off[row], end = out_off[row + 1];      // >= 0: sums of counts
    const long long room = capacity - at - add_special;             // tokens of this row in front of the capacity
    row_tokens(text, s, e, lane, T, unk_id, room, [&](long long t, int id) { out_ids[at + add_special + t] = id; });
    if (lane == 0 && add_special) {
        if (at < capacity) out_ids[at] = start_id;
        if (end - 1 < capacity) out_ids[end - 1] = end_id;
    }
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

extern "C" size_t i2l_tokenize_packed_workspace_bytes(int rows) {
    return i2l_align((size_t)(rows > 0 ? rows : 1) * sizeof(int32_t));
}

extern "C" int i2l_tokenize_packed(const uint8_t* text, int64_t text_bytes, const int32_t* row_off, int rows, const void* table,
                                   size_t table_bytes, int unk_id, int start_id, int end_id, int add_special, int32_t* out_ids,
                                   int64_t out_capacity, int64_t* out_off, int32_t* status, void* workspace,
                                   size_t workspace_bytes, i2l_stream_t stream) {
    if (text_bytes > 0x7fffffffLL || rows > 0x7fffffff - SCAN_T) return I2L_ERR_UNSUPPORTED;
    if (rows < 0 || text_bytes < 0 || out_capacity < 0 || (add_special != 0 && add_special != 1)) return I2L_ERR_ARG;
    if (!out_off || !status || (out_capacity > 0 && !out_ids)) return I2L_ERR_ARG;
    if (rows > 0 && (!row_off || !table || table_bytes < (size_t)HDR_WORDS * 4 || (text_bytes > 0 && !text))) return I2L_ERR_ARG;
    if (rows > 0 && (!workspace || workspace_bytes < i2l_tokenize_packed_workspace_bytes(rows))) return I2L_ERR_WORKSPACE;
    hipStream_t s = i2l_s(stream);
    int32_t* row_ids = static_cast<int32_t*>(workspace);
    const dim3 grid(i2l_cdiv(rows, TT / 64)), block(TT);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return I2L_ERR_LAUNCH;
    if (rows > 0) {
        hipLaunchKernelGGL(packed_count_kernel, grid, block, 0, s, text, (long long)text_bytes, row_off, rows,
                           static_cast<const int32_t*>(table), (long long)table_bytes, add_special, row_ids, status);
        I2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(packed_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, (const int32_t*)row_ids, rows, (long long)out_capacity,
                       out_off, status);
    I2L_CHECK_LAUNCH();
    if (rows > 0) {
        hipLaunchKernelGGL(packed_write_kernel, grid, block, 0, s, text, (long long)text_bytes, row_off, rows,
                           static_cast<const int32_t*>(table), (long long)table_bytes, unk_id, start_id, end_id, add_special,
                           (const int64_t*)out_off, out_ids, (long long)out_capacity);
        I2L_CHECK_LAUNCH();
    }
    return I2L_OK;
}
