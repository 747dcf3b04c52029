// Packed UTF-8 text -> the fitted vocabulary on the device: LaTeXTokenizer.fit (reference img2latex/data/tokenizer.py:
// 80-117).  Tokens are what str.split() yields per row (text_scan.inc.h: the classifier, chunk scan and walk of
// tokenize.hip); they are ordered by count descending, ties by first occurrence in the corpus (Counter keeps insertion
// order, sorted() is stable) = the smallest global byte offset, so the sort key (count, first offset) is unique per token
// and nothing depends on scheduling.  Tokens equal to a skip string (the special tokens) are counted, not emitted.
//
// Count phase, one launch: a wave per row, lane = byte; the lane on a token's first byte walks and hashes it and finds
// or claims a slot of an open-addressing table in the workspace.  A slot's key is ONE 64-bit word, (offset << 32) |
// length of a representative occurrence in the input text, published by one compare-and-swap from 0 (a token has a
// byte, so no key is 0).  A lane that meets a claimed slot compares the length and then the text at the representative
// with its own: the text is immutable, nothing else is published, no lane ever waits for another.  Probes are bounded by
// the slot count.  Counts (atomicAdd) and first offsets (atomicMin) are gathered per workgroup in a small LDS table
// keyed by the global slot and flushed once at the end: a handful of tokens make up half of a formula corpus and their
// adds would otherwise queue on two or three words of L2.
//
// Order phase: compact the claimed slots (the skip strings drop out here) into (key = ~count << 32 | first offset,
// value = slot), bitonic sort of the next power of two (pads are all-ones keys; steps of distance < 1024 run inside an
// LDS tile, so 65536 entries take 21 launches and launches beyond the device-side count return at once), one workgroup
// scans the token lengths into offsets and writes the meta block, a thread per token copies its bytes out.
#include "common.h"

#include <string.h>

namespace {

#include "text_scan.inc.h"

constexpr int CT = 256;                         // count kernel: threads per workgroup, four rows at a time
constexpr int COUNT_GRID = 1024;                // persistent workgroups: each flushes its LDS table once
constexpr int LT = 1024;                        // LDS table entries (global slot + 1, count, first offset)
constexpr int LT_PROBES = 4;
constexpr unsigned SORT_TILE = 1024;            // entries sorted inside LDS by one workgroup of SORT_TILE / 2 threads
constexpr int SCAN_T = 1024;
constexpr int CTRL_WORDS = 64;                  // workspace head, see enum
constexpr int MAX_SKIP = 8, MAX_SKIP_BYTES = 256;
constexpr int64_t MAX_SLOTS = 1ll << 28;

enum { C_CLAIMED = 0, C_EMIT = 1, C_SKIPPED = 2, C_TOTAL = 3, C_LONGEST = 4, C_STATUS = 5, C_SKIP_COUNT = 8 };
enum { M_EMITTED = 0, M_SKIPPED = 1, M_TOTAL = 2, M_LONGEST = 3, M_BYTES = 4, M_STATUS = 5, M_SKIP_COUNT = 8 };

struct SkipSet {                                // by value in the kernel arguments
    int n;
    int off[MAX_SKIP + 1];
    uint8_t bytes[MAX_SKIP_BYTES];
};

struct Layout {                                 // byte offsets into the workspace
    size_t keys, cnt, first, sort_key, sort_val, total;
    size_t sort_n;                              // entries of the sort arrays: max(slots / 2, SORT_TILE)
};

Layout layout(size_t slots) {
    Layout l;
    l.sort_n = slots / 2 > SORT_TILE ? slots / 2 : SORT_TILE;
    l.keys = (size_t)CTRL_WORDS * 4;            // zeroed: ctrl, keys, cnt
    l.cnt = l.keys + 8 * slots;
    l.first = l.cnt + 4 * slots;                // all ones: first, sort_key
    l.sort_key = l.first + 4 * slots;           // 256 + 16 * slots: 8-byte aligned
    l.sort_val = l.sort_key + 8 * l.sort_n;
    l.total = l.sort_val + 4 * l.sort_n;
    return l;
}

__device__ inline bool same_bytes(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, long long n) {
    long long k = 0;
    while (k < n && a[k] == b[k]) ++k;
    return k == n;
}

template <bool AGG>
__global__ __launch_bounds__(CT) void count_kernel(const uint8_t* __restrict__ text, long long text_bytes,
                                                   const int32_t* __restrict__ row_off, int rows,
                                                   unsigned long long* keys, uint32_t* cnt, uint32_t* first,
                                                   long long n_slots, int32_t* ctrl) {
    __shared__ uint32_t l_tag[AGG ? LT : 1], l_cnt[AGG ? LT : 1], l_first[AGG ? LT : 1];
    __shared__ int l_total, l_longest, l_status;
    if (AGG)
        for (int i = threadIdx.x; i < LT; i += CT) {
            l_tag[i] = 0u;
            l_cnt[i] = 0u;
            l_first[i] = 0xffffffffu;
        }
    if (threadIdx.x == 0) l_total = l_longest = l_status = 0;
    __syncthreads();

    const int lane = threadIdx.x & 63;
    const uint32_t mask = (uint32_t)(n_slots - 1);
    int flags = 0, claimed = 0;
    for (long long row = (long long)blockIdx.x * (CT / 64) + (threadIdx.x >> 6); row < rows;
         row += (long long)gridDim.x * (CT / 64)) {
        long long s = row_off[row], e = row_off[row + 1];
        if (s < 0 || e < s || e > text_bytes) {                      // unusable offsets: an empty row, nothing is read
            s = e = 0;
            flags |= I2L_VOCAB_FIT_BAD_OFFSETS;
        }
        int n_tok = 0;
        ChunkScan scan;
        for (long long base = s; base < e; base += 64) {
            const long long p = base + lane;
            if (scan.step(text, base, e, lane)) {
                uint32_t h;
                const long long len = token_walk(text, p, e, scan.c0, scan.c1, scan.c2, 0x7fffffffffffffffLL, h);
                const unsigned long long mine = ((unsigned long long)p << 32) | (unsigned long long)len;
                uint32_t sl = first_slot(h, mask);
                bool found = false;
                for (long long probe = 0; probe < n_slots; ++probe) {
                    unsigned long long k = __hip_atomic_load(&keys[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (k == 0ull) {
                        k = atomicCAS(&keys[sl], 0ull, mine);        // the one publication: (offset, length) in one word
                        if (k == 0ull) {
                            ++claimed;
                            found = true;
                            break;
                        }
                    }
                    if ((long long)(k & 0xffffffffull) == len && same_bytes(text + (k >> 32), text + p, len)) {
                        found = true;
                        break;
                    }
                    sl = (sl + 1) & mask;
                }
                if (!found) {
                    flags |= I2L_VOCAB_FIT_FULL;
                } else {
                    bool local = false;
                    if (AGG) {
                        const uint32_t tag = sl + 1u;
                        for (int t = 0; t < LT_PROBES && !local; ++t) {
                            const uint32_t j = (sl + t) & (LT - 1);
                            const uint32_t prev = atomicCAS(&l_tag[j], 0u, tag);
                            if (prev == 0u || prev == tag) {
                                atomicAdd(&l_cnt[j], 1u);
                                atomicMin(&l_first[j], (uint32_t)p);
                                local = true;
                            }
                        }
                    }
                    if (!local) {                                    // no room in the LDS table (or the ablation): straight to L2
                        atomicAdd(&cnt[sl], 1u);
                        atomicMin(&first[sl], (uint32_t)p);
                    }
                }
            }
            n_tok += __popcll(scan.starts);
        }
        if (lane == 0) {
            atomicAdd(&l_total, n_tok);
            atomicMax(&l_longest, n_tok);
        }
    }
    if (claimed) atomicAdd(&ctrl[C_CLAIMED], claimed);
    if (flags) atomicOr(&l_status, flags);
    __syncthreads();
    if (AGG)
        for (int i = threadIdx.x; i < LT; i += CT)
            if (l_tag[i]) {
                atomicAdd(&cnt[l_tag[i] - 1u], l_cnt[i]);
                atomicMin(&first[l_tag[i] - 1u], l_first[i]);
            }
    if (threadIdx.x == 0) {
        if (l_total) atomicAdd(&ctrl[C_TOTAL], l_total);
        if (l_longest) atomicMax(&ctrl[C_LONGEST], l_longest);
        if (l_status) atomicOr(&ctrl[C_STATUS], l_status);
    }
}

// a thread per slot: a claimed slot is a skip string (its count goes to the control block) or one entry of the sort
__global__ __launch_bounds__(256) void compact_kernel(const uint8_t* __restrict__ text, const unsigned long long* __restrict__ keys,
                                                      const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ first,
                                                      long long n_slots, SkipSet skip, unsigned long long* sort_key,
                                                      uint32_t* sort_val, unsigned cap, int32_t* ctrl) {
    __shared__ SkipSet sk;
    for (unsigned i = threadIdx.x; i < sizeof(SkipSet) / 4; i += blockDim.x)
        reinterpret_cast<uint32_t*>(&sk)[i] = reinterpret_cast<const uint32_t*>(&skip)[i];
    __syncthreads();
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const unsigned long long k = keys[s];
    if (k == 0ull) return;
    const int len = (int)(k & 0xffffffffull);
    const uint8_t* tok = text + (k >> 32);
    for (int i = 0; i < sk.n; ++i) {
        if (sk.off[i + 1] - sk.off[i] != len) continue;
        int b = 0;
        while (b < len && sk.bytes[sk.off[i] + b] == tok[b]) ++b;
        if (b == len) {
            ctrl[C_SKIP_COUNT + i] = (int32_t)cnt[s];
            atomicAdd(&ctrl[C_SKIPPED], 1);
            return;
        }
    }
    const unsigned idx = (unsigned)atomicAdd(&ctrl[C_EMIT], 1);
    if (idx < cap) {                                                 // beyond cap the table was over-full: FULL is reported
        sort_key[idx] = ((unsigned long long)(~cnt[s]) << 32) | first[s];
        sort_val[idx] = (uint32_t)s;
    }
}

// the sort's length: the power of two (>= one tile) that holds the compacted entries; the rest of the arrays is not touched
__device__ inline unsigned sort_len(const int32_t* ctrl, unsigned cap) {
    const unsigned found = (unsigned)ctrl[C_EMIT], n = found < cap ? found : cap;
    unsigned m = SORT_TILE;
    while (m < n) m <<= 1;
    return m;
}

// bitonic steps inside one tile: for k = k_first, 2 k_first .. k_last the distances min(k / 2, SORT_TILE / 2) .. 1
__global__ __launch_bounds__(SORT_TILE / 2) void sort_tile_kernel(unsigned long long* sort_key, uint32_t* sort_val,
                                                                  const int32_t* __restrict__ ctrl, unsigned cap,
                                                                  unsigned k_first, unsigned k_last) {
    __shared__ unsigned long long sk[SORT_TILE];
    __shared__ uint32_t sv[SORT_TILE];
    const unsigned m = sort_len(ctrl, cap), base = blockIdx.x * SORT_TILE, t = threadIdx.x;
    if (base >= m || k_first > m) return;                            // uniform per workgroup
    sk[t] = sort_key[base + t];
    sv[t] = sort_val[base + t];
    sk[t + SORT_TILE / 2] = sort_key[base + t + SORT_TILE / 2];
    sv[t + SORT_TILE / 2] = sort_val[base + t + SORT_TILE / 2];
    __syncthreads();
    for (unsigned k = k_first; k <= k_last && k <= m; k <<= 1) {
        for (unsigned j = (k >> 1) < SORT_TILE / 2 ? (k >> 1) : SORT_TILE / 2; j > 0; j >>= 1) {
            const unsigned a = 2 * t - (t & (j - 1)), b = a + j;
            const bool up = ((base + a) & k) == 0;
            const unsigned long long ka = sk[a], kb = sk[b];
            if ((ka > kb) == up) {
                sk[a] = kb;
                sk[b] = ka;
                const uint32_t va = sv[a];
                sv[a] = sv[b];
                sv[b] = va;
            }
            __syncthreads();
        }
    }
    sort_key[base + t] = sk[t];
    sort_val[base + t] = sv[t];
    sort_key[base + t + SORT_TILE / 2] = sk[t + SORT_TILE / 2];
    sort_val[base + t + SORT_TILE / 2] = sv[t + SORT_TILE / 2];
}

// one bitonic step of distance j >= SORT_TILE in global memory; a thread per pair
__global__ __launch_bounds__(256) void sort_step_kernel(unsigned long long* sort_key, uint32_t* sort_val,
                                                        const int32_t* __restrict__ ctrl, unsigned cap, unsigned k, unsigned j) {
    const unsigned m = sort_len(ctrl, cap), t = blockIdx.x * 256u + threadIdx.x;
    if (k > m || t >= m / 2) return;
    const unsigned a = 2 * t - (t & (j - 1)), b = a + j;
    const bool up = (a & k) == 0;
    const unsigned long long ka = sort_key[a], kb = sort_key[b];
    if ((ka > kb) == up) {
        sort_key[a] = kb;
        sort_key[b] = ka;
        const uint32_t va = sort_val[a];
        sort_val[a] = sort_val[b];
        sort_val[b] = va;
    }
}

// ONE workgroup: exclusive scan of the token lengths in rank order -> out_off, then the meta block
__global__ __launch_bounds__(SCAN_T) void offsets_kernel(const unsigned long long* __restrict__ keys,
                                                         const uint32_t* __restrict__ sort_val, unsigned cap,
                                                         long long n_slots, const int32_t* __restrict__ ctrl,
                                                         int32_t* __restrict__ out_off, int out_capacity,
                                                         long long out_byte_capacity, int32_t* __restrict__ meta) {
    __shared__ long long part[SCAN_T];
    const unsigned found = (unsigned)ctrl[C_EMIT], n = found < cap ? found : cap, t = threadIdx.x;
    const unsigned per = (n + SCAN_T - 1) / SCAN_T, lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    long long sum = 0;
    for (unsigned r = lo; r < hi; ++r) sum += (long long)(keys[sort_val[r]] & 0xffffffffull);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int i = 0; i < SCAN_T; ++i) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
        // distinct tokens occupy disjoint bytes of the text: run <= text_bytes < 2^31
        int status = ctrl[C_STATUS];
        if ((long long)ctrl[C_CLAIMED] > n_slots / 2) status |= I2L_VOCAB_FIT_FULL;
        if (found > (unsigned)out_capacity || run > out_byte_capacity) status |= I2L_VOCAB_FIT_OUT_TOO_SMALL;
        meta[M_EMITTED] = (int32_t)found;
        meta[M_SKIPPED] = ctrl[C_SKIPPED];
        meta[M_TOTAL] = ctrl[C_TOTAL];
        meta[M_LONGEST] = ctrl[C_LONGEST];
        meta[M_BYTES] = (int32_t)run;
        meta[M_STATUS] = status;
        meta[6] = meta[7] = 0;
        for (int i = 0; i < MAX_SKIP; ++i) meta[M_SKIP_COUNT + i] = ctrl[C_SKIP_COUNT + i];
        if (n <= (unsigned)out_capacity) out_off[n] = (int32_t)run;
    }
    __syncthreads();
    long long o = part[t];
    for (unsigned r = lo; r < hi; ++r) {
        if (r <= (unsigned)out_capacity) out_off[r] = (int32_t)o;    // out_off has out_capacity + 1 words
        o += (long long)(keys[sort_val[r]] & 0xffffffffull);
    }
}

// a thread per emitted token: count, first offset, bytes (none at or beyond out_byte_capacity)
__global__ __launch_bounds__(256) void emit_kernel(const uint8_t* __restrict__ text, const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ sort_val, unsigned cap,
                                                   const int32_t* __restrict__ ctrl, const int32_t* __restrict__ out_off,
                                                   int out_capacity, uint8_t* __restrict__ out_bytes,
                                                   long long out_byte_capacity, int32_t* __restrict__ out_count,
                                                   int32_t* __restrict__ out_first) {
    const unsigned found = (unsigned)ctrl[C_EMIT];
    unsigned n = found < cap ? found : cap;
    if (n > (unsigned)out_capacity) n = (unsigned)out_capacity;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t s = sort_val[r];
    const unsigned long long k = keys[s];
    const long long len = (long long)(k & 0xffffffffull), o = out_off[r];
    const uint8_t* tok = text + (k >> 32);
    out_count[r] = (int32_t)cnt[s];
    out_first[r] = (int32_t)first[s];
    for (long long i = 0; i < len && o + i < out_byte_capacity; ++i) out_bytes[o + i] = tok[i];
}

bool usable_slots(int64_t slots) { return slots >= 2 && slots <= MAX_SLOTS && (slots & (slots - 1)) == 0; }

}  // namespace

extern "C" size_t i2l_vocab_fit_workspace_bytes(int rows, int64_t slots) {
    if (rows < 0 || !usable_slots(slots)) return 0;
    return layout((size_t)slots).total;
}

extern "C" int i2l_vocab_fit(const uint8_t* text, int64_t text_bytes, const int32_t* row_off, int rows,
                             const uint8_t* skip_bytes, const int32_t* skip_off, int n_skip, int64_t slots, int flags,
                             uint8_t* out_bytes, int64_t out_byte_capacity, int32_t* out_off, int32_t* out_count,
                             int32_t* out_first, int out_capacity, int32_t* meta, void* workspace, size_t workspace_bytes,
                             i2l_stream_t stream) {
    if (text_bytes > 0x7fffffffLL || n_skip > MAX_SKIP) return I2L_ERR_UNSUPPORTED;
    if (rows < 0 || text_bytes < 0 || n_skip < 0 || out_capacity < 0 || out_byte_capacity < 0 || !usable_slots(slots) ||
        (flags & ~I2L_VOCAB_FIT_NO_AGGREGATE) != 0)
        return I2L_ERR_ARG;
    if (!row_off || !out_off || !meta || (text_bytes > 0 && !text) || (n_skip > 0 && !skip_off) ||
        (out_capacity > 0 && (!out_count || !out_first)) || (out_byte_capacity > 0 && !out_bytes))
        return I2L_ERR_ARG;
    SkipSet skip;
    memset(&skip, 0, sizeof(skip));
    skip.n = n_skip;
    for (int i = 0; i < n_skip; ++i) {
        const long long a = skip_off[i], b = skip_off[i + 1];
        if (a < skip_off[0] || b < a) return I2L_ERR_ARG;
        if (b - skip_off[0] > MAX_SKIP_BYTES) return I2L_ERR_UNSUPPORTED;
        skip.off[i] = (int)(a - skip_off[0]);
        skip.off[i + 1] = (int)(b - skip_off[0]);
    }
    if (skip.off[n_skip] > 0) {
        if (!skip_bytes) return I2L_ERR_ARG;
        memcpy(skip.bytes, skip_bytes + skip_off[0], (size_t)skip.off[n_skip]);
    }
    const Layout l = layout((size_t)slots);
    if (!workspace || workspace_bytes < l.total) return I2L_ERR_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return I2L_ERR_ARG;

    hipStream_t s = i2l_s(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    int32_t* ctrl = reinterpret_cast<int32_t*>(ws);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws + l.keys);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(ws + l.cnt);
    uint32_t* first = reinterpret_cast<uint32_t*>(ws + l.first);
    unsigned long long* sort_key = reinterpret_cast<unsigned long long*>(ws + l.sort_key);
    uint32_t* sort_val = reinterpret_cast<uint32_t*>(ws + l.sort_val);
    const unsigned cap = (unsigned)(slots / 2), sort_n = (unsigned)l.sort_n;

    if (hipMemsetAsync(ws, 0, l.first, s) != hipSuccess) return I2L_ERR_LAUNCH;
    if (hipMemsetAsync(ws + l.first, 0xff, l.sort_val - l.first, s) != hipSuccess) return I2L_ERR_LAUNCH;
    if (rows > 0) {
        const int grid = i2l_cdiv(rows, CT / 64) < COUNT_GRID ? i2l_cdiv(rows, CT / 64) : COUNT_GRID;
        if (flags & I2L_VOCAB_FIT_NO_AGGREGATE)
            hipLaunchKernelGGL(count_kernel<false>, dim3(grid), dim3(CT), 0, s, text, (long long)text_bytes, row_off, rows,
                               keys, cnt, first, (long long)slots, ctrl);
        else
            hipLaunchKernelGGL(count_kernel<true>, dim3(grid), dim3(CT), 0, s, text, (long long)text_bytes, row_off, rows,
                               keys, cnt, first, (long long)slots, ctrl);
        I2L_CHECK_LAUNCH();
        hipLaunchKernelGGL(compact_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, text, keys, cnt, first,
                           (long long)slots, skip, sort_key, sort_val, cap, ctrl);
        I2L_CHECK_LAUNCH();
        hipLaunchKernelGGL(sort_tile_kernel, dim3(sort_n / SORT_TILE), dim3(SORT_TILE / 2), 0, s, sort_key, sort_val, ctrl, cap,
                           2u, SORT_TILE);
        for (unsigned k = 2 * SORT_TILE; k <= sort_n; k <<= 1) {
            for (unsigned j = k >> 1; j >= SORT_TILE; j >>= 1)
                hipLaunchKernelGGL(sort_step_kernel, dim3(sort_n / 512), dim3(256), 0, s, sort_key, sort_val, ctrl, cap, k, j);
            hipLaunchKernelGGL(sort_tile_kernel, dim3(sort_n / SORT_TILE), dim3(SORT_TILE / 2), 0, s, sort_key, sort_val, ctrl,
                               cap, k, k);
        }
        I2L_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(SCAN_T), 0, s, keys, sort_val, cap, (long long)slots, ctrl, out_off,
                       out_capacity, (long long)out_byte_capacity, meta);
    I2L_CHECK_LAUNCH();
    if (rows > 0 && out_capacity > 0) {
        const unsigned n_max = cap < (unsigned)out_capacity ? cap : (unsigned)out_capacity;
        hipLaunchKernelGGL(emit_kernel, dim3((n_max + 255) / 256), dim3(256), 0, s, text, keys, cnt, first, sort_val, cap, ctrl,
                           out_off, out_capacity, out_bytes, (long long)out_byte_capacity, out_count, out_first);
        I2L_CHECK_LAUNCH();
    }
    return I2L_OK;
}
