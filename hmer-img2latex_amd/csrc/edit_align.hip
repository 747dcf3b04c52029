// Error analysis on the device: the edit script of every (target, prediction) pair and the token confusion matrix of a
// whole split (i2l_edit_alignment), its margins (i2l_confusion_margins) and its largest cells (i2l_confusion_top).  The
// rules -- which script is THE script, what it adds to the matrix -- are edit_align_rules.inc.h's; this file holds the
// kernels' glue: who loads what, where the bit vectors live, how the cells are scanned and sorted.
#include "common.h"
#include "edit_align_rules.inc.h"

namespace {

constexpr int EA_LDS_VEC_BYTES = 16 * 1024;     // the columns' bit vectors stay in LDS up to here (256 x 256 tokens)

// blocks of 64 target rows the kernel is instantiated for
int ea_blocks(int target_stride) {
    const int w = (target_stride + 63) / 64;
    return w <= 1 ? 1 : w <= 2 ? 2 : w <= 3 ? 3 : w <= 4 ? 4 : w <= 8 ? 8 : 16;
}
size_t ea_vec_bytes(int pred_stride, int target_stride) {
    return (size_t)pred_stride * ea_blocks(target_stride) * 2 * sizeof(ea_u64);
}
size_t ea_pair_scratch(int pred_stride, int target_stride) {
    const size_t b = ea_vec_bytes(pred_stride, target_stride);
    return b <= (size_t)EA_LDS_VEC_BYTES ? 0 : b;
}

// One wave per pair.  The target's tokens sit in registers (lane = row within a block of 64, W blocks); per prediction
// token a ballot yields a block's match mask, ea_block_step turns it into the column's vectors, and lane 0 stores the
// two the backtrace needs.  Lane 0 then walks back from (m, n) -- at most m + n steps of two loads -- and the wave
// writes the script out in forward order.  LDS: [vec when it fits] | r | p | the reversed script | len.  IN_LDS is a
// template argument so that the vectors' loads and stores are LDS or global instructions, not flat ones.
template <int W, bool IN_LDS>
__global__ __launch_bounds__(64) void edit_align_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ pred_len,
                                                        int pred_stride, const int32_t* __restrict__ tgt,
                                                        const int32_t* __restrict__ tgt_len, int tgt_stride, int V,
                                                        ea_u64* __restrict__ scratch, size_t pair_scratch_words,
                                                        int32_t* __restrict__ ops_out, uint8_t* __restrict__ script_out,
                                                        int32_t* __restrict__ script_len_out, uint32_t* __restrict__ C) {
    extern __shared__ ea_u64 sm64[];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(pred_len[pair], 0), pred_stride), m = min(max(tgt_len[pair], 0), tgt_stride);
    const size_t lds_vec_words = IN_LDS ? (size_t)pred_stride * W * 2 : 0;
    ea_u64* vec = IN_LDS ? sm64 : scratch + (size_t)pair * pair_scratch_words;
    int32_t* r = reinterpret_cast<int32_t*>(sm64 + lds_vec_words);
    int32_t* p = r + tgt_stride;
    int32_t* meta = p + pred_stride;                        // [0..3] ops, [4] len
    uint8_t* rev = reinterpret_cast<uint8_t*>(meta + 8);
    for (int i = lane; i < m; i += 64) r[i] = tgt[(size_t)pair * tgt_stride + i];
    for (int i = lane; i < n; i += 64) p[i] = pred[(size_t)pair * pred_stride + i];
    __syncthreads();
    if (m > 0 && n > 0) {
        int ra[W];
        bool ok[W];
        ea_u64 Pv[W], Mv[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            ok[w] = 64 * w + lane < m;
            ra[w] = ok[w] ? r[64 * w + lane] : 0;
            Pv[w] = ~0ull;
            Mv[w] = 0ull;
        }
        const int last = (m - 1) >> 6;
        for (int j = 0; j < n; ++j) {
            const int t = p[j];
            ea_u64* col = vec + (size_t)j * W * 2;
            int hin = 1;                                    // D[0][j+1] - D[0][j]
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (w <= last) {
                    const ea_u64 eq = __ballot(ok[w] && ra[w] == t);
                    ea_u64 d0;
                    hin = ea_block_step(eq, Pv[w], Mv[w], hin, d0);
                    if (lane == 0) { col[2 * w] = Pv[w]; col[2 * w + 1] = d0; }
                }
            }
        }
    }
    __syncthreads();
    if (lane == 0) meta[4] = ea_walk(r, m, p, n, EaBitCells{vec, W}, V, rev, meta, C);   // reads what lane 0 itself stored
    __syncthreads();
    if (ops_out && lane < 4) ops_out[(size_t)pair * 4 + lane] = meta[lane];
    if (script_out) {
        const int len = meta[4];
        uint8_t* dst = script_out + (size_t)pair * ((size_t)pred_stride + tgt_stride);
        for (int k = lane; k < len; k += 64) dst[k] = rev[len - 1 - k];
        if (lane == 0) script_len_out[pair] = len;
    }
}

// ------------------------------------------------------------------------------------------------ margins
// One wave per row a: row_total[a] = sum_b C[a][b], and diag[a] = C[a][a] for a < V.
__global__ __launch_bounds__(256) void confusion_rows_kernel(const uint32_t* __restrict__ C, int V, uint32_t* __restrict__ row_total,
                                                             uint32_t* __restrict__ diag) {
    const int lane = threadIdx.x & 63, a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a > V) return;
    const uint32_t* row = C + (size_t)a * (V + 1);
    uint32_t s = 0;
    for (int b = lane; b <= V; b += 64) s += row[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) {
        if (row_total) row_total[a] = s;
        if (diag && a < V) diag[a] = row[a];
    }
}

// 64 columns per workgroup, the rows dealt to its four waves: col_total[b] = sum_a C[a][b].
__global__ __launch_bounds__(256) void confusion_cols_kernel(const uint32_t* __restrict__ C, int V, uint32_t* __restrict__ col_total) {
    __shared__ uint32_t part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x * 64 + lane;
    uint32_t s = 0;
    if (b <= V)
        for (int a = wave; a <= V; a += 4) s += C[(size_t)a * (V + 1) + b];
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && b <= V) col_total[b] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}

// ------------------------------------------------------------------------------------------------ top cells
constexpr int TOP_T = 1024;                     // threads of a workgroup = the longest list
constexpr int TOP_MAX_GROUPS = 128;
constexpr int TOP_CELLS_PER_GROUP = 16 * TOP_T;

int top_groups(int vocab) {
    const long cells = ((long)vocab + 1) * ((long)vocab + 1);
    const long g = (cells + TOP_CELLS_PER_GROUP - 1) / TOP_CELLS_PER_GROUP;
    return (int)(g < 1 ? 1 : g > TOP_MAX_GROUPS ? TOP_MAX_GROUPS : g);
}

// A cell's key: the count above the complement of its index, so that the larger key is the cell listed first (count
// descending, then row ascending, then column ascending) and no two cells share one.  0: not a candidate.
__device__ __forceinline__ ea_u64 top_key(const uint32_t* __restrict__ C, int V, int kinds, long idx) {
    const int row = (int)(idx / (V + 1)), col = (int)(idx % (V + 1));
    const int kind = row == V ? (col == V ? 0 : I2L_CONFUSION_INSERTIONS)
                              : (col == V ? I2L_CONFUSION_DELETIONS
                                          : (row == col ? I2L_CONFUSION_MATCHES : I2L_CONFUSION_SUBSTITUTIONS));
    if (!(kind & kinds)) return 0ull;
    const uint32_t c = C[idx];
    return c ? ((ea_u64)c << 32) | (ea_u64)(0xffffffffu - (uint32_t)idx) : 0ull;
}

// Bitonic sort of keys[0, 2 TOP_T), descending, by TOP_T threads.
__device__ void top_sort(ea_u64* keys, int tid) {
    for (int k = 2; k <= 2 * TOP_T; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i | j;
            const bool desc = (i & k) == 0;
            const ea_u64 a = keys[i], b = keys[l];
            if (desc ? a < b : a > b) { keys[i] = b; keys[l] = a; }
            __syncthreads();
        }
    }
}

// The n largest keys of src(begin .. end) into keys[0, n), descending (0 where there are fewer).  keys[0, TOP_T) is the
// list so far, sorted; a key enters keys[TOP_T, 2 TOP_T) only if it beats the list's n-th, and a sort of both halves
// merges the candidates of a pass in -- rarely, once the list's n-th key has risen.
template <class Src>
__device__ void top_scan(ea_u64* keys, int* cand, int n, long begin, long end, const Src& src) {
    const int tid = threadIdx.x;
    keys[tid] = 0ull;
    keys[TOP_T + tid] = 0ull;
    if (tid == 0) *cand = 0;
    __syncthreads();
    for (long base = begin; base < end; base += TOP_T) {
        const long idx = base + tid;
        const ea_u64 key = idx < end ? src(idx) : 0ull;
        const bool in = key > keys[n - 1];
        if (in) keys[TOP_T + atomicAdd(cand, 1)] = key;
        const int c = __syncthreads_count(in);              // uniform, and the candidates' stores are done
        if (c > 0) {
            if (tid >= c) keys[TOP_T + tid] = 0ull;
            if (tid == 0) *cand = 0;
            __syncthreads();
            top_sort(keys, tid);                            // ends on a barrier
        }
    }
}

__global__ __launch_bounds__(TOP_T) void confusion_top_groups_kernel(const uint32_t* __restrict__ C, int V, int kinds, int n,
                                                                     ea_u64* __restrict__ lists) {
    __shared__ ea_u64 keys[2 * TOP_T];
    __shared__ int cand;
    const long cells = ((long)V + 1) * ((long)V + 1);
    const long per = (cells + gridDim.x - 1) / gridDim.x;
    const long begin = per * blockIdx.x, end = begin + per < cells ? begin + per : cells;
    top_scan(keys, &cand, n, begin, end, [=](long idx) { return top_key(C, V, kinds, idx); });
    lists[(size_t)blockIdx.x * TOP_T + threadIdx.x] = keys[threadIdx.x];
}

__global__ __launch_bounds__(TOP_T) void confusion_top_merge_kernel(const ea_u64* __restrict__ lists, int groups, int V, int n,
                                                                    int32_t* __restrict__ row_out, int32_t* __restrict__ col_out,
                                                                    uint32_t* __restrict__ count_out, int32_t* __restrict__ listed_out) {
    __shared__ ea_u64 keys[2 * TOP_T];
    __shared__ int cand;
    const int tid = threadIdx.x;
    top_scan(keys, &cand, n, 0, (long)groups * TOP_T, [=](long idx) { return lists[idx]; });
    const ea_u64 key = tid < n ? keys[tid] : 0ull;
    const int listed = __syncthreads_count(key != 0ull);
    if (tid < n) {
        const uint32_t idx = 0xffffffffu - (uint32_t)key;
        row_out[tid] = key ? (int32_t)(idx / (uint32_t)(V + 1)) : -1;
        col_out[tid] = key ? (int32_t)(idx % (uint32_t)(V + 1)) : -1;
        count_out[tid] = (uint32_t)(key >> 32);
    }
    if (tid == 0) *listed_out = listed;
}

}  // namespace

extern "C" size_t i2l_edit_alignment_scratch_bytes(int pairs, int pred_stride, int target_stride) {
    if (pairs <= 0 || pred_stride <= 0 || target_stride <= 0 || pred_stride > EA_MAX_STRIDE || target_stride > EA_MAX_STRIDE)
        return 0;
    return (size_t)pairs * ea_pair_scratch(pred_stride, target_stride);
}

extern "C" int i2l_edit_alignment(const int32_t* pred, const int32_t* pred_len, int pred_stride, const int32_t* target,
                                  const int32_t* target_len, int target_stride, int pairs, int vocab, void* scratch,
                                  size_t scratch_bytes, int32_t* ops_out, uint8_t* script_out, int32_t* script_len_out,
                                  uint32_t* confusion, i2l_stream_t stream) {
    if (!pred || !pred_len || !target || !target_len || pairs <= 0 || pred_stride <= 0 || target_stride <= 0 || vocab <= 0 ||
        (script_out == nullptr) != (script_len_out == nullptr) || (!ops_out && !script_out && !confusion))
        return I2L_ERR_ARG;
    if (pred_stride > EA_MAX_STRIDE || target_stride > EA_MAX_STRIDE || vocab > EA_MAX_VOCAB) return I2L_ERR_UNSUPPORTED;
    const size_t per_pair = ea_pair_scratch(pred_stride, target_stride);
    if (per_pair && (!scratch || scratch_bytes < (size_t)pairs * per_pair)) return I2L_ERR_WORKSPACE;
    const int W = ea_blocks(target_stride);
    const size_t lds = (per_pair ? 0 : ea_vec_bytes(pred_stride, target_stride)) +
                       ((size_t)pred_stride + target_stride + 8) * sizeof(int32_t) +
                       i2l_align((size_t)pred_stride + target_stride, 8);
    hipStream_t s = i2l_s(stream);
#define I2L_EA_AT(W_, LDS_) hipLaunchKernelGGL((edit_align_kernel<W_, LDS_>), dim3(pairs), dim3(64), lds, s, pred, pred_len, \
                                               pred_stride, target, target_len, target_stride, vocab,                      \
                                               static_cast<ea_u64*>(scratch), per_pair / sizeof(ea_u64), ops_out,          \
                                               script_out, script_len_out, confusion)
#define I2L_EA(W_) do { if (per_pair) I2L_EA_AT(W_, false); else I2L_EA_AT(W_, true); } while (0)
    switch (W) {
        case 1: I2L_EA(1); break;
        case 2: I2L_EA(2); break;
        case 3: I2L_EA(3); break;
        case 4: I2L_EA(4); break;
        case 8: I2L_EA(8); break;
        default: I2L_EA(16); break;
    }
#undef I2L_EA
#undef I2L_EA_AT
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

extern "C" int i2l_confusion_margins(const uint32_t* confusion, int vocab, uint32_t* row_total, uint32_t* col_total,
                                     uint32_t* diag, i2l_stream_t stream) {
    if (!confusion || vocab <= 0 || (!row_total && !col_total && !diag)) return I2L_ERR_ARG;
    if (vocab > EA_MAX_VOCAB) return I2L_ERR_UNSUPPORTED;
    hipStream_t s = i2l_s(stream);
    if (row_total || diag) {
        hipLaunchKernelGGL(confusion_rows_kernel, dim3(i2l_cdiv(vocab + 1, 4)), dim3(256), 0, s, confusion, vocab, row_total, diag);
        I2L_CHECK_LAUNCH();
    }
    if (col_total) {
        hipLaunchKernelGGL(confusion_cols_kernel, dim3(i2l_cdiv(vocab + 1, 64)), dim3(256), 0, s, confusion, vocab, col_total);
        I2L_CHECK_LAUNCH();
    }
    return I2L_OK;
}

extern "C" size_t i2l_confusion_top_scratch_bytes(int vocab) {
    if (vocab <= 0 || vocab > EA_MAX_VOCAB) return 0;
    return (size_t)top_groups(vocab) * TOP_T * sizeof(ea_u64);
}

extern "C" int i2l_confusion_top(const uint32_t* confusion, int vocab, int kinds, int n, void* scratch, size_t scratch_bytes,
                                 int32_t* row_out, int32_t* col_out, uint32_t* count_out, int32_t* listed_out,
                                 i2l_stream_t stream) {
    if (!confusion || vocab <= 0 || n <= 0 || !row_out || !col_out || !count_out || !listed_out || kinds <= 0 ||
        (kinds & ~I2L_CONFUSION_ALL))
        return I2L_ERR_ARG;
    if (vocab > EA_MAX_VOCAB || n > TOP_T) return I2L_ERR_UNSUPPORTED;
    if (!scratch || scratch_bytes < i2l_confusion_top_scratch_bytes(vocab)) return I2L_ERR_WORKSPACE;
    const int groups = top_groups(vocab);
    ea_u64* lists = static_cast<ea_u64*>(scratch);
    hipStream_t s = i2l_s(stream);
    hipLaunchKernelGGL(confusion_top_groups_kernel, dim3(groups), dim3(TOP_T), 0, s, confusion, vocab, kinds, n, lists);
    I2L_CHECK_LAUNCH();
    hipLaunchKernelGGL(confusion_top_merge_kernel, dim3(1), dim3(TOP_T), 0, s, (const ea_u64*)lists, groups, vocab, n, row_out,
                       col_out, count_out, listed_out);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
