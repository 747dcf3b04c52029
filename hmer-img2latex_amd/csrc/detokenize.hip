// Token ids -> packed UTF-8 text on the device: LaTeXTokenizer.decode (reference img2latex/data/tokenizer.py:166-192:
// drop the special ids, look every other id up, " ".join) on top of the predictor's END handling (training/predictor.py:
// 350-358,384-391: a row is cut before its first END).  The row rule is compact_ids_kernel's (metrics.hip); what is new
// is the text: row r becomes out_bytes[out_off[r] .. out_off[r + 1]).
//
// Three launches: (1) one wave per row adds up the row's bytes, (2) one workgroup turns the row totals into out_off
// (chunks of 1024 rows with a running carry: any number of rows), (3) one wave per row writes the bytes.  A kept token
// is a PIECE of the row: its separator (one 0x20 in front of every kept token but the row's first) followed by its
// bytes.  Per 64 positions a wave prefix sum of the piece lengths gives every piece its place; the writing pass then
// walks the OUTPUT bytes of those 64 pieces, lane = byte: each lane finds its piece by a 6-step search over the prefix
// sums (cross-lane reads, no LDS) and copies one byte, so neighbouring lanes store neighbouring bytes whatever the token
// lengths are (a lane per token would scatter 1 - 15 byte runs).
#include "common.h"

#include <vector>

namespace {

constexpr int DT = 256;                 // threads of the row kernels: four rows per workgroup
constexpr int SCAN_T = 1024;            // threads of the scan workgroup

struct Piece {
    int len;        // bytes of this lane's piece: separator + token; 0 = nothing kept at this position
    int src;        // tok_bytes index of the token's first byte
    int sep;        // 1: the piece begins with a separator
};

// The 64 positions base .. base + 63 of one row.  `kept` = tokens kept in the chunks before (the row's first kept token
// takes no separator).  Returns true when the row stops inside this chunk.  Wave-uniform control flow throughout.
__device__ __forceinline__ bool classify_chunk(const int32_t* __restrict__ src_ids, int width, int base, int lane, int end_id,
                                               const int (&d)[8], const int32_t* __restrict__ tok_off, int vocab, int unk_id,
                                               int& kept, Piece& p) {
    const int pos = base + lane;
    const int v = pos < width ? src_ids[pos] : -1;
    const bool stop = pos >= width || v < 0 || v == end_id;
    const unsigned long long stops = __ballot(stop);
    const int first_stop = stops ? __ffsll((long long)stops) - 1 : 64;
    bool keep = lane < first_stop;
#pragma unroll
    for (int j = 0; j < 8; ++j) keep = keep && v != d[j];
    const unsigned long long km = __ballot(keep);
    p.len = 0; p.src = 0; p.sep = 0;
    if (keep) {
        const int t = v < vocab ? v : unk_id;                       // v >= 0 here: a negative id stopped the row
        const int o0 = tok_off[t], o1 = tok_off[t + 1];
        p.sep = (kept + __popcll(km & ((1ull << lane) - 1ull))) > 0 ? 1 : 0;
        p.src = o0;
        p.len = (o1 - o0) + p.sep;
    }
    kept += __popcll(km);
    return first_stop < 64;
}

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}

__device__ __forceinline__ void load_drop(const int* __restrict__ drop, int n_drop, int (&d)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = j < n_drop ? drop[j] : -0x7fffffff;
}

__global__ __launch_bounds__(DT) void detok_size_kernel(const int32_t* __restrict__ ids, int rows, int width, int stride, int end_id,
                                                        const int* __restrict__ drop, int n_drop,
                                                        const int32_t* __restrict__ tok_off, int vocab, int unk_id,
                                                        int32_t* __restrict__ row_bytes) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int32_t* src = ids + (size_t)row * stride;
    int d[8];
    load_drop(drop, n_drop, d);
    int kept = 0, total = 0;                                       // total: the bytes of the chunks before, carried
    for (int base = 0; base < width; base += 64) {
        Piece p;
        const bool last = classify_chunk(src, width, base, lane, end_id, d, tok_off, vocab, unk_id, kept, p);
        total += __shfl(wave_inclusive_sum(p.len, lane), 63, 64);
        if (last) break;
    }
    if (lane == 0) row_bytes[row] = total;
}

// Exclusive scan of row_bytes into out_off[0 .. rows], out_off[rows] = the total; status = 1 iff it exceeds the capacity.
__global__ __launch_bounds__(SCAN_T) void detok_scan_kernel(const int32_t* __restrict__ row_bytes, int rows, long long capacity,
                                                            int32_t* __restrict__ out_off, int32_t* __restrict__ status) {
    __shared__ int wave_sum[SCAN_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < rows; base += SCAN_T) {
        const int r = base + tid;
        const int v = r < rows ? row_bytes[r] : 0;
        const int incl = wave_inclusive_sum(v, lane);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SCAN_T / 64; ++w) {
            const int s = wave_sum[w];
            before += w < wave ? s : 0;
            all += s;
        }
        if (r < rows) out_off[r] = carry + before + incl - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        out_off[rows] = carry;
        *status = (long long)carry > capacity ? 1 : 0;
    }
}

__global__ __launch_bounds__(DT) void detok_write_kernel(const int32_t* __restrict__ ids, int rows, int width, int stride, int end_id,
                                                         const int* __restrict__ drop, int n_drop,
                                                         const uint8_t* __restrict__ tok_bytes,
                                                         const int32_t* __restrict__ tok_off, int vocab, int unk_id,
                                                         const int32_t* __restrict__ out_off, uint8_t* __restrict__ out,
                                                         long long capacity) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (DT / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int32_t* src = ids + (size_t)row * stride;
    int d[8];
    load_drop(drop, n_drop, d);
    int kept = 0;
    long long at = out_off[row];                                   // where this chunk's bytes begin
    for (int base = 0; base < width; base += 64) {
        Piece p;
        const bool last = classify_chunk(src, width, base, lane, end_id, d, tok_off, vocab, unk_id, kept, p);
        const int incl = wave_inclusive_sum(p.len, lane);
        const int chunk_bytes = __shfl(incl, 63, 64);
        for (int b0 = 0; b0 < chunk_bytes; b0 += 64) {
            const int j = b0 + lane;                               // byte of this chunk; lanes past its end search too
            // the piece of byte j = the first lane whose inclusive sum exceeds j (an empty piece never is: its sum
            // equals its predecessor's); lower bound over 64 sorted values in 6 steps
            int lo = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                const int probe = __shfl(incl, lo + step - 1, 64);
                if (probe <= j) lo += step;
            }
            const int owner = min(lo, 63);
            const int o_incl = __shfl(incl, owner, 64), o_len = __shfl(p.len, owner, 64);
            const int o_src = __shfl(p.src, owner, 64), o_sep = __shfl(p.sep, owner, 64);
            const int k = j - (o_incl - o_len);                    // byte within the piece
            const long long g = at + j;
            if (j < chunk_bytes && g >= 0 && g < capacity)
                out[g] = k < o_sep ? (uint8_t)0x20 : tok_bytes[o_src + (k - o_sep)];
        }
        at += chunk_bytes;
        if (last) break;
    }
}

}  // namespace

extern "C" size_t i2l_detokenize_workspace_bytes(int rows) {
    return i2l_align((size_t)(rows > 0 ? rows : 1) * sizeof(int32_t));
}

extern "C" int i2l_detokenize(const int32_t* ids, int rows, int width, int stride, int end_id, const int32_t* drop_ids,
                              int n_drop, const uint8_t* tok_bytes, const int32_t* tok_off, int vocab, int unk_id,
                              uint8_t* out_bytes, int64_t out_capacity, int32_t* out_off, int32_t* status, void* workspace,
                              size_t workspace_bytes, i2l_stream_t stream) {
    if (n_drop > 8 || vocab <= 0) return I2L_ERR_UNSUPPORTED;
    if (!ids || !tok_bytes || !tok_off || !out_off || !status || rows <= 0 || width <= 0 || stride < width || n_drop < 0 ||
        (n_drop > 0 && !drop_ids) || unk_id < 0 || unk_id >= vocab || out_capacity < 0 || (out_capacity > 0 && !out_bytes))
        return I2L_ERR_ARG;
    // the longest token bounds every int32 byte count below, and tok_off lives on the device: it is read here (a
    // blocking copy of vocab + 1 words, no launch), which also refuses an offset table that is not ascending
    std::vector<int32_t> off((size_t)vocab + 1);
    if (hipMemcpy(off.data(), tok_off, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return I2L_ERR_LAUNCH;
    long long longest = 0;
    if (off[0] < 0) return I2L_ERR_ARG;
    for (int v = 0; v < vocab; ++v) {
        const long long n = (long long)off[v + 1] - off[v];
        if (n < 0) return I2L_ERR_ARG;
        longest = n > longest ? n : longest;
    }
    const long long worst = (long long)rows * width;               // <= 2^62
    if (worst > 0x7fffffffLL || worst * (longest + 1) > 0x7fffffffLL) return I2L_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < i2l_detokenize_workspace_bytes(rows)) return I2L_ERR_WORKSPACE;
    int32_t* row_bytes = static_cast<int32_t*>(workspace);
    hipStream_t s = i2l_s(stream);
    const dim3 grid(i2l_cdiv(rows, DT / 64)), block(DT);
    hipLaunchKernelGGL(detok_size_kernel, grid, block, 0, s, ids, rows, width, stride, end_id, drop_ids, n_drop, tok_off,
                       vocab, unk_id, row_bytes);
    I2L_CHECK_LAUNCH();
    hipLaunchKernelGGL(detok_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, (const int32_t*)row_bytes, rows,
                       (long long)out_capacity, out_off, status);
    I2L_CHECK_LAUNCH();
    hipLaunchKernelGGL(detok_write_kernel, grid, block, 0, s, ids, rows, width, stride, end_id, drop_ids, n_drop, tok_bytes,
                       tok_off, vocab, unk_id, (const int32_t*)out_off, out_bytes, (long long)out_capacity);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
