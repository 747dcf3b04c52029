// The two per-batch kernels of the device-resident data set (img2latex_amd/data/dataset.py).  The corpus is tokenized
// once into a CSR store (i2l_tokenize_packed, tokenize.hip) and the pages are decoded and uploaded once into one uint8
// buffer; a batch is then an index list:
//
//   i2l_collate_ids       Im2LatexCollator (reference img2latex/data/dataset.py:59-66) from the CSR store: row b of the
//                         batch is store row index[b], padded with PAD to the batch's width.  One launch, a wave per
//                         row, lane = column.
//   i2l_gather_ragged_u8  n byte ranges of the page store -> the compact pixel block i2l_preprocess_images reads.  The
//                         store aligns its pages, the block packs them back to back (preprocess_batch's src_offset), so
//                         source and destination are misaligned against each other in general.  A workgroup copies 16 KB
//                         tiles of one range, lane = 16 consecutive destination bytes: aligned 16-byte stores; the source
//                         comes in as one 16-byte load when it is aligned too, else as the five aligned words that hold
//                         the 16 bytes, shifted together.  The bytes in front of the first aligned destination address,
//                         behind the last, and a group whose five words would reach outside the range are loaded byte by
//                         byte: no byte outside [src_off, src_off + size) is read, none outside the destination range
//                         written.
#include "common.h"

namespace {

constexpr int CT = 256;                         // collate: four rows per workgroup
constexpr int GT = 256;                         // gather: threads per workgroup
constexpr int G_ITER = 4;                       // 16-byte groups per lane and tile
constexpr long long G_TILE = (long long)GT * 16 * G_ITER;    // 16 KB of destination per workgroup and step

__global__ __launch_bounds__(CT) void collate_ids_kernel(const int32_t* __restrict__ ids, const int64_t* __restrict__ off,
                                                         long long rows, long long n_ids, const int64_t* __restrict__ index,
                                                         int B, int width, int pad_id, int32_t* __restrict__ out,
                                                         int out_stride, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    const long long r = index[b];
    long long s = 0, len = 0;
    int flags = 0;
    if (r < 0 || r >= rows) {
        flags = 2;
    } else {
        s = off[r];
        len = off[r + 1] - s;
        if (s < 0 || len < 0 || s + len > n_ids) {                   // a store that does not add up: treated as a bad index
            flags = 2;
            len = 0;
        } else if (len > width) {
            flags = 1;
            len = 0;
        }
    }
    int32_t* o = out + (size_t)b * out_stride;
    for (int c = lane; c < width; c += 64) o[c] = c < len ? ids[s + c] : pad_id;
    if (flags && lane == 0) atomicOr(status, flags);
}

__device__ __forceinline__ uint32_t bytes_le(const uint8_t* __restrict__ p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__global__ __launch_bounds__(GT) void gather_ragged_u8_kernel(const uint8_t* __restrict__ src, long long src_bytes,
                                                              const int64_t* __restrict__ src_off,
                                                              const int64_t* __restrict__ size, uint8_t* __restrict__ dst,
                                                              long long dst_bytes, const int64_t* __restrict__ dst_off,
                                                              int32_t* __restrict__ status) {
    const int i = blockIdx.y;
    const long long n = size[i], so = src_off[i], d_o = dst_off[i];
    if (n <= 0 || so < 0 || d_o < 0 || so > src_bytes - n || d_o > dst_bytes - n) {
        if (n != 0 && threadIdx.x == 0 && blockIdx.x == 0) atomicOr(status, 1);      // a range outside a buffer: not copied
        return;
    }
    const uint8_t* s = src + so;
    uint8_t* d = dst + d_o;
    long long head = (long long)((16u - (unsigned)(reinterpret_cast<uintptr_t>(d) & 15u)) & 15u);
    head = head < n ? head : n;
    const long long groups = (n - head) >> 4;
    const long long tail = head + (groups << 4);                     // first byte behind the last whole group
    if (blockIdx.x == 0) {                                           // < 16 bytes at either end, lane = byte
        const long long t = threadIdx.x;
        if (t < head) d[t] = s[t];
        if (t >= 16 && tail + (t - 16) < n) d[tail + (t - 16)] = s[tail + (t - 16)];
    }
    const uint8_t* sb = s + head;
    uint4* db = reinterpret_cast<uint4*>(d + head);                  // 16-byte aligned
    const unsigned mis = (unsigned)(reinterpret_cast<uintptr_t>(sb) & 15u);
    const unsigned sh = mis & 3u;
    for (long long g0 = (long long)blockIdx.x * (GT * G_ITER); g0 < groups; g0 += (long long)gridDim.x * (GT * G_ITER)) {
#pragma unroll
        for (int it = 0; it < G_ITER; ++it) {
            const long long g = g0 + it * GT + threadIdx.x;
            if (g >= groups) break;
            const uint8_t* p = sb + (g << 4);
            uint4 v;
            if (mis == 0) {
                v = *reinterpret_cast<const uint4*>(p);
            } else if (sh == 0) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
                v = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                const uint8_t* a = p - sh;                           // the aligned word that holds p[0]
                if (a >= s && a + 20 <= s + n) {
                    const uint32_t* w = reinterpret_cast<const uint32_t*>(a);
                    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
                    const unsigned r = 8u * sh, l = 32u - r;
                    v = make_uint4((w0 >> r) | (w1 << l), (w1 >> r) | (w2 << l), (w2 >> r) | (w3 << l), (w3 >> r) | (w4 << l));
                } else {                                             // the range's first or last group
                    v = make_uint4(bytes_le(p), bytes_le(p + 4), bytes_le(p + 8), bytes_le(p + 12));
                }
            }
            db[g] = v;
        }
    }
}

}  // namespace

extern "C" int i2l_collate_ids(const int32_t* ids, int64_t n_ids, const int64_t* off, int64_t rows, const int64_t* index, int B,
                               int width, int pad_id, int32_t* out, int out_stride, int32_t* status, i2l_stream_t stream) {
    if (width <= 0 || out_stride < width) return I2L_ERR_UNSUPPORTED;
    if (B < 0 || rows < 0 || n_ids < 0) return I2L_ERR_ARG;
    if (B == 0) return I2L_OK;
    if (!off || !index || !out || !status || (n_ids > 0 && !ids)) return I2L_ERR_ARG;
    hipStream_t s = i2l_s(stream);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return I2L_ERR_LAUNCH;
    hipLaunchKernelGGL(collate_ids_kernel, dim3(i2l_cdiv(B, CT / 64)), dim3(CT), 0, s, ids, off, (long long)rows,
                       (long long)n_ids, index, B, width, pad_id, out, out_stride, status);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

extern "C" int i2l_gather_ragged_u8(const uint8_t* src, int64_t src_bytes, const int64_t* src_off, const int64_t* size, int n,
                                    int64_t max_size, uint8_t* dst, int64_t dst_bytes, const int64_t* dst_off, int32_t* status,
                                    i2l_stream_t stream) {
    if (n > 65535) return I2L_ERR_UNSUPPORTED;                       // a range per grid row
    if (n < 0 || src_bytes < 0 || dst_bytes < 0 || max_size < 0) return I2L_ERR_ARG;
    if (n == 0) return I2L_OK;
    if (!src_off || !size || !dst_off || !status || (src_bytes > 0 && !src) || (dst_bytes > 0 && !dst)) return I2L_ERR_ARG;
    hipStream_t s = i2l_s(stream);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), s) != hipSuccess) return I2L_ERR_LAUNCH;
    long long tiles = (max_size + G_TILE - 1) / G_TILE;              // the kernel strides, so a larger range is still whole
    tiles = tiles < 1 ? 1 : (tiles > 4096 ? 4096 : tiles);
    hipLaunchKernelGGL(gather_ragged_u8_kernel, dim3((unsigned)tiles, (unsigned)n), dim3(GT), 0, s, src, (long long)src_bytes,
                       src_off, size, dst, (long long)dst_bytes, dst_off, status);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
