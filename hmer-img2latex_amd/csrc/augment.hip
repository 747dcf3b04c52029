// Train-time augmentation on the device (reference img2latex/data/dataset.py:486-492): RandomRotation(degrees=5,
// fill=(255,)) followed by RandomAffine(degrees=0, translate=(0.02, 0.02), fill=(255,)) on the decoded page.  On PIL
// images both resample NEAREST, so torchvision ends in two Pillow calls,
//     rot = page.rotate(angle, NEAREST, expand=False, center=None, fillcolor=white)
//     out = rot.transform(rot.size, AFFINE, (1, 0, -tx, 0, 1, -ty), NEAREST, fillcolor=white)
// and Pillow's nearest affine (libImaging/Geometry.c affine_fixed) is 16.16 fixed point: with the six coefficients
// a0..a5 = FIX(matrix), output pixel (x, y) reads source pixel ((a2 + a0*x + a1*y) >> 16, (a5 + a3*x + a4*y) >> 16)
// or the fill colour when that lies off the page.  The shift pass reduces to (x - tx, y - ty) exactly, so the two
// passes are ONE gather: shift, fill if off the page, else the rotation look-up at the shifted position, which may
// itself yield fill.  The coefficients are computed on the host in Python doubles (data/augment.py: Image.rotate's own
// arithmetic); the device work is integer only and the result is Pillow's, byte for byte.
//
// The kernel is a pure gather: scattered reads, nothing shared between lanes.  Each lane owns AFF_VEC consecutive output
// elements that start on an AFF_VEC-element boundary of the output ADDRESS, so a full chunk leaves in one 8-byte (uint8)
// or 16-byte (fp32) store whatever a page's offset in the ragged buffer is; the chunks at a page's two ends are stored
// element by element.
#include <type_traits>

#include "common.h"

namespace {

constexpr int AFF_MAX_SIDE = 16384;      // (a2 + a0*x + a1*y) stays far inside int64, pixel counts inside int32
constexpr int AFF_MAX_CHANNELS = 4;      // fp32 flavour: the fill colour travels by value

struct AffFill { float v[AFF_MAX_CHANNELS]; };

// (a select chain, not an indexed read: the struct is a kernel argument and stays in registers)
__device__ __forceinline__ float aff_fill(const AffFill& f, int ch) {
    return ch == 0 ? f.v[0] : ch == 1 ? f.v[1] : ch == 2 ? f.v[2] : f.v[3];
}

template <typename T> struct AffVec;
template <> struct AffVec<uint8_t> { static constexpr int N = 8; };
template <> struct AffVec<float> { static constexpr int N = 4; };

// T = uint8_t: ragged batch of interleaved pages, page b described by plans[b] (src_offset / src_h / src_w / src_c), fill 255.
// T = float:   dense (n, c, h, w) planes, fill.v[channel].
template <typename T>
__global__ __launch_bounds__(256) void affine_nearest_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                             const i2l_resize_plan* __restrict__ plans,
                                                             const i2l_affine_params* __restrict__ params, int dense_c,
                                                             int dense_h, int dense_w, AffFill fill) {
    constexpr bool planar = std::is_same<T, float>::value;
    constexpr int VEC = AffVec<T>::N;
    struct alignas(sizeof(T) * VEC) Chunk { T v[VEC]; };
    const int b = blockIdx.y;
    int h, w, c;
    long off;
    if constexpr (planar) {
        h = dense_h; w = dense_w; c = dense_c;
        off = (long)b * c * h * w;
    } else {
        const i2l_resize_plan pl = plans[b];
        h = pl.src_h; w = pl.src_w; c = pl.src_c;
        off = pl.src_offset;
        if (h <= 0 || w <= 0 || h > AFF_MAX_SIDE || w > AFF_MAX_SIDE || (c != 1 && c != 3)) return;
    }
    const i2l_affine_params p = params[b];
    const int hw = h * w;
    const long total = (long)hw * c;
    const T* __restrict__ src = in + off;
    T* __restrict__ dst = out + off;
    const int mis = (int)((reinterpret_cast<uintptr_t>(dst) / sizeof(T)) % VEC);   // elements past a chunk boundary
    const long chunks = (total + mis + VEC - 1) / VEC;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < chunks; k += (long)gridDim.x * 256) {
        const long e0 = k * VEC - mis;
        const long first = e0 < 0 ? 0 : e0;
        // element -> (channel, y, x): one set of divisions per chunk, then steps
        int ch, pix;
        if constexpr (planar) { ch = (int)(first / hw); pix = (int)(first - (long)ch * hw); }
        else { pix = (int)(first / c); ch = (int)(first - (long)pix * c); }
        int y = pix / w, x = pix - y * w;
        long sp = -1;                       // source pixel of (x, y), -1 = fill
        bool fresh = true;
        Chunk o;
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const long e = e0 + j;
            const bool live = e >= 0 && e < total;
            if (live) {
                if (fresh) {
                    const int xs = x - p.tx, ys = y - p.ty;                     // the shift pass
                    sp = -1;
                    if (xs >= 0 && xs < w && ys >= 0 && ys < h) {               // else: its fill
                        const long xin = ((long)p.a2 + (long)p.a0 * xs + (long)p.a1 * ys) >> 16;   // the rotation pass
                        const long yin = ((long)p.a5 + (long)p.a3 * xs + (long)p.a4 * ys) >> 16;
                        if (xin >= 0 && xin < w && yin >= 0 && yin < h) sp = yin * w + xin;
                    }
                }
                if constexpr (planar) o.v[j] = sp < 0 ? aff_fill(fill, ch) : src[(long)ch * hw + sp];
                else o.v[j] = sp < 0 ? (T)255 : src[sp * c + ch];
                // next element
                if constexpr (planar) {
                    fresh = true;
                    if (++x == w) { x = 0; if (++y == h) { y = 0; ++ch; } }
                } else {
                    fresh = false;
                    if (++ch == c) { ch = 0; fresh = true; if (++x == w) { x = 0; ++y; } }
                }
            } else {
                o.v[j] = (T)0;
            }
        }
        if (e0 >= 0 && e0 + VEC <= total) {
            *reinterpret_cast<Chunk*>(dst + e0) = o;
        } else {
#pragma unroll
            for (int j = 0; j < VEC; ++j)
                if (e0 + j >= 0 && e0 + j < total) dst[e0 + j] = o.v[j];
        }
    }
}

// load-latency bound: enough workgroups to fill every CU's wave slots a few times over, the rest by the grid stride
int aff_blocks_x(long max_elems, int vec, int n) {
    long bx = ((max_elems + 2 * vec - 2) / vec + 255) / 256;
    const long cap = 8192 / n > 1 ? 8192 / n : 1;
    if (bx > cap) bx = cap;
    return (int)(bx < 1 ? 1 : bx);
}

}  // namespace

extern "C" int i2l_affine_nearest_u8(const uint8_t* pixels, uint8_t* out, const i2l_resize_plan* plans,
                                     const i2l_affine_params* params, int n, int max_side, int64_t max_page_bytes,
                                     i2l_stream_t stream) {
    if (!pixels || !out || pixels == out || !plans || !params || n <= 0 || n > 65535 || max_side <= 0 || max_page_bytes <= 0)
        return I2L_ERR_ARG;
    if (max_side > AFF_MAX_SIDE || max_page_bytes > 3ll * AFF_MAX_SIDE * AFF_MAX_SIDE) return I2L_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(affine_nearest_kernel<uint8_t>, dim3(aff_blocks_x(max_page_bytes, AffVec<uint8_t>::N, n), n), dim3(256), 0,
                       i2l_s(stream), pixels, out, plans, params, 0, 0, 0, AffFill{});
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}

extern "C" int i2l_affine_nearest_f32(const float* x, float* out, const i2l_affine_params* params, const float* fill, int n,
                                      int c, int h, int w, i2l_stream_t stream) {
    if (!x || !out || x == out || !params || !fill || n <= 0 || n > 65535 || c <= 0 || h <= 0 || w <= 0) return I2L_ERR_ARG;
    if (c > AFF_MAX_CHANNELS || h > AFF_MAX_SIDE || w > AFF_MAX_SIDE) return I2L_ERR_UNSUPPORTED;
    AffFill f{};
    for (int i = 0; i < c; ++i) f.v[i] = fill[i];
    hipLaunchKernelGGL(affine_nearest_kernel<float>, dim3(aff_blocks_x((long)c * h * w, AffVec<float>::N, n), n), dim3(256), 0,
                       i2l_s(stream), x, out, static_cast<const i2l_resize_plan*>(nullptr), params, c, h, w, f);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
