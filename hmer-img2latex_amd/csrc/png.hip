// PNG pages decoded on the device (img2latex_amd/data/png.py parses the container on the host and hands over the zlib
// stream undecompressed): i2l_png_decode inflates, unfilters and converts n images in ONE launch, a wave per image, four
// waves per workgroup, and writes a status word per image.
//
// Work split inside the wave.  The bit stream is serial by nature: every lane runs the shared decode core
// (png_core.inc.h) with the same values -- loads of one address are a broadcast, control flow stays wave-uniform, and
// a wave instruction costs the same for one active lane as for 64 -- while the tables (3.5 KB of LDS per wave) and the
// literals are written by lane 0 alone.  The 64 lanes share the copies: a match of `len` bytes at distance `dist` is
// the periodic copy out[pos + i] = out[pos - dist + i % dist], whose sources all lie in front of `pos`, so an
// overlapping match (dist < len) needs no second pass; stored blocks and the Adler-32 sums are lane-strided too.
// Unfiltering walks the rows in order (Up, Average and Paeth read the row above): None and Up are lane = byte, Sub is a
// wave scan per channel over chunks of 64 pixels, Average and Paeth are serial along the row, lane = channel byte.
// Each finished row is converted to the page (lane = pixel) while it is still in cache.
//
// What bounds it.  The input is untrusted: the core returns on the first bit that is not there and decides every
// output position before a Sink call (pos + len <= expect, dist <= pos), the descriptors are checked on the host before
// the launch, so a wave touches nothing but its own stream, its own workspace slice and its own page.  Waves never wait
// for each other: no barrier, no poll, no atomics.  A wave's own stores are read back by other lanes of the same wave
// only; the wave executes its memory instructions in order, and a wavefront-scope fence keeps the compiler from moving
// them across each other.
#include <algorithm>
#include <vector>

#include "common.h"
#include "png_core.inc.h"

namespace {

constexpr int PT = 256;                          // four images per workgroup
constexpr int64_t PNG_MAX_FILTERED = (int64_t)1 << 27;   // per image: the Adler-32 sums stay inside uint64 (png_adler_partial)
constexpr int PNG_MAX_IMAGES = 1 << 20;

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct WaveSink {
    uint8_t* out;
    int lane;
    __device__ bool leader() const { return lane == 0; }
    __device__ void sync() const { wave_sync(); }
    __device__ void literal(int64_t pos, uint8_t v) const {
        if (lane == 0) out[pos] = v;
    }
    __device__ void match(int64_t pos, int dist, int len) const {
        wave_sync();                                                  // the source bytes were written by other lanes
        const uint8_t* src = out + (pos - dist);
        if (dist >= len) {
            for (int i = lane; i < len; i += 64) out[pos + i] = src[i];
        } else {
            for (int i = lane; i < len; i += 64) out[pos + i] = src[i % dist];
        }
    }
    __device__ void stored(int64_t pos, const uint8_t* src, int len) const {
        for (int i = lane; i < len; i += 64) out[pos + i] = src[i];
    }
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int off = 32; off > 0; off >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, off, 64);
    return v;
}

// rows of `rb` bytes behind a filter byte, in place; returns a status
__device__ int unfilter_convert(uint8_t* f, const i2l_png_image& im, int bpp, const uint8_t* pal, uint8_t* page, int lane) {
    const int w = im.width, h = im.height, oc = im.channels, ct = im.colour_type;
    const int64_t rb = (int64_t)w * bpp, stride = rb + 1;
    bool bad_index = false;
    for (int y = 0; y < h; ++y) {
        wave_sync();                                                  // the row above, and this one, as other lanes left them
        uint8_t* cur = f + y * stride + 1;
        const uint8_t* prev = cur - stride;                           // read only when y > 0
        const int ft = cur[-1];
        if (ft > 4) return PNG_E_FILTER;
        if (ft == 2) {
            if (y > 0)
                for (int64_t i = lane; i < rb; i += 64) cur[i] = (uint8_t)(cur[i] + prev[i]);
        } else if (ft == 1) {
            for (int c = 0; c < bpp; ++c) {
                int carry = 0;
                for (int p0 = 0; p0 < w; p0 += 64) {                  // an inclusive scan over 64 pixels of one channel
                    const int p = p0 + lane;
                    int v = p < w ? cur[(int64_t)p * bpp + c] : 0;
                    for (int off = 1; off < 64; off <<= 1) {
                        const int t = __shfl_up(v, off, 64);
                        if (lane >= off) v += t;
                    }
                    v += carry;
                    if (p < w) cur[(int64_t)p * bpp + c] = (uint8_t)v;
                    carry = __shfl(v, 63, 64) & 255;
                }
            }
        } else if (ft >= 3) {
            if (lane < bpp) {                                         // serial along the row, a lane per channel byte
                int a = 0, c = 0;
                for (int p0 = 0; p0 < w; p0 += 8) {
                    const int m = w - p0 < 8 ? w - p0 : 8;
                    int x[8], b[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {                     // the loads first: they do not depend on the chain
                        const int64_t at = (int64_t)(p0 + (k < m ? k : 0)) * bpp + lane;
                        x[k] = cur[at];
                        b[k] = y > 0 ? prev[at] : 0;
                    }
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        if (k < m) {
                            a = png_recon(ft, x[k], a, b[k], c);
                            c = b[k];
                            cur[(int64_t)(p0 + k) * bpp + lane] = (uint8_t)a;
                        }
                    }
                }
            }
        }
        wave_sync();
        uint8_t* o = page + (int64_t)y * w * oc;
        for (int p = lane; p < w; p += 64) {
            const uint8_t* s = cur + (int64_t)p * bpp;
            int r = s[0], g = r, bl = r;
            if (ct == 2 || ct == 6) {
                g = s[1];
                bl = s[2];
            } else if (ct == 3) {
                if (r >= im.pal_n) {
                    bad_index = true;
                    r = g = bl = 0;
                } else {
                    const uint8_t* e = pal + 3 * r;
                    r = e[0];
                    g = e[1];
                    bl = e[2];
                }
            }
            if (oc == 1) {
                o[p] = (ct == 0 || ct == 4) ? (uint8_t)r : png_luma(r, g, bl);
            } else {
                o[3 * (int64_t)p] = (uint8_t)r;
                o[3 * (int64_t)p + 1] = (uint8_t)g;
                o[3 * (int64_t)p + 2] = (uint8_t)bl;
            }
        }
    }
    return __any(bad_index) ? PNG_E_PALETTE : PNG_OK;
}

__global__ __launch_bounds__(PT) void png_decode_kernel(const uint8_t* __restrict__ z, const i2l_png_image* __restrict__ images,
                                                        const int64_t* __restrict__ ws_off, int n, uint8_t* pixels,
                                                        int32_t* __restrict__ status, uint8_t* ws) {
    __shared__ PngTables tables[PT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * (PT / 64) + wave;
    if (i >= n) return;                                               // wave-uniform; the waves share no barrier
    const i2l_png_image im = images[i];
    const int bpp = png_bpp(im.colour_type);
    const int64_t expect = (int64_t)im.height * (1 + (int64_t)im.width * bpp);
    uint8_t* f = ws + ws_off[i];
    WaveSink sink{f, lane};
    uint32_t want = 0;
    int rc = png_inflate(z + im.z_off, im.z_len, expect, tables[wave], sink, &want);
    if (rc == PNG_OK) {
        wave_sync();
        uint64_t sa = 0, sb = 0;
        png_adler_partial(f, expect, lane, 64, &sa, &sb);
        if (png_adler_finish(wave_sum(sa), wave_sum(sb), expect) != want) rc = PNG_E_ADLER;
    }
    if (rc == PNG_OK) rc = unfilter_convert(f, im, bpp, im.pal_off >= 0 ? z + im.pal_off : nullptr, pixels + im.out_off, lane);
    if (lane == 0) status[i] = rc;
}

struct Layout {
    size_t images, offsets, data, total;
};
Layout png_layout(int n, int64_t filtered_total) {
    Layout l;
    l.images = 0;
    l.offsets = i2l_align((size_t)n * sizeof(i2l_png_image));
    l.data = l.offsets + i2l_align((size_t)n * sizeof(int64_t));
    l.total = l.data + (size_t)filtered_total + (size_t)n * 16 + 256;  // every image's slice starts at a multiple of 16
    return l;
}

}  // namespace

extern "C" size_t i2l_png_decode_workspace_bytes(int n, int64_t filtered_bytes_total) {
    if (n < 0 || filtered_bytes_total < 0) return 0;
    return png_layout(n, filtered_bytes_total).total;
}

extern "C" int i2l_png_decode(const uint8_t* z, int64_t z_bytes, const i2l_png_image* images, int n, uint8_t* pixels,
                              int64_t pixels_bytes, int32_t* status, void* workspace, size_t workspace_bytes,
                              i2l_stream_t stream) {
    if (n < 0 || z_bytes < 0 || pixels_bytes < 0) return I2L_ERR_ARG;
    if (n == 0) return I2L_OK;
    if (n > PNG_MAX_IMAGES) return I2L_ERR_UNSUPPORTED;
    if (!z || !images || !pixels || !status) return I2L_ERR_ARG;
    std::vector<int64_t> off((size_t)n);
    std::vector<std::pair<int64_t, int64_t>> pages((size_t)n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        const i2l_png_image& im = images[i];
        const int bpp = png_bpp(im.colour_type);
        if (bpp == 0 || im.width < 1 || im.height < 1) return I2L_ERR_ARG;
        if (im.channels != 1 && im.channels != 3) return I2L_ERR_ARG;
        if ((im.colour_type == 0 && im.channels != 1) || (im.colour_type == 2 && im.channels != 3)) return I2L_ERR_ARG;
        if (im.z_off < 0 || im.z_len < 0 || im.z_off > z_bytes - im.z_len) return I2L_ERR_ARG;
        if (im.colour_type == 3) {
            if (im.pal_n < 1 || im.pal_n > 256 || im.pal_off < 0 || im.pal_off > z_bytes - 3 * (int64_t)im.pal_n) return I2L_ERR_ARG;
        }
        const int64_t filtered = (int64_t)im.height * (1 + (int64_t)im.width * bpp);     // both factors below 2^31 * 4 + 1
        if ((int64_t)im.width * bpp >= PNG_MAX_FILTERED || filtered > PNG_MAX_FILTERED) return I2L_ERR_UNSUPPORTED;
        const int64_t page = (int64_t)im.height * im.width * im.channels;
        if (im.out_off < 0 || im.out_off > pixels_bytes - page) return I2L_ERR_ARG;
        pages[(size_t)i] = {im.out_off, page};
        off[(size_t)i] = total;
        total += (filtered + 15) / 16 * 16;
    }
    std::sort(pages.begin(), pages.end());
    for (int i = 1; i < n; ++i)
        if (pages[(size_t)i - 1].first + pages[(size_t)i - 1].second > pages[(size_t)i].first) return I2L_ERR_ARG;   // pages overlap
    const Layout l = png_layout(n, total);
    if (!workspace || workspace_bytes < l.data + (size_t)total) return I2L_ERR_WORKSPACE;   // `total` counts the 16-byte rounding
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return I2L_ERR_ARG;
    hipStream_t s = i2l_s(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    // `images` and `off` are pageable host memory: HIP performs such a copy synchronously with respect to the host, and the
    // wait below makes that explicit -- both copies have been performed when it returns, so the caller's array and the
    // local vector may go.  The price is the documented one: the call blocks until `stream` has reached the copies.
    if (hipMemcpyAsync(ws + l.images, images, (size_t)n * sizeof(i2l_png_image), hipMemcpyHostToDevice, s) != hipSuccess) return I2L_ERR_LAUNCH;
    if (hipMemcpyAsync(ws + l.offsets, off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, s) != hipSuccess) return I2L_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return I2L_ERR_LAUNCH;
    hipLaunchKernelGGL(png_decode_kernel, dim3((unsigned)i2l_cdiv(n, PT / 64)), dim3(PT), 0, s, z,
                       reinterpret_cast<const i2l_png_image*>(ws + l.images), reinterpret_cast<const int64_t*>(ws + l.offsets), n,
                       pixels, status, ws + l.data);
    I2L_CHECK_LAUNCH();
    return I2L_OK;
}
