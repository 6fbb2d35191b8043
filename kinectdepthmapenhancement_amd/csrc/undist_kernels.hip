// undist_kernels.hip — LensUndistortion: frames of a camera with lens distortion (OpenCV's rational model, of which
// Brown-Conrady is the case k4 = k5 = k6 = 0) resampled into a pinhole view, for n frames on the device.  The reference has no
// such step (its frames come through OpenNI from a Kinect v1); every class here assumes the pinhole view this produces.
//   U0 reset     filled[f] = 0 for the frames of the call, in front of U2 behind a kernel boundary (a kernel and not a memset
//                node: reg_kernels.hip, R0)
//   U1 colour    a thread owns four consecutive output pixels = 12 bytes; each pixel computes its source point from the
//                coefficients in the kernel arguments (no table: the kernel moves 6 B per pixel, a float2 map would add 8)
//                and blends four taps, gathers that neighbouring pixels share in L2: the two taps of a row are six
//                consecutive bytes, fetched as 4 + 2 where both lie inside (byte loads at the frame's border); a wave's 768
//                bytes pass through LDS so that each store instruction writes 256 consecutive bytes (as R3 of reg_kernels.hip)
//   U2 depth     a thread owns four consecutive output pixels of each of its workgroup's eight tiles: one 16-byte (float) or
//                8-byte (uint16) store where the output frame starts on such a boundary, element stores elsewhere and in the
//                frame's partial tail; the pixels that got a depth are counted per wave and meet in one integer atomicAdd
//                per workgroup (8192 pixels)
//   U3 map       (us, vs) of every output pixel as float2, for kde_undist_map_device; U1 and U2 do not read it
// The rule (every operation one IEEE binary32 operation in this order, no fused multiply-add, correctly rounded divisions),
// for output pixel (i, j):
//   x  = ((float)i - cxn) / fxn;  y = ((float)j - cyn) / fyn
//   xx = x * x;  yy = y * y;  xy = x * y;  r2 = xx + yy
//   num = ((k3 * r2 + k2) * r2 + k1) * r2 + 1;  den = ((k6 * r2 + k5) * r2 + k4) * r2 + 1;  rad = num / den
//   xd = (x * rad + p1 * (xy + xy)) + p2 * (r2 + (xx + xx));  yd = (y * rad + p1 * (r2 + (yy + yy))) + p2 * (xy + xy)
//   us = fx * xd + cx;  vs = fy * yd + cy
//   bilinear(p): x0 = floorf(us), ax = us - x0, y0, ay likewise; top = p00 + ax * (p01 - p00), bot = p10 + ax * (p11 - p10),
//                top + ay * (bot - top)
//   colour    (0, 0, 0) unless us > -1 && us < sw && vs > -1 && vs < sh (on the floats, a NaN fails); a tap outside the source
//             is (0, 0, 0); per channel rintf(bilinear) clamped to 0 .. 255
//   depth     valid iff z > z_min && z < z_max.  nearest: fu = rintf(us), fv = rintf(vs) (ties to even), kept iff 0 <= fu <=
//             sw - 1 && 0 <= fv <= sh - 1 (on the floats) and the sample is valid, else 0.  depth_interp == 1: bilinear iff
//             x0 >= 0 && x0 + 1 <= sw - 1 && y0 >= 0 && y0 + 1 <= sh - 1, the four taps are valid and max - min <= max_gap;
//             the nearest rule in every other case.  filled[f] counts the pixels that were kept, before any rounding to uint16.
// Every output pixel is a function of the source frame and its own coordinates, the count an integer sum: the same bytes for
// any n, place in the batch and alignment.  The gathers use default caching in every call (a source byte serves up to four
// output pixels out of L2); the stores stream past the Infinity Cache when the call moves more than it holds.
#include "kde_internal.h"
#include "kde_device_math.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kQuad = 4;                               // output pixels per thread
constexpr unsigned kWavePixels = 64 * kQuad;
constexpr unsigned kBlockPixels = kWaves * kWavePixels;
constexpr unsigned kDepthTiles = 8;                         // tiles of kBlockPixels one workgroup of U2 takes: one atomicAdd for 8192 pixels

typedef unsigned u_v2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void source_point(const UndistCalib& c, unsigned i, unsigned j, float& us, float& vs)
{
    const float x = ((float)i - c.cxn) / c.fxn, y = ((float)j - c.cyn) / c.fyn;
    const float xx = x * x, yy = y * y, xy = x * y, r2 = xx + yy;
    const float num = ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2 + 1.0f;
    const float den = ((c.k6 * r2 + c.k5) * r2 + c.k4) * r2 + 1.0f;
    const float rad = num / den;
    const float xd = (x * rad + c.p1 * (xy + xy)) + c.p2 * (r2 + (xx + xx));
    const float yd = (y * rad + c.p1 * (r2 + (yy + yy))) + c.p2 * (xy + xy);
    us = c.fx * xd + c.cx;
    vs = c.fy * yd + c.cy;
}

__device__ __forceinline__ float bilinear(float p00, float p01, float p10, float p11, float ax, float ay)
{
    const float top = p00 + ax * (p01 - p00), bot = p10 + ax * (p11 - p10);
    return top + ay * (bot - top);
}

// the pixel after (i, j) in raster order
__device__ __forceinline__ void next_pixel(unsigned& i, unsigned& j, unsigned ow)
{
    if (++i == ow) {
        i = 0;
        j++;
    }
}

// one tap of the colour image: b, g, r as floats, zeros outside the source frame
__device__ __forceinline__ void color_tap(const uint8_t* img, int x, int y, int sw, int sh, float* v)
{
    v[0] = v[1] = v[2] = 0.0f;
    if ((unsigned)x < (unsigned)sw && (unsigned)y < (unsigned)sh) {
        const uint8_t* s = img + ((size_t)y * (unsigned)sw + (unsigned)x) * 3;
        v[0] = (float)s[0];
        v[1] = (float)s[1];
        v[2] = (float)s[2];
    }
}

// the taps (x, y) and (x + 1, y) of one row, both inside the frame: six consecutive bytes fetched as 4 + 2 (global loads need
// no alignment), two gather instructions where six byte loads took the kernel's time
__device__ __forceinline__ void color_pair(const uint8_t* img, int x, int y, int sw, float* a, float* b)
{
    const uint8_t* s = img + ((size_t)y * (unsigned)sw + (unsigned)x) * 3;
    uint32_t lo;
    uint16_t hi;
    __builtin_memcpy(&lo, s, 4);
    __builtin_memcpy(&hi, s + 4, 2);
    a[0] = (float)(lo & 0xffu);
    a[1] = (float)((lo >> 8) & 0xffu);
    a[2] = (float)((lo >> 16) & 0xffu);
    b[0] = (float)(lo >> 24);
    b[1] = (float)(hi & 0xffu);
    b[2] = (float)(hi >> 8);
}

// the taps (x, y) and (x + 1, y) where some of them may lie outside
__device__ __forceinline__ void color_row(const uint8_t* img, int x, int y, int sw, int sh, float* a, float* b)
{
    if (x >= 0 && x + 1 < sw && (unsigned)y < (unsigned)sh) {
        color_pair(img, x, y, sw, a, b);
    } else {
        color_tap(img, x, y, sw, sh, a);
        color_tap(img, x + 1, y, sw, sh, b);
    }
}

// b | g << 8 | r << 16 of output pixel (i, j)
__device__ __forceinline__ uint32_t color_pixel(const UndistLaunch& L, const uint8_t* img, unsigned i, unsigned j)
{
    float us, vs;
    source_point(L.c, i, j, us, vs);
    if (!(us > -1.0f && us < (float)L.sw && vs > -1.0f && vs < (float)L.sh)) return 0u;    // a NaN fails
    const float x0 = floorf(us), y0 = floorf(vs);           // -1 .. sw - 1, -1 .. sh - 1
    const float ax = us - x0, ay = vs - y0;
    const int ix = (int)x0, iy = (int)y0;
    float p00[3], p01[3], p10[3], p11[3];
    color_row(img, ix, iy, L.sw, L.sh, p00, p01);
    color_row(img, ix, iy + 1, L.sw, L.sh, p10, p11);
    uint32_t c = 0u;
#pragma unroll
    for (unsigned ch = 0; ch < 3; ch++) {
        const float r = fminf(fmaxf(rintf(bilinear(p00[ch], p01[ch], p10[ch], p11[ch], ax, ay)), 0.0f), 255.0f);
        c |= (uint32_t)r << (8u * ch);
    }
    return c;
}

// samples idx and idx + 1 of a source frame in one load (an element-aligned pair)
__device__ __forceinline__ void source_depth_pair(const char* frame, int format, size_t idx, float& a, float& b)
{
    if (format == KDE_DEPTH_F32) {
        float v[2];
        __builtin_memcpy(v, __builtin_assume_aligned(frame + idx * sizeof(float), 4), sizeof(v));
        a = v[0];
        b = v[1];
    } else {
        uint32_t w;
        __builtin_memcpy(&w, __builtin_assume_aligned(frame + idx * sizeof(uint16_t), 2), sizeof(w));
        a = (float)(w & 0xffffu);
        b = (float)(w >> 16);
    }
}

// the depth of output pixel (i, j): false and 0 where it gets none
__device__ __forceinline__ bool depth_pixel(const UndistLaunch& L, const char* frame, unsigned i, unsigned j, float& z)
{
    float us, vs;
    source_point(L.c, i, j, us, vs);
    const float lastx = (float)(L.sw - 1), lasty = (float)(L.sh - 1);
    if (L.depth_interp) {
        const float x0 = floorf(us), y0 = floorf(vs);
        if (x0 >= 0.0f && x0 + 1.0f <= lastx && y0 >= 0.0f && y0 + 1.0f <= lasty) {     // all four taps inside; a NaN fails
            const size_t at = (size_t)y0 * (unsigned)L.sw + (size_t)x0;
            float z00, z01, z10, z11;
            source_depth_pair(frame, L.depth_format, at, z00, z01);
            source_depth_pair(frame, L.depth_format, at + (unsigned)L.sw, z10, z11);
            const bool valid = z00 > L.z_min && z00 < L.z_max && z01 > L.z_min && z01 < L.z_max && z10 > L.z_min && z10 < L.z_max &&
                               z11 > L.z_min && z11 < L.z_max;
            if (valid) {                                    // four finite positive numbers
                const float hi = fmaxf(fmaxf(z00, z01), fmaxf(z10, z11)), lo = fminf(fminf(z00, z01), fminf(z10, z11));
                if (hi - lo <= L.max_gap) {
                    z = bilinear(z00, z01, z10, z11, us - x0, vs - y0);
                    return true;
                }
            }
        }
    }
    z = 0.0f;
    const float fu = rintf(us), fv = rintf(vs);             // ties to even, like depth_to_u16
    if (!(fu >= 0.0f && fu <= lastx && fv >= 0.0f && fv <= lasty)) return false;
    const float zn = load_depth(frame, L.depth_format == KDE_DEPTH_F32, (size_t)fv * (unsigned)L.sw + (size_t)fu);
    if (!(zn > L.z_min && zn < L.z_max)) return false;
    z = zn;
    return true;
}

// U0: one thread per frame
__global__ __launch_bounds__(kThreads) void undist_reset_kernel(uint32_t* __restrict__ filled, unsigned n)
{
    const unsigned f = blockIdx.x * kThreads + threadIdx.x;
    if (f < n) filled[f] = 0u;
}

// U1: grid (blocks of 1024 output pixels, n), block 256
template <bool NT>
__global__ __launch_bounds__(kThreads) void undist_color_kernel(UndistLaunch L, const uint8_t* __restrict__ bgr, int bgr_frames,
                                                                uint8_t* __restrict__ out)
{
    __shared__ uint32_t stage[kWaves][192];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)L.ow * (unsigned)L.oh;
    const unsigned frame = blockIdx.y;
    const unsigned base = blockIdx.x * kBlockPixels + wv * kWavePixels;     // wave-uniform
    if (base >= px) return;
    const uint8_t* img = bgr + (bgr_frames == 1 ? (size_t)0 : (size_t)frame) * (size_t)L.sw * L.sh * 3;
    const unsigned first = base + kQuad * lane;
    unsigned j = first / (unsigned)L.ow, i = first - j * (unsigned)L.ow;
    uint32_t c[4];
#pragma unroll
    for (unsigned k = 0; k < kQuad; k++) {
        c[k] = first + k < px ? color_pixel(L, img, i, j) : 0u;
        next_pixel(i, j, (unsigned)L.ow);
    }
    uint8_t* o = out + (size_t)frame * px * 3;
    if (base + kWavePixels <= px && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
        uint32_t* w = stage[wv];
        w[3 * lane] = c[0] | (c[1] << 24);
        w[3 * lane + 1] = (c[1] >> 8) | (c[2] << 16);
        w[3 * lane + 2] = (c[2] >> 16) | (c[3] << 8);
        wave_exchange_fence();
        uint32_t* d = reinterpret_cast<uint32_t*>(o + (size_t)base * 3);
#pragma unroll
        for (unsigned q = 0; q < 3; q++) {
            if (NT) __builtin_nontemporal_store(w[64u * q + lane], d + 64u * q + lane);
            else d[64u * q + lane] = w[64u * q + lane];
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < kQuad; k++) {
            const unsigned p = first + k;
            if (p < px) {
                o[3 * (size_t)p] = (uint8_t)c[k];
                o[3 * (size_t)p + 1] = (uint8_t)(c[k] >> 8);
                o[3 * (size_t)p + 2] = (uint8_t)(c[k] >> 16);
            }
        }
    }
}

// U2: grid (blocks of 8 x 1024 consecutive output pixels, n), block 256.  Eight tiles per workgroup, because the counts of all
// frames lie in one or two cache lines: with one atomicAdd per 1024 pixels the call took the time of those adds.
template <bool NT>
__global__ __launch_bounds__(kThreads) void undist_depth_kernel(UndistLaunch L)
{
    __shared__ uint32_t wave_count[kWaves];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)L.ow * (unsigned)L.oh;
    const unsigned frame = blockIdx.y;
    const char* sframe = static_cast<const char*>(L.depth) + (size_t)frame * (size_t)L.sw * L.sh * depth_element(L.depth_format);
    uint32_t count = 0;
    for (unsigned t = 0; t < kDepthTiles; t++) {
        const unsigned first = ((blockIdx.x * kDepthTiles + t) * kThreads + threadIdx.x) * kQuad;
        if (first >= px) break;
        unsigned j = first / (unsigned)L.ow, i = first - j * (unsigned)L.ow;
        float z[4];
#pragma unroll
        for (unsigned k = 0; k < kQuad; k++) {
            z[k] = 0.0f;
            if (first + k < px && depth_pixel(L, sframe, i, j, z[k])) count++;
            next_pixel(i, j, (unsigned)L.ow);
        }
        const bool whole = first + kQuad <= px;
        if (L.out_format == KDE_DEPTH_F32) {
            float* o = static_cast<float*>(L.out) + (size_t)frame * px;
            if (whole && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
                st4(reinterpret_cast<float4*>(o + first), make_float4(z[0], z[1], z[2], z[3]), NT);
            } else {
#pragma unroll
                for (unsigned k = 0; k < kQuad; k++) {
                    if (first + k < px) o[first + k] = z[k];
                }
            }
        } else {
            uint16_t* o = static_cast<uint16_t*>(L.out) + (size_t)frame * px;
            uint32_t d[4];
#pragma unroll
            for (unsigned k = 0; k < kQuad; k++) d[k] = depth_to_u16(z[k]);
            if (whole && (reinterpret_cast<uintptr_t>(o) & 7u) == 0) {
                const u_v2 v = {d[0] | (d[1] << 16), d[2] | (d[3] << 16)};
                u_v2* q = reinterpret_cast<u_v2*>(o + first);
                if (NT) __builtin_nontemporal_store(v, q);
                else *q = v;
            } else {
#pragma unroll
                for (unsigned k = 0; k < kQuad; k++) {
                    if (first + k < px) o[first + k] = (uint16_t)d[k];
                }
            }
        }
    }
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) count += (uint32_t)__shfl_xor((int)count, (int)off, 64);
    if (lane == 0) wave_count[wv] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        if (total) atomicAdd(&L.filled[frame], total);      // an integer sum: the same in any order
    }
}

// U3: one output pixel per thread
__global__ __launch_bounds__(kThreads) void undist_map_kernel(UndistCalib c, unsigned ow, unsigned px, float2* __restrict__ map)
{
    const unsigned p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= px) return;
    const unsigned j = p / ow, i = p - j * ow;
    float us, vs;
    source_point(c, i, j, us, vs);
    map[p] = make_float2(us, vs);
}

}  // namespace

int launch_undist_color(const UndistLaunch& a, const uint8_t* bgr, int bgr_frames, uint8_t* out, hipStream_t s)
{
    const size_t spx = (size_t)a.sw * a.sh, opx = (size_t)a.ow * a.oh;
    const bool nt = past_cache(kSiteUndistColor, ((size_t)bgr_frames * spx + (size_t)a.n * opx) * 3);
    const dim3 grid((unsigned)((opx + kBlockPixels - 1) / kBlockPixels), (unsigned)a.n), block(kThreads);
    if (nt) hipLaunchKernelGGL(undist_color_kernel<true>, grid, block, 0, s, a, bgr, bgr_frames, out);
    else hipLaunchKernelGGL(undist_color_kernel<false>, grid, block, 0, s, a, bgr, bgr_frames, out);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

int launch_undist_depth(const UndistLaunch& a, hipStream_t s)
{
    const size_t spx = (size_t)a.sw * a.sh, opx = (size_t)a.ow * a.oh;
    const bool nt = past_cache(kSiteUndistDepth, (size_t)a.n * (spx * depth_element(a.depth_format) + opx * depth_element(a.out_format)));
    const size_t per_block = (size_t)kBlockPixels * kDepthTiles;
    const dim3 grid((unsigned)((opx + per_block - 1) / per_block), (unsigned)a.n), block(kThreads);
    hipLaunchKernelGGL(undist_reset_kernel, dim3((unsigned)((a.n + kThreads - 1) / kThreads)), block, 0, s, a.filled, (unsigned)a.n);
    if (nt) hipLaunchKernelGGL(undist_depth_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(undist_depth_kernel<false>, grid, block, 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

int launch_undist_map(const UndistLaunch& a, float2* map, hipStream_t s)
{
    const size_t opx = (size_t)a.ow * a.oh;
    hipLaunchKernelGGL(undist_map_kernel, dim3((unsigned)((opx + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, a.c, (unsigned)a.ow,
                       (unsigned)opx, map);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
