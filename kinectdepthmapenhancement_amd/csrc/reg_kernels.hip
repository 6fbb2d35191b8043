// reg_kernels.hip — DepthRegistration: what Kinect::InitAllData (Kinect.cpp:71-75) asks OpenNI for before any frame reaches
// main.cpp -- the depth map warped into the colour camera's view -- for n frames on the device.
//   R0 reset     every key of the z-buffer becomes 0xFFFFFFFF.  A kernel and not a memset node: in a captured graph the
//                replay on this runtime did not keep a memset node in front of the kernel node behind it (the keys of the
//                scatter were wiped, in part or all), while kernel nodes keep their order
//   R1 scatter   a wave owns 256 consecutive source pixels, lane l the pixels base + 64 k + l (k = 0..3), so every atomic
//                wave-instruction comes from 64 consecutive pixels of (mostly) one row and, at like resolutions, falls on a
//                contiguous run of the target.  Each valid pixel is projected into the colour camera and its Zc, as its
//                bit pattern, is min-ed into the z-buffer: one pixel (point mode) or the footprint of the source pixel's
//                square (splat mode).  Relaxed agent-scope unsigned min, result unused.
//   R2 finalise  a thread owns eight keys (two 16-byte loads): an untouched key becomes 0, any other its Zc (float) or
//                depth_to_u16(Zc); the reached keys are counted per wave and meet in one integer atomicAdd per workgroup.
//   R3 gather    the companion: every depth pixel fetches the colour of its point-mode target; four pixels = 12 bytes per
//                lane, a wave's 768 bytes through LDS so that each store instruction writes 256 consecutive bytes.
// The rule (every operation one IEEE binary32 operation in this order, no fused multiply-add, correctly rounded divisions):
//   valid    z > z_min && z < z_max
//   project(a, b):  xn = (a - cxd) / fxd, yn = (b - cyd) / fyd, X = xn * z, Y = yn * z
//                   Xc = ((r00 * X + r01 * Y) + r02 * z) + tx, Yc and Zc likewise; fails unless Zc > z_min && Zc < z_max
//                   uc = fxc * (Xc / Zc) + cxc, vc = fyc * (Yc / Zc) + cyc
//   point    iu = rintf(uc), iv = rintf(vc) of project(u, v); kept iff 0 <= iu <= Wc - 1 && 0 <= iv <= Hc - 1 (on the floats)
//   splat    (ua, va) = project(u - 0.5, v - 0.5), (ub, vb) = project(u + 0.5, v + 0.5); the columns
//            max(ceilf(min(ua, ub)), 0) .. min(ceilf(max(ua, ub)) - 1, Wc - 1), at most max_splat of them from the first;
//            rows likewise; a failed corner, a NaN coordinate or an empty span drops the pixel
//   key      the bits of the centre's Zc (positive, so unsigned order is numeric order); zbuf = min(zbuf, key)
// A minimum does not depend on the order of its operands, the count is an integer sum, and the kernel boundary orders R1
// before R2: the result is a function of the frame alone, the same bytes for any n, place in the batch and alignment.
// A source frame on a 16-byte (float) or 8-byte (uint16) boundary is read four pixels per lane and transposed through LDS;
// any other frame, and a wave that holds the frame's end, with element loads.
#include "kde_internal.h"
#include "kde_device_math.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kWavePixels = 256;                       // four per lane
constexpr unsigned kBlockPixels = kWaves * kWavePixels;
constexpr unsigned kOctet = 8;                              // keys per thread of R2
constexpr uint32_t kEmpty = 0xffffffffu;                    // what R0 leaves: no source pixel came here

typedef unsigned r_v2 __attribute__((ext_vector_type(2)));

struct Projected {
    float u, v, z;
    bool ok;
};

__device__ __forceinline__ Projected project(float a, float b, float z, const RegLaunch& L)
{
    const RegCalib& c = L.c;
    const float xn = (a - c.cxd) / c.fxd, yn = (b - c.cyd) / c.fyd;
    const float X = xn * z, Y = yn * z;
    const float Xc = ((c.r[0] * X + c.r[1] * Y) + c.r[2] * z) + c.t[0];
    const float Yc = ((c.r[3] * X + c.r[4] * Y) + c.r[5] * z) + c.t[1];
    const float Zc = ((c.r[6] * X + c.r[7] * Y) + c.r[8] * z) + c.t[2];
    Projected p;
    p.z = Zc;
    p.ok = Zc > L.z_min && Zc < L.z_max;
    p.u = c.fxc * (Xc / Zc) + c.cxc;
    p.v = c.fyc * (Yc / Zc) + c.cyc;
    return p;
}

// the point-mode target of a centre: false when it leaves the frame (a NaN fails every comparison)
__device__ __forceinline__ bool point_target(const Projected& c, const RegLaunch& L, unsigned& iu, unsigned& iv)
{
    const float fu = rintf(c.u), fv = rintf(c.v);           // ties to even, like depth_to_u16
    if (!(fu >= 0.0f && fu <= (float)(L.wc - 1) && fv >= 0.0f && fv <= (float)(L.hc - 1))) return false;
    iu = (unsigned)fu;
    iv = (unsigned)fv;
    return true;
}

// the integers i with min(a, b) <= i < max(a, b) inside 0 .. last, at most max_splat of them; a and b are no NaN
__device__ __forceinline__ bool splat_span(float a, float b, float last, int max_splat, int& i0, int& i1)
{
    const float lo = a < b ? a : b, hi = a < b ? b : a;
    const float f0 = fmaxf(ceilf(lo), 0.0f), f1 = fminf(ceilf(hi) - 1.0f, last);
    if (!(f0 <= f1)) return false;                          // 0 <= f0 <= f1 <= last from here
    i0 = (int)f0;
    i1 = (int)f1;
    if (i1 - i0 + 1 > max_splat) i1 = i0 + max_splat - 1;
    return true;
}

__device__ __forceinline__ void key_min(uint32_t* p, uint32_t key)
{
    (void)__hip_atomic_fetch_min(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void scatter_pixel(const RegLaunch& L, uint32_t* __restrict__ zb, unsigned u, unsigned v, float z)
{
    if (!(z > L.z_min && z < L.z_max)) return;
    const float fu = (float)u, fv = (float)v;
    const Projected c = project(fu, fv, z, L);
    if (!c.ok) return;
    const uint32_t key = __float_as_uint(c.z);
    if (L.max_splat == 0) {
        unsigned iu, iv;
        if (point_target(c, L, iu, iv)) key_min(zb + (size_t)iv * (unsigned)L.wc + iu, key);
        return;
    }
    const Projected a = project(fu - 0.5f, fv - 0.5f, z, L), b = project(fu + 0.5f, fv + 0.5f, z, L);
    if (!a.ok || !b.ok) return;
    if (a.u != a.u || a.v != a.v || b.u != b.u || b.v != b.v) return;
    int i0, i1, j0, j1;
    if (!splat_span(a.u, b.u, (float)(L.wc - 1), L.max_splat, i0, i1)) return;
    if (!splat_span(a.v, b.v, (float)(L.hc - 1), L.max_splat, j0, j1)) return;
    for (int j = j0; j <= j1; j++) {
        uint32_t* row = zb + (size_t)j * (unsigned)L.wc;
        for (int i = i0; i <= i1; i++) key_min(row + i, key);
    }
}

__device__ __forceinline__ const char* depth_frame(const RegLaunch& L, unsigned frame, unsigned px)
{
    return static_cast<const char*>(L.depth) + (size_t)frame * px * (L.depth_format == KDE_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float));
}

// whether the wave that owns the pixels base .. base + 255 of this frame reads them four per lane
__device__ __forceinline__ bool wave_vector_loads(const char* frame, int format, unsigned base, unsigned px)
{
    const uintptr_t mask = format == KDE_DEPTH_U16 ? 7u : 15u;
    return (reinterpret_cast<uintptr_t>(frame) & mask) == 0 && base + kWavePixels <= px;
}

// the pixels base + 4 * lane .. + 3 of an aligned frame; uint16 widened by (float)u, exact
template <bool NT>
__device__ __forceinline__ float4 load_quad(const char* frame, int format, unsigned base, unsigned lane)
{
    if (format == KDE_DEPTH_F32) return ld4(reinterpret_cast<const float4*>(frame) + base / 4 + lane, NT);
    const r_v2* p = reinterpret_cast<const r_v2*>(frame) + base / 4 + lane;
    const r_v2 w = NT ? __builtin_nontemporal_load(p) : *p;
    return make_float4((float)(w.x & 0xffffu), (float)(w.x >> 16), (float)(w.y & 0xffffu), (float)(w.y >> 16));
}

__device__ __forceinline__ float load_element(const char* frame, int format, unsigned p, unsigned px)
{
    if (p >= px) return NAN;                                // no range admits it
    return load_depth(frame, format == KDE_DEPTH_F32, p);
}

// R0: the grid of R2; every key of the frames in use becomes kEmpty (a thread its octet, two 16-byte stores)
__global__ __launch_bounds__(kThreads) void reg_reset_kernel(uint32_t* __restrict__ zbuf, unsigned px)
{
    const unsigned first = (blockIdx.x * kThreads + threadIdx.x) * kOctet;
    if (first >= px) return;
    uint4* q = reinterpret_cast<uint4*>(zbuf + (size_t)blockIdx.y * reg_zstride(px) + first);
    q[0] = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
    q[1] = make_uint4(kEmpty, kEmpty, kEmpty, kEmpty);
}

// R1: grid (blocks of 1024 source pixels, n), block 256
template <bool NT>
__global__ __launch_bounds__(kThreads) void reg_scatter_kernel(RegLaunch L)
{
    __shared__ float4 xch[kWaves][64];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)L.wd * (unsigned)L.hd;
    const unsigned frame = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) L.filled[frame] = 0u;      // R2 adds to it, behind the kernel boundary
    const unsigned base = blockIdx.x * kBlockPixels + wv * kWavePixels; // wave-uniform
    if (base >= px) return;
    const char* sframe = depth_frame(L, frame, px);
    float z[4];
    if (wave_vector_loads(sframe, L.depth_format, base, px)) {
        xch[wv][lane] = load_quad<NT>(sframe, L.depth_format, base, lane);
        wave_exchange_fence();
        const float* w = reinterpret_cast<const float*>(xch[wv]);
#pragma unroll
        for (unsigned k = 0; k < 4; k++) z[k] = w[64u * k + lane];
    } else {
#pragma unroll
        for (unsigned k = 0; k < 4; k++) z[k] = load_element(sframe, L.depth_format, base + 64u * k + lane, px);
    }
    uint32_t* zb = L.zbuf + (size_t)frame * reg_zstride((size_t)L.wc * L.hc);
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        const unsigned p = base + 64u * k + lane;
        if (p < px) {
            const unsigned v = p / (unsigned)L.wd, u = p - v * (unsigned)L.wd;
            scatter_pixel(L, zb, u, v, z[k]);
        }
    }
}

// R2: grid (blocks of 2048 keys, n), block 256
template <bool NT>
__global__ __launch_bounds__(kThreads) void reg_finalise_kernel(RegLaunch L)
{
    __shared__ uint32_t wave_count[kWaves];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)L.wc * (unsigned)L.hc;
    const unsigned frame = blockIdx.y;
    const unsigned first = (blockIdx.x * kThreads + threadIdx.x) * kOctet;
    uint32_t c = 0;
    if (first < px) {                                       // the octet lies inside the frame's reg_zstride keys
        const float4* zq = reinterpret_cast<const float4*>(L.zbuf + (size_t)frame * reg_zstride(px) + first);
        const float4 a = ld4(zq, NT), b = ld4(zq + 1, NT);  // keys: moved, not converted
        const uint32_t key[8] = {__float_as_uint(a.x), __float_as_uint(a.y), __float_as_uint(a.z), __float_as_uint(a.w),
                                 __float_as_uint(b.x), __float_as_uint(b.y), __float_as_uint(b.z), __float_as_uint(b.w)};
        uint32_t zc[8];                                     // Zc's bits, 0 where nothing came (a padding key was never touched)
#pragma unroll
        for (unsigned k = 0; k < kOctet; k++) {
            const bool reached = key[k] != kEmpty;
            c += reached ? 1u : 0u;
            zc[k] = reached ? key[k] : 0u;
        }
        const bool whole = first + kOctet <= px;
        if (L.out_format == KDE_DEPTH_F32) {
            float* o = static_cast<float*>(L.out) + (size_t)frame * px;
            if (whole && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
                float4* q = reinterpret_cast<float4*>(o + first);
                st4(q, make_float4(__uint_as_float(zc[0]), __uint_as_float(zc[1]), __uint_as_float(zc[2]), __uint_as_float(zc[3])), NT);
                st4(q + 1, make_float4(__uint_as_float(zc[4]), __uint_as_float(zc[5]), __uint_as_float(zc[6]), __uint_as_float(zc[7])), NT);
            } else {
#pragma unroll
                for (unsigned k = 0; k < kOctet; k++) {
                    if (first + k < px) reinterpret_cast<uint32_t*>(o)[first + k] = zc[k];
                }
            }
        } else {
            uint16_t* o = static_cast<uint16_t*>(L.out) + (size_t)frame * px;
            uint32_t d[8];
#pragma unroll
            for (unsigned k = 0; k < kOctet; k++) d[k] = depth_to_u16(__uint_as_float(zc[k]));
            if (whole && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
                st4(reinterpret_cast<float4*>(o + first),
                    make_float4(__uint_as_float(d[0] | (d[1] << 16)), __uint_as_float(d[2] | (d[3] << 16)),
                                __uint_as_float(d[4] | (d[5] << 16)), __uint_as_float(d[6] | (d[7] << 16))), NT);
            } else {
#pragma unroll
                for (unsigned k = 0; k < kOctet; k++) {
                    if (first + k < px) o[first + k] = (uint16_t)d[k];
                }
            }
        }
    }
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) c += (uint32_t)__shfl_xor((int)c, (int)off, 64);
    if (lane == 0) wave_count[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
        if (total) atomicAdd(&L.filled[frame], total);      // an integer sum: the same in any order
    }
}

// R3: grid (blocks of 1024 depth pixels, n), block 256.  No occlusion test: a depth pixel hidden from the colour camera
// takes the colour of whatever hides it.
template <bool NT>
__global__ __launch_bounds__(kThreads) void reg_gather_kernel(RegLaunch L, const uint8_t* __restrict__ bgr, int bgr_frames,
                                                              uint8_t* __restrict__ out)
{
    __shared__ uint32_t stage[kWaves][192];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)L.wd * (unsigned)L.hd;
    const unsigned frame = blockIdx.y;
    const unsigned base = blockIdx.x * kBlockPixels + wv * kWavePixels; // wave-uniform
    if (base >= px) return;
    const char* sframe = depth_frame(L, frame, px);
    float z[4];
    if (wave_vector_loads(sframe, L.depth_format, base, px)) {
        const float4 q = load_quad<NT>(sframe, L.depth_format, base, lane);
        z[0] = q.x; z[1] = q.y; z[2] = q.z; z[3] = q.w;
    } else {
#pragma unroll
        for (unsigned k = 0; k < 4; k++) z[k] = load_element(sframe, L.depth_format, base + 4u * lane + k, px);
    }
    const uint8_t* img = bgr + (bgr_frames == 1 ? (size_t)0 : (size_t)frame) * (size_t)L.wc * L.hc * 3;
    uint32_t c[4];                                          // b | g << 8 | r << 16, 0 where the pixel has no target
#pragma unroll
    for (unsigned k = 0; k < 4; k++) {
        const unsigned p = base + 4u * lane + k;
        c[k] = 0u;
        if (p < px && z[k] > L.z_min && z[k] < L.z_max) {
            const unsigned v = p / (unsigned)L.wd, u = p - v * (unsigned)L.wd;
            const Projected t = project((float)u, (float)v, z[k], L);
            unsigned iu, iv;
            if (t.ok && point_target(t, L, iu, iv)) {
                c[k] = pack_bgr(img + ((size_t)iv * (unsigned)L.wc + iu) * 3);
            }
        }
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
        for (unsigned j = 0; j < 3; j++) {
            if (NT) __builtin_nontemporal_store(w[64u * j + lane], d + 64u * j + lane);
            else d[64u * j + lane] = w[64u * j + lane];
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < 4; k++) {
            const unsigned p = base + 4u * lane + k;
            if (p < px) {
                o[3 * (size_t)p] = (uint8_t)c[k];
                o[3 * (size_t)p + 1] = (uint8_t)(c[k] >> 8);
                o[3 * (size_t)p + 2] = (uint8_t)(c[k] >> 16);
            }
        }
    }
}

}  // namespace

int launch_reg(const RegLaunch& a, hipStream_t s)
{
    const size_t pxd = (size_t)a.wd * a.hd, pxc = (size_t)a.wc * a.hc;
    const bool nt = past_cache(kSiteReg, (size_t)a.n * (pxd * depth_element(a.depth_format) + pxc * depth_element(a.out_format)));
    const dim3 block(kThreads);
    const dim3 sgrid((unsigned)((pxd + kBlockPixels - 1) / kBlockPixels), (unsigned)a.n);
    const dim3 fgrid((unsigned)((pxc + kThreads * kOctet - 1) / (kThreads * kOctet)), (unsigned)a.n);
    hipLaunchKernelGGL(reg_reset_kernel, fgrid, block, 0, s, a.zbuf, (unsigned)pxc);
    if (nt) {
        hipLaunchKernelGGL(reg_scatter_kernel<true>, sgrid, block, 0, s, a);
        hipLaunchKernelGGL(reg_finalise_kernel<true>, fgrid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL(reg_scatter_kernel<false>, sgrid, block, 0, s, a);
        hipLaunchKernelGGL(reg_finalise_kernel<false>, fgrid, block, 0, s, a);
    }
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

int launch_reg_gather(const RegLaunch& a, const uint8_t* bgr, int bgr_frames, uint8_t* out, hipStream_t s)
{
    const size_t pxd = (size_t)a.wd * a.hd, pxc = (size_t)a.wc * a.hc;
    const bool nt = past_cache(kSiteRegGather, (size_t)a.n * pxd * (depth_element(a.depth_format) + 3) + (size_t)bgr_frames * pxc * 3);
    const dim3 grid((unsigned)((pxd + kBlockPixels - 1) / kBlockPixels), (unsigned)a.n), block(kThreads);
    if (nt) hipLaunchKernelGGL(reg_gather_kernel<true>, grid, block, 0, s, a, bgr, bgr_frames, out);
    else hipLaunchKernelGGL(reg_gather_kernel<false>, grid, block, 0, s, a, bgr, bgr_frames, out);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
