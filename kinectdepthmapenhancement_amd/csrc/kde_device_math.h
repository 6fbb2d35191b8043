// kde_device_math.h — small device functions shared by the product kernels and the test-hook library
// (tools/hooks/test_hooks.hip), so that a test can call exactly the code a kernel runs.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace kde {

// A depth in millimetres as the sensor's uint16 (OpenNI XnDepthPixel, 0 = invalid): rounded half to even, and 0 for
// everything that is not a depth the format holds -- NaN, +-inf, z < 0.5, z >= 65535.5.  The exact inverse of the
// (float)u widening of launch_widen_u16: every integer-valued z in 1..65535 comes back as itself.  One function for the
// kernels (stream_kernels.hip) and the host, so that a CPU test checks the rule the kernels run.
__host__ __device__ inline uint16_t depth_to_u16(float z)
{
    const float r = rintf(z);
    return (r >= 1.0f && r <= 65535.0f) ? (uint16_t)r : (uint16_t)0;
}

// ---- depth frames of either format, guide colours, counts (reg, undist, upsample, holefill kernels) -----------------------
// Element `at` of a depth frame that holds floats (is_f32) or the sensor's uint16, widened by (float)u: exact
__device__ __forceinline__ float load_depth(const char* frame, bool is_f32, size_t at)
{
    return is_f32 ? reinterpret_cast<const float*>(frame)[at] : (float)reinterpret_cast<const uint16_t*>(frame)[at];
}

__device__ __forceinline__ void store_depth(char* frame, bool is_f32, size_t at, float z)
{
    if (is_f32) reinterpret_cast<float*>(frame)[at] = z;
    else reinterpret_cast<uint16_t*>(frame)[at] = depth_to_u16(z);
}

// ---- the depth link of DepthSpeckleFilter and OrganizedMesh (speckle_kernels.hip, mesh_kernels.hip) ------------------------
// |za - zb| <= max_diff + rel_diff * min(za, zb) for two depths that are both valid: one subtraction, one product, one sum,
// each rounded on its own (-ffp-contract=off)
__device__ __forceinline__ bool depth_close(float za, float zb, float max_diff, float rel_diff)
{
    const float m = rel_diff * fminf(za, zb);
    const float t = max_diff + m;
    return fabsf(za - zb) <= t;
}

// the link of the speckle rule: a state of 0 is an invalid pixel and links to nothing
__device__ __forceinline__ bool linked(float za, float zb, float max_diff, float rel_diff)
{
    if (!(za > 0.0f && zb > 0.0f)) return false;
    return depth_close(za, zb, max_diff, rel_diff);
}

// a packed BGR pixel as b | g << 8 | r << 16: |db| + |dg| + |dr| of two of them is one v_sad_u8
__device__ __forceinline__ uint32_t pack_bgr(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

// The sum of v over a workgroup of 256 threads, in two steps so that only the threads that want it read it: the sums of the
// four waves meet in part[4] (LDS nobody else uses) behind one barrier; block_sum_u32(part) is then their sum.  An integer
// sum: the same in any order.  (Where the compiler's code for a kernel moved with them, that kernel spells the steps out.)
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)off, 64);
    return v;
}
__device__ __forceinline__ void block_partials_u32(uint32_t v, uint32_t* part)
{
    v = wave_sum_u32(v);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
}
__device__ __forceinline__ uint32_t block_sum_u32(const uint32_t* part) { return (part[0] + part[1]) + (part[2] + part[3]); }

// sqrtf() of an integer-valued float in [0, 2^24): v_rsq_f32 estimate, one Heron step on the exact fma residual.
// The library sqrtf() spends 14 instructions (denormal scaling, two +-1 ulp probes, class test) to be correctly
// rounded for every float; on this domain 6 are enough -- tests/test_gpu_dasp_ers.py checks ALL 2^24 arguments
// against sqrtf bit for bit (px*px + py*py of pixel offsets, the only argument K7 has, is such an integer).
__device__ __forceinline__ float sqrt_int24(float x)
{
    const float y = __builtin_amdgcn_rsqf(x);          // 1/sqrt(x), 1 ulp; +inf for x == 0
    const float r = x * y;
    const float e = __builtin_fmaf(-r, r, x);          // exact residual x - r^2
    const float r1 = __builtin_fmaf(e, 0.5f * y, r);
    return x == 0.0f ? 0.0f : r1;
}

// expf() for the reference-shaped kernels.  The reference's rule "a factor that underflowed to exactly 0 is skipped"
//  is stated for an expf() that rounds to the binary32 denormal grid: 0 iff the true value is below 2^-150
// (x < -150 ln 2 = -103.972).  The library expf() returns 0 as soon as the true value is below the smallest denormal
// 2^-149 (x < -103.28), so a weight of half a unit to one unit of the grid would be lost.  Below -64 the argument is
// shifted by 64 and the (normal) result multiplied by e^-64: that product is rounded to the denormal grid once.
__device__ __forceinline__ float exp_denormal(float x)
{
    const bool shifted = x < -64.0f;
    const float r = expf(shifted ? x + 64.0f : x);
    return shifted ? r * 0x1.969d48p-93f : r;
}

// x / d for 0 <= x < 2^24 by a multiplication: with l = ceil(log2 d), m = floor(2^(24+l) / d) + 1 and sh = 24 + l,
// floor(x * m / 2^sh) == floor(x / d) (m * d = 2^sh + e with 0 < e <= 2^l, so the product overshoots x / d by less than
// 1 / d).  Two instructions (v_mad_u64_u32, v_lshrrev_b64) instead of the ~20 of a 32-bit division.  ok == 0 (operands
// beyond the proven range) falls back to the division.
struct FastDiv24 {
    uint32_t m, sh, d, ok;
};
inline FastDiv24 make_fastdiv24(uint32_t d, uint64_t max_dividend)
{
    FastDiv24 f{0u, 0u, d, 0u};
    if (d == 0 || d >= (1u << 24) || max_dividend >= (1ull << 24)) return f;
    uint32_t l = 0;
    while ((1u << l) < d) l++;
    f.sh = 24 + l;
    f.m = (uint32_t)((1ull << f.sh) / d + 1);      // < 2^(25+l) / d + 1 <= 2^25 + 1: fits
    f.ok = 1;
    return f;
}
__device__ __forceinline__ uint32_t fastdiv24(uint32_t x, const FastDiv24& f)
{
    return f.ok ? (uint32_t)(((uint64_t)x * f.m) >> f.sh) : x / f.d;
}

// DimensionConvertor's camera (DimensionConvertor.cpp:3-13): cx, cy truncated to int as the reference stores them
struct Camera {
    float fx, fy;
    int cx, cy;
    int width, height;
};

// ---- DimensionConvertor: projectiveToReal of one pixel ------------------------------------------------------------------
// One function for stream_kernels.hip (K2) and error3d_kernels.hip (a depth-map source of the quality metric), so that a
// term computed from a depth map has the bits the float3 cloud of that map would give.
__device__ __forceinline__ void convert_ptr(float& x, float& y, float z, const Camera& c)
{
    // DimensionConvertor.h:34-48 — subtract, divide, multiply (in that order)
    y = (float)c.cy - y;
    x = x - (float)c.cx;
    x /= c.fx;
    y /= c.fy;
    x *= z;
    y *= z;
}

__device__ __forceinline__ void p2r_one(const Camera& c, int interp, unsigned x, unsigned y, float z, float* r)
{
    float fx_, fy_;
    if (!interp) {
        // convert_ptr(tuple<float,int>), DimensionConvertor.h:51-62
        fy_ = (float)(int)y;
        fx_ = (float)(int)x;
        convert_ptr(fx_, fy_, z, c);
    } else {
        // convert_ptr_int, DimensionConvertor.h:80-103 (half-pixel grid, index decomposed over 2*width)
        fy_ = (float)(int)y;
        fx_ = (float)(int)x;
        fy_ = (float)c.cy - fy_ / 2.0f;
        fx_ = fx_ / 2.0f - (float)c.cx;
        fx_ /= c.fx;
        fy_ /= c.fy;
        fx_ *= z;
        fy_ *= z;
    }
    r[0] = fx_;
    r[1] = fy_;
    r[2] = z;
}

// ---- packed float3 through LDS, streaming accesses (stream_kernels.hip, error3d_kernels.hip) ---------------------------------
// A thread owns 4 pixels = 48 B of packed float3, which it could only load or store as three 16-byte
// pieces 48 B apart.  Each wave therefore passes its 3 KB through LDS once, so that every global store
// (and, for the float3 -> float3 maps, every load) instruction moves 64 consecutive float4 = 1 KB.
// LDS instructions of one wave execute in issue order, so a wave-level compiler barrier is all that is
// needed between the write and the transposed read.
__device__ __forceinline__ void wave_exchange_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// NT: streaming (non-temporal) loads and stores, used when the call moves more than the 256 MB Infinity Cache can
// hold anyway (a batch); single frames keep default caching so that the next kernel of the chain reads them on-chip.
typedef float s_v4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float4* p, bool nt)
{
    if (!nt) return *p;
    const s_v4 v = __builtin_nontemporal_load(reinterpret_cast<const s_v4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st4(float4* p, float4 v, bool nt)
{
    if (nt) __builtin_nontemporal_store(s_v4{v.x, v.y, v.z, v.w}, reinterpret_cast<s_v4*>(p));
    else *p = v;
}

// Workgroups are dealt round-robin over the 8 XCDs, each with its own L2.  Mapping workgroup `lin` of `nblk` to the
// tile xcd_band_id(lin, nblk) gives XCD k the k-th contiguous eighth of the (raster-ordered) tile list, so the halo
// rows two neighbouring tiles share are fetched into one L2 instead of two.  Bijective for any nblk.
__device__ __forceinline__ unsigned xcd_band_id(unsigned lin, unsigned nblk)
{
    const unsigned per = nblk / 8, rem = nblk % 8;
    const unsigned xcd = lin % 8, slot = lin / 8;
    return xcd * per + (xcd < rem ? xcd : rem) + slot;
}

}  // namespace kde
