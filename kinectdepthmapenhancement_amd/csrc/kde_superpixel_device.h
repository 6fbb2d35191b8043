// kde_superpixel_device.h — what the two superpixel segmenters share on the device: dasp_kernels.hip
// (DepthAdaptiveSuperpixel.cu) and nasp_kernels.hip (NormalAdaptiveSuperpixel.cu).  The member walks of their cluster
// kernels differ on purpose (chunked 16-byte label loads against walk_members) and stay in their files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/kde_hip.h"

namespace kde {

// ---- argmin updates without the v_cndmask stall ---------------------------------------------------------------------
// "take = d < best; best = take ? d : best; label = take ? id : label" compiles to one v_cmp and TWO back-to-back
// v_cndmask_b32 in the VOP2 encoding (condition implicitly in VCC) -- and on gfx950 the second of two adjacent VOP2 v_cndmask
// stalls the SIMD for ~20 cycles (tools/valu_microbench: "1 v_cmp + 2 v_cndmask (vcc)" 3.2-6.8 ns per instruction against
// 1.3 with one other VALU instruction between them and 1.7 in the VOP3 encoding; profiles/r04_valu_microbench_vcc.txt).
// The argmin update therefore keeps its condition in an SGPR pair and selects with the VOP3 form: same results, no stall.
// (A 64-bit SGPR pair is the condition of a 64-wide wavefront: this library is built for gfx950 only, see the Makefile.)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "kde_superpixel_device.h: the SGPR-pair conditions below assume gfx950 (wave64); build with --offload-arch=gfx950"
#endif
__device__ __forceinline__ uint64_t lt_mask(float x, float y)
{
    uint64_t m;
    asm("v_cmp_lt_f32_e64 %0, %1, %2" : "=s"(m) : "v"(x), "v"(y));
    return m;
}
__device__ __forceinline__ float sel_f(uint64_t m, float a, float b)       // m ? a : b
{
    float r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
    return r;
}
__device__ __forceinline__ int sel_i(uint64_t m, int a, int b)
{
    int r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
    return r;
}

__device__ __forceinline__ int f2i_rz(float v) { return (int)v; }   // v_cvt_i32_f32: RZ, saturating, NaN -> 0

// ---- the 256-way tree of the cluster kernels ------------------------------------------------------------------------
// (DepthAdaptiveSuperpixel.cu:425-528; NormalAdaptiveSuperpixel.cu:457-621, :825-999)
// The reference's summation order -- per-thread serial, then this tree -- is what the float sums depend on bit for bit:
// levels +128, +64 through LDS (DepthAdaptiveSuperpixel.cu:425-454), +32 ... +1 inside the first wavefront (.cu:455-528);
// lane 0 of it sees the clean tree (the other lanes
// of that wavefront hold partial sums nobody reads, as in the reference's lock-step warp).
// Integer sums wrap as the reference's 32-bit adds do.  buf: (NI + NF) x 256 words of LDS, integer rows first.
template <int NI, int NF>
__device__ __forceinline__ void tree256(int tid, uint32_t (*buf)[256], int* iv, float* fv)
{
    int(*si)[256] = reinterpret_cast<int(*)[256]>(buf);
    float(*sf)[256] = reinterpret_cast<float(*)[256]>(buf + NI);
#pragma unroll
    for (int k = 0; k < NI; k++) si[k][tid] = iv[k];
#pragma unroll
    for (int k = 0; k < NF; k++) sf[k][tid] = fv[k];
    __syncthreads();
    if (tid < 128) {
#pragma unroll
        for (int k = 0; k < NI; k++) si[k][tid] = (int)((unsigned)si[k][tid] + (unsigned)si[k][tid + 128]);
#pragma unroll
        for (int k = 0; k < NF; k++) sf[k][tid] += sf[k][tid + 128];
    }
    __syncthreads();
    if (tid < 64) {
#pragma unroll
        for (int k = 0; k < NI; k++) iv[k] = (int)((unsigned)si[k][tid] + (unsigned)si[k][tid + 64]);
#pragma unroll
        for (int k = 0; k < NF; k++) fv[k] = sf[k][tid] + sf[k][tid + 64];
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
#pragma unroll
            for (int k = 0; k < NI; k++) iv[k] = (int)((unsigned)iv[k] + (unsigned)__shfl_down(iv[k], step, 64));
#pragma unroll
            for (int k = 0; k < NF; k++) fv[k] += __shfl_down(fv[k], step, 64);
        }
    }
}

// ---- from the reduced sums to the new cluster record ----------------------------------------------------------------
// (DepthAdaptiveSuperpixel.cu:530-566; NormalAdaptiveSuperpixel.cu:623-683, :1001-1066)
// a channel mean as the record's byte: clamped to 0..255
__device__ __forceinline__ uint8_t channel_mean(int q)
{
    q = q > 255 ? 255 : q;
    return (uint8_t)(q < 0 ? 0 : q);
}
// sum / npoints of a float3 (cluster centre, cluster normal)
__device__ __forceinline__ kde_float3 mean3(float sx, float sy, float sz, int np)
{
    return kde_float3{sx / (float)np, sy / (float)np, sz / (float)np};
}
// The pixel under the new centre c, through the intrinsics.  A projection outside the image falls back to (fb_x, fb_y), the
// mean position of the members -- but the row test reads pix_y <= height (sic, DepthAdaptiveSuperpixel.cu:549,
// NormalAdaptiveSuperpixel.cu:652, :1031): every row inside the image falls back too, and a row BELOW it is kept.
__device__ __forceinline__ void reproject_centre(const kde_float3& c, const float* __restrict__ intr, int width, int height, int fb_x,
                                                 int fb_y, int& pix_x, int& pix_y)
{
    const float nx = c.x / c.z, ny = c.y / c.z;
    pix_x = f2i_rz(nx * intr[0] + intr[2]);
    pix_y = f2i_rz(intr[5] - ny * intr[4]);
    if (pix_x < 0 || pix_x >= width || pix_y < 0 || pix_y <= height) {
        pix_x = fb_x;
        pix_y = fb_y;
    }
}

}  // namespace kde
