// proj_kernels.hip — Projection_GPU::PlaneProjection(nd, labels, variance, points, size), the five-argument overload, on gfx950.
// Reference: Projection_GPU/Projection_GPU.cu:21-54 (setPsuedoDepth), :188-211 (variance_optimization), :213-246
// (bilateralfilter), :248-272 (the call: 3 kernels and a device copy per frame); definition and the deviations P1-P5 in
// DESIGN.md ("Plane projection (five-argument)").  Comparable with tools/proj_ref.c, which states the same result one
// reference kernel at a time.
//
// Only z evolves between setPsuedoDepth and bilateralfilter, and each of the first three steps reads and writes the pixel's
// own entry alone, so they are one pass:
//   proj_pixel_kernel      label, (n, d), point, ray and two table look-ups in; plane-fitted point and pre-filter z out.
//   proj_bilateral_kernel  the window on an LDS tile of the pre-filter z with a window/2 halo (P4: every tap reads what the
//                          first pass left); a tap outside the frame is stored as 0, which the reference's own z > 50 test
//                          rejects, so the inner loop has one test.  Writes packed (ray * z, z).
// Two launches per batch, the frame is a grid dimension; no atomics, no fill, no allocation.
#include "kde_internal.h"
#include "kde_device_math.h"

namespace kde {
namespace {

constexpr int kPixThreads = 256;
// 64 x 16 pixels per workgroup of 256 threads (4 rows per thread, lanes along x: LDS rows are read at consecutive
// addresses, conflict-free).  The largest tile, window 15, is 78 x 30 floats = 9360 B, with the spatial table 10260 B, so
// LDS never limits occupancy (8 workgroups of 4 waves per CU need 82 KB of 160 KB); the default window 7 re-reads
// (70 * 22) / (64 * 16) = 1.5 x the frame's z, from L2.
constexpr int kTileW = 64, kTileH = 16, kBilThreads = 256;
constexpr int kRowStep = kBilThreads / kTileW;

__device__ __forceinline__ bool in_table(int label, int nc) { return (unsigned)label < (unsigned)nc; }   // P1

// grid = (ceil(W*H / 256), frames)
__global__ __launch_bounds__(kPixThreads) void proj_pixel_kernel(ProjLaunch a)
{
    const int npix = a.width * a.height;
    const int p = blockIdx.x * kPixThreads + threadIdx.x;
    if (p >= npix) return;
    const int f = blockIdx.y;
    const size_t i = (size_t)f * npix + p;
    const int l = a.labels[i];
    const bool labelled = in_table(l, a.nc);
    const float v = labelled ? a.variance[(size_t)f * a.nc + l] : 0.0f;
    const bool planar = labelled && v <= 1.0f && v > a.thr;               // P3: acos(v) < max_angle
    const kde_float3 in = a.pts[i];
    kde_float3 pf = in;
    if (planar) {                                                         // setPsuedoDepth, .cu:38-48
        const float4 nd = a.nd[i];
        const float2 ray = a.nxy[p];
        pf.z = fabsf(nd.w / ((nd.x * ray.x + nd.y * ray.y) + nd.z));
        pf.x = pf.z * ray.x;
        pf.y = pf.z * ray.y;
    }
    a.plane_fitted[i] = pf;
    float z = in.z;                                                       // P5: Optimized = points (.cu:255)
    if (pf.z > 50.0f) {                                                   // variance_optimization, .cu:201-209
        const float diff = fabsf(z - pf.z);
        if (diff < z * 0.03f && planar && a.size[(size_t)f * a.nc + l] > a.min_size)
            z = diff < z * 0.01f ? pf.z : pf.z * v + z * (1.0f - v);
    }
    a.z[i] = z;
}

// grid = (ceil(W / 64), ceil(H / 16), frames).  WIN > 0: the window is a compile-time constant (the reference's 7);
// WIN == 0: a.window at run time.  Same operations in the same order either way.
template <int WIN>
__global__ __launch_bounds__(kBilThreads) void proj_bilateral_kernel(ProjLaunch a)
{
    __shared__ float tile[(kTileW + kProjMaxWindow - 1) * (kTileH + kProjMaxWindow - 1)];
    __shared__ float spatial[kProjMaxWindow * kProjMaxWindow];
    const int window = WIN > 0 ? WIN : a.window, r = window / 2;
    const int W = a.width, H = a.height, f = blockIdx.z;
    const size_t fpx = (size_t)f * W * H;
    const float* __restrict__ zin = a.z + fpx;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int tw = kTileW + 2 * r, th = kTileH + 2 * r;
    for (int t = threadIdx.x; t < tw * th; t += kBilThreads) {
        const int ty = t / tw, tx = t - ty * tw;
        const int gx = x0 + tx - r, gy = y0 + ty - r;
        tile[t] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? zin[(size_t)gy * W + gx] : 0.0f;
    }
    for (int t = threadIdx.x; t < window * window; t += kBilThreads) spatial[t] = a.spatial[t];
    __syncthreads();
    const int lx = threadIdx.x & (kTileW - 1);
    const int x = x0 + lx;
    if (x >= W) return;
    for (int ly = threadIdx.x / kTileW; ly < kTileH; ly += kRowStep) {
        const int y = y0 + ly;
        if (y >= H) return;
        const float zc = tile[(ly + r) * tw + lx + r];
        float numerator = 0.0f, denominator = 0.0f;                       // bilateralfilter, .cu:224-242
        for (int i = 0; i < window; i++) {
            const float* row = tile + (ly + i) * tw + lx;
#pragma unroll
            for (int j = 0; j < window; j++) {
                const float zt = row[j];
                if (zt > 50.0f) {
                    const float d = zt - zc;
                    float filter = exp_denormal(-(d * d) / a.depth_den);
                    filter *= spatial[i * window + j];
                    numerator += zt * filter;
                    denominator += filter;
                }
            }
        }
        const float zo = denominator == 0.0f ? 0.0f : numerator / denominator;
        const float2 ray = a.nxy[(size_t)y * W + x];
        a.optimized[fpx + (size_t)y * W + x] = kde_float3{ray.x * zo, ray.y * zo, zo};
    }
}

}  // namespace

int launch_proj_plane_projection(const ProjLaunch& a, hipStream_t s)
{
    const int npix = a.width * a.height;
    hipLaunchKernelGGL(proj_pixel_kernel, dim3(ceil_div(npix, kPixThreads), a.n), dim3(kPixThreads), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    const dim3 grid(ceil_div(a.width, kTileW), ceil_div(a.height, kTileH), a.n);
    if (a.window == 7) hipLaunchKernelGGL(proj_bilateral_kernel<7>, grid, dim3(kBilThreads), 0, s, a);
    else hipLaunchKernelGGL(proj_bilateral_kernel<0>, grid, dim3(kBilThreads), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
