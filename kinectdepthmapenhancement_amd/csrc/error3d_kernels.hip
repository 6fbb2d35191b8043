// error3d_kernels.hip — MeanError3D: the reference's quality figure (main.cpp:220-308) for n frames x m candidates against
// one truth, as two launches and no float atomics.
//   E1 partial sums  one workgroup reduces one segment of kError3dSegmentPixels pixels of one frame for every candidate:
//                    the truth is read once per pixel and held in registers while the m candidates pass by
//   E2 final         one wave per (frame, candidate) adds that pair's partials and writes the kde_error3d_result
// Every order is fixed by the pixel index alone: thread t of a segment owns the pixel octet t of it, walks it
// in raster order and adds the float32 terms to a binary64 sum; the lanes of a wave meet in a xor butterfly (32, 16, .. 1),
// the waves of the workgroup in wave order, the partials of a frame in a stride-64 walk and the same butterfly.  Nothing of
// that depends on n, m, the frame's place in the batch, the candidate's place among the m, or on which loads fetched the
// pixels, so a (frame, candidate) record has the same bytes in every call that holds that pair.
// A frame that starts on a 16-byte boundary is read with 16-byte loads (packed float3 through LDS as in stream_kernels.hip);
// any other frame -- a pointer with only its element's alignment, or the later frames of a batch whose frame size is odd --
// with element loads.  Both paths fill the same registers.
#include "kde_internal.h"
#include "kde_device_math.h"
#include "kde_source_load.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kSegmentOctets = kError3dSegmentPixels / 8;
constexpr unsigned kOctetsPerThread = kSegmentOctets / kThreads;
static_assert(kOctetsPerThread * kThreads * 8 == kError3dSegmentPixels, "a segment is a whole number of octets per thread");

// lanes of a wave in a fixed xor butterfly: every lane ends with the same total
__device__ __forceinline__ void wave_sum(double& s, uint32_t& k)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        k += (uint32_t)__shfl_xor((int)k, off, 64);
    }
}

// E1: grid (segments of a frame, n); block 256.  Error3dLaunch travels as the kernel's argument block: the m descriptors are
// read on the host at call time and nothing is uploaded.  Without a register target the compiler takes 170 registers (two
// waves per SIMD); the target of three waves gives 161 without a spill, a target of four spills (EXPERIMENTS.md).
template <bool NT>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 8))) void error3d_partial_kernel(Error3dLaunch a)
{
    __shared__ float4 xch[kWaves][6 * 64];
    __shared__ double red_sum[kWaves][kError3dMaxCandidates];
    __shared__ uint32_t red_count[kWaves][kError3dMaxCandidates];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)a.cam.width * (unsigned)a.cam.height;
    const unsigned seg = blockIdx.x, frame = blockIdx.y;
    const char* tframe = static_cast<const char*>(a.truth) +
                         (a.truth_frames == 1 ? (size_t)0 : (size_t)frame) * px * source_element_size(a.truth_format);
    const bool tvec = (reinterpret_cast<uintptr_t>(tframe) & 15u) == 0;
    // the truth of the thread's pixels, read once and held while the candidates pass by
    float T[kOctetsPerThread][24];
    bool tv[kOctetsPerThread][8];
#pragma unroll
    for (unsigned j = 0; j < kOctetsPerThread; j++) {
        const unsigned oct0 = seg * kSegmentOctets + j * kThreads + wv * 64u;   // wave-uniform
        load_octet<NT>(tframe, a.truth_format, tvec, oct0, lane, px, a.cam, xch[wv], T[j]);
#pragma unroll
        for (int k = 0; k < 8; k++) tv[j][k] = T[j][3 * k + 2] > a.z_min && T[j][3 * k + 2] < a.z_max;
    }
#pragma unroll 1
    for (int c = 0; c < a.m; c++) {
        const void* cbase = a.cand[0];              // the c-th descriptor of the argument block, by scalar selects
        int cformat = a.cand_format[0];
#pragma unroll
        for (int i = 1; i < kError3dMaxCandidates; i++) {
            if (c == i) {
                cbase = a.cand[i];
                cformat = a.cand_format[i];
            }
        }
        const char* cframe = static_cast<const char*>(cbase) + (size_t)frame * px * source_element_size(cformat);
        const bool cvec = (reinterpret_cast<uintptr_t>(cframe) & 15u) == 0;
        double sum = 0.0;
        uint32_t count = 0;
#pragma unroll
        for (unsigned j = 0; j < kOctetsPerThread; j++) {
            const unsigned oct0 = seg * kSegmentOctets + j * kThreads + wv * 64u;
            float P[24];
            load_octet<NT>(cframe, cformat, cvec, oct0, lane, px, a.cam, xch[wv], P);
#pragma unroll
            for (int k = 0; k < 8; k++) {
                // main.cpp:233-244: both points inside (z_min, z_max), then sqrtf of the three squared differences
                if (tv[j][k] && P[3 * k + 2] > a.z_min && P[3 * k + 2] < a.z_max) {
                    const float dz = P[3 * k + 2] - T[j][3 * k + 2], dy = P[3 * k + 1] - T[j][3 * k + 1], dx = P[3 * k] - T[j][3 * k];
                    const float e = sqrtf((dz * dz + dy * dy) + dx * dx);
                    sum += (double)e;
                    count++;
                }
            }
        }
        wave_sum(sum, count);
        if (lane == 0) {
            red_sum[wv][c] = sum;
            red_count[wv][c] = count;
        }
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)a.m) {
        const unsigned c = threadIdx.x;
        Error3dPartial r{red_sum[0][c], red_count[0][c], 0u};
        for (int w = 1; w < kWaves; w++) {            // wave order
            r.sum += red_sum[w][c];
            r.count += red_count[w][c];
        }
        a.partials[((size_t)frame * a.m + c) * gridDim.x + seg] = r;
    }
}

// E2: grid n * m, block 64: lane l adds the partials l, l + 64, ... of its (frame, candidate), then the butterfly
__global__ __launch_bounds__(64) void error3d_final_kernel(const Error3dPartial* __restrict__ partials, unsigned segs,
                                                          kde_error3d_result* __restrict__ results)
{
    const Error3dPartial* p = partials + (size_t)blockIdx.x * segs;
    double s = 0.0;
    uint32_t k = 0;
    for (unsigned i = threadIdx.x; i < segs; i += 64u) {
        s += p[i].sum;
        k += p[i].count;
    }
    wave_sum(s, k);
    if (threadIdx.x == 0) {
        kde_error3d_result r;
        r.sum = s;
        r.count = k;
        r.mean = (float)(s / (double)k);              // count == 0: 0.0 / 0.0 = NaN, the reference's 0.0f / 0 (main.cpp:304-308)
        results[blockIdx.x] = r;
    }
}

}  // namespace

int launch_error3d(const Error3dLaunch& a, hipStream_t s)
{
    const size_t px = (size_t)a.cam.width * a.cam.height;
    const unsigned segs = error3d_segments(px);
    auto esz = [](int f) { return f == KDE_SRC_POINTS_F32 ? sizeof(kde_float3) : f == KDE_SRC_DEPTH_F32 ? sizeof(float) : sizeof(uint16_t); };
    size_t bytes = px * a.truth_frames * esz(a.truth_format);
    for (int c = 0; c < a.m; c++) bytes += px * a.n * esz(a.cand_format[c]);
    const dim3 grid(segs, (unsigned)a.n), block(kThreads);
    if (past_cache(kSiteError3d, bytes)) hipLaunchKernelGGL(error3d_partial_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(error3d_partial_kernel<false>, grid, block, 0, s, a);
    hipLaunchKernelGGL(error3d_final_kernel, dim3((unsigned)(a.n * a.m)), dim3(64), 0, s, a.partials, segs, a.results);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
