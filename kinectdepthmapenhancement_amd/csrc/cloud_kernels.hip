// cloud_kernels.hip — PointCloudXYZRGB: the output step of the reference (main.cpp:211-300) for n frames of one method: the
// organised float3 grid and the colour image become 16-byte XYZRGB records, the valid ones compacted in raster order.
//   C1 count    one workgroup counts the valid pixels of one segment of kCloudSegmentPixels pixels of one frame
//   C2 scan     one workgroup per frame: exclusive scan of the frame's segment counts, kCloudScanThreads per pass with a
//               running carry; the total is count[f]
//   C3 scatter  the grid of C1: every wave ranks its valid pixels (a wave scan of the per-lane counts of 8 consecutive
//               pixels), gathers their records in LDS in that order and stores them at slot + segment offset + the counts
//               of the waves before it, 64 consecutive records per store instruction
// Organised mode is C3's kernel without the ranks: every pixel's record goes to its own place and the counts of the
// workgroups meet in one integer atomicAdd per workgroup on count[f] (zeroed by a memset node in front of the launch).
// No workgroup waits for another inside a launch and no position comes from an atomic, so the records are a function of the
// frame alone: the same bytes for any batch size, place in the batch and pointer alignment.
// Thread t of a segment owns the pixel octet t, as in error3d_kernels.hip, and reads it with the same load_octet
// (kde_source_load.h): 16-byte loads where the frame starts on a 16-byte boundary, element loads elsewhere.
#include "kde_internal.h"
#include "kde_device_math.h"
#include "kde_source_load.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kSegmentOctets = kCloudSegmentPixels / 8;
static_assert(kSegmentOctets == kThreads, "a thread owns one octet of its segment");
static_assert(kCloudScanThreads == 256, "C2 is written for four waves");
constexpr unsigned kWavePixels = 64 * 8;

typedef unsigned u_v4 __attribute__((ext_vector_type(4)));

// A record travels as four 32-bit words (the packed colour is a denormal when read as a float: no float instruction sees it)
__device__ __forceinline__ void store_record(kde_cloud_point* p, uint4 v, bool nt)
{
    if (nt) __builtin_nontemporal_store(u_v4{v.x, v.y, v.z, v.w}, reinterpret_cast<u_v4*>(p));
    else *reinterpret_cast<uint4*>(p) = v;
}

// Where record p of a wave's 512 sits in its LDS buffer: the record's place within its group of eight is rotated by the
// group's index, so that the lanes of an organised write (p = 8 * lane + k, k fixed) spread over all eight 16-byte slots of
// a bank row instead of meeting in one
__device__ __forceinline__ unsigned stage_slot(unsigned p) { return (p & ~7u) | ((p + (p >> 3)) & 7u); }

__device__ __forceinline__ bool cloud_valid(float z, const CloudLaunch& a) { return z > a.z_min && z < a.z_max; }   // main.cpp:227

// The colours of the pixels 8 * oct .. 8 * oct + 7 as PCL's packed rgb, (r << 16) | (g << 8) | b (main.cpp:223-225): the
// three bytes of a packed BGR pixel read as one little-endian 24-bit number.  A frame on an 8-byte boundary is read with
// three 8-byte loads per whole octet, any other frame and the partial last octet byte by byte; a pixel beyond the frame gets 0.
__device__ __forceinline__ void load_colour(const uint8_t* __restrict__ frame, bool vec, unsigned oct, unsigned px, uint32_t (&rgb)[8])
{
    const uint8_t* c = frame + 24 * (size_t)oct;
    if (vec && oct < px / 8) {
        const uint2* q = reinterpret_cast<const uint2*>(c);
        const uint2 q0 = q[0], q1 = q[1], q2 = q[2];
        const uint32_t w[7] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, 0u};
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            const unsigned i = (3 * k) >> 2, sh = 8 * ((3 * k) & 3);
            const uint64_t pair = ((uint64_t)w[i + 1] << 32) | w[i];
            rgb[k] = (uint32_t)(pair >> sh) & 0xffffffu;
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            rgb[k] = 0u;
            if (oct * 8 + k < px) rgb[k] = ((uint32_t)c[3 * k + 2] << 16) | ((uint32_t)c[3 * k + 1] << 8) | (uint32_t)c[3 * k];
        }
    }
}

// main.cpp:228-231: the record of a valid point; an invalid one (organised mode) is three quiet NaNs and its colour
__device__ __forceinline__ uint4 cloud_record(const float* p, uint32_t rgb, bool valid, const CloudLaunch& a)
{
    const float x = p[0] / a.divisor, y = p[1] / a.divisor, q = p[2] / a.divisor;
    const float z = a.negate_z ? -q : q;
    const uint32_t nan = 0x7fc00000u;
    return valid ? make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), rgb) : make_uint4(nan, nan, nan, rgb);
}

// inclusive scan over the lanes of a wave
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, unsigned lane)
{
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

__device__ __forceinline__ const char* source_frame(const CloudLaunch& a, unsigned frame, unsigned px)
{
    return static_cast<const char*>(a.src) + (size_t)frame * px * source_element_size(a.format);
}

// C1: grid (segments of a frame, n), block 256
template <bool NT>
__global__ __launch_bounds__(kThreads) void cloud_count_kernel(CloudLaunch a)
{
    __shared__ float4 xch[kWaves][6 * 64];
    __shared__ uint32_t wave_count[kWaves];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)a.cam.width * (unsigned)a.cam.height;
    const unsigned seg = blockIdx.x, frame = blockIdx.y;
    const char* sframe = source_frame(a, frame, px);
    const bool vec = (reinterpret_cast<uintptr_t>(sframe) & 15u) == 0;
    float P[24];
    load_octet<NT>(sframe, a.format, vec, seg * kSegmentOctets + wv * 64u, lane, px, a.cam, xch[wv], P);
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) c += cloud_valid(P[3 * k + 2], a) ? 1u : 0u;
    c = wave_scan(c, lane);
    if (lane == 63) wave_count[wv] = c;
    __syncthreads();
    if (threadIdx.x == 0) a.seg[(size_t)frame * gridDim.x + seg] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
}

// C2: grid n, block kCloudScanThreads: the frame's counts become the offsets of its segments, in place
__global__ __launch_bounds__(kCloudScanThreads) void cloud_scan_kernel(uint32_t* __restrict__ seg, unsigned segs, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t wave_total[kWaves];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t* p = seg + (size_t)blockIdx.x * segs;
    uint32_t carry = 0;
    for (unsigned base = 0; base < segs; base += kCloudScanThreads) {
        const unsigned i = base + threadIdx.x;
        const uint32_t v = i < segs ? p[i] : 0u;
        const uint32_t s = wave_scan(v, lane);
        if (lane == 63) wave_total[wv] = s;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (unsigned w = 0; w < (unsigned)kWaves; w++) {
            if (w < wv) before += wave_total[w];
            total += wave_total[w];
        }
        if (i < segs) p[i] = carry + before + (s - v);
        carry += total;
        __syncthreads();                                // wave_total is rewritten by the next pass
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// C3 (ORGANIZED == false) and the organised mode's only kernel: grid (segments of a frame, n), block 256
template <bool NT, bool ORGANIZED>
__global__ __launch_bounds__(kThreads) void cloud_write_kernel(CloudLaunch a)
{
    // per wave 8 KB: first the 6 KB of load_octet's exchange, then the wave's records in output order
    __shared__ float4 buf[kWaves][kWavePixels];
    __shared__ uint32_t wave_count[kWaves];
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned px = (unsigned)a.cam.width * (unsigned)a.cam.height;
    const unsigned seg = blockIdx.x, frame = blockIdx.y;
    const char* sframe = source_frame(a, frame, px);
    const bool vec = (reinterpret_cast<uintptr_t>(sframe) & 15u) == 0;
    const unsigned oct0 = seg * kSegmentOctets + wv * 64u;          // wave-uniform
    float P[24];
    load_octet<NT>(sframe, a.format, vec, oct0, lane, px, a.cam, buf[wv], P);
    const uint8_t* cframe = a.bgr + (a.bgr_frames == 1 ? (size_t)0 : (size_t)frame) * px * 3;
    uint32_t rgb[8];
    load_colour(cframe, (reinterpret_cast<uintptr_t>(cframe) & 7u) == 0, oct0 + lane, px, rgb);
    bool v[8];
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        v[k] = cloud_valid(P[3 * k + 2], a);
        c += v[k] ? 1u : 0u;
    }
    const uint32_t s = wave_scan(c, lane);
    if (lane == 63) wave_count[wv] = s;
    uint4* stage = reinterpret_cast<uint4*>(buf[wv]);
    kde_cloud_point* slot = a.out + (size_t)frame * px;
    if (ORGANIZED) {
#pragma unroll
        for (unsigned k = 0; k < 8; k++) stage[stage_slot(lane * 8 + k)] = cloud_record(&P[3 * k], rgb[k], v[k], a);
        wave_exchange_fence();
        const unsigned first = oct0 * 8;
        const unsigned limit = first < px ? (px - first < kWavePixels ? px - first : kWavePixels) : 0u;
#pragma unroll
        for (unsigned j = 0; j < 8; j++) {
            const unsigned i = j * 64u + lane;
            if (i < limit) store_record(slot + first + i, stage[stage_slot(i)], NT);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
            if (total) atomicAdd(&a.counts[frame], total);          // an integer sum: the same in any order
        }
    } else {
        unsigned r = s - c;                                         // the rank of this lane's first valid pixel in the wave
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            if (v[k]) stage[stage_slot(r++)] = cloud_record(&P[3 * k], rgb[k], true, a);
        }
        __syncthreads();                                            // the counts of the waves before this one; orders the LDS writes too
        uint32_t before = 0;
#pragma unroll
        for (unsigned w = 0; w < (unsigned)kWaves; w++) {
            if (w < wv) before += wave_count[w];
        }
        const uint32_t total = wave_count[wv];                      // <= 512, wave-uniform
        kde_cloud_point* dst = slot + a.seg[(size_t)frame * gridDim.x + seg] + before;
        for (unsigned i = lane; i < total; i += 64u) store_record(dst + i, stage[stage_slot(i)], NT);
    }
}

}  // namespace

// C2 on its own, for another table of per-segment counts (mesh_kernels.hip): offsets in place, the totals of the n frames
int launch_segment_scan(uint32_t* seg, unsigned segs, uint32_t* counts, int n, hipStream_t s)
{
    hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)n), dim3(kCloudScanThreads), 0, s, seg, segs, counts);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

int launch_cloud(const CloudLaunch& a, hipStream_t s)
{
    const size_t px = (size_t)a.cam.width * a.cam.height;
    const unsigned segs = cloud_segments(px);
    const size_t esz = a.format == KDE_SRC_POINTS_F32 ? sizeof(kde_float3) : a.format == KDE_SRC_DEPTH_F32 ? sizeof(float) : sizeof(uint16_t);
    const size_t bytes = px * a.n * (esz + sizeof(kde_cloud_point)) + px * a.bgr_frames * 3;
    const bool nt = past_cache(kSiteCloud, bytes);
    const dim3 grid(segs, (unsigned)a.n), block(kThreads);
    if (a.organized) {
        KDE_HIP_TRY(hipMemsetAsync(a.counts, 0, (size_t)a.n * sizeof(uint32_t), s));
        if (nt) hipLaunchKernelGGL((cloud_write_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cloud_write_kernel<false, true>), grid, block, 0, s, a);
    } else {
        if (nt) hipLaunchKernelGGL(cloud_count_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(cloud_count_kernel<false>, grid, block, 0, s, a);
        hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)a.n), dim3(kCloudScanThreads), 0, s, a.seg, segs, a.counts);
        if (nt) hipLaunchKernelGGL((cloud_write_kernel<true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((cloud_write_kernel<false, false>), grid, block, 0, s, a);
    }
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
