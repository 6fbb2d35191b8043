// upsample_kernels.hip — GuidedDepthUpsampling: joint bilateral upsampling (Kopf et al. 2007) of a low-resolution depth frame
// to the size of its colour image, for n frames on the device.  The reference has no such step (its class of a similar name,
// SPDepthSuperResolution, fits planes at one size); every class here takes depth and colour of one size, which this produces.
//   G1 upsample  a workgroup of 256 threads takes four consecutive tiles of 32 x 8 output pixels, a thread one pixel of each.
//                Per tile it stages in LDS the taps any of its pixels reads: their depth as a float, 0 where the tap lies
//                outside the source or is invalid (a valid depth is > z_min >= 0, so 0 means absent), and the guide colour at
//                (gx_of[qx], gy_of[qy]) packed as b | g << 8 | r << 16, gathered in the same loop.  The 766 weights of the
//                range table are staged once per workgroup.  A pixel reads its own guide colour once, forms k with one
//                v_sad_u8 per tap and looks the weight up: no transcendental at run time.
//                With the guard (max_gap > 0) the arg-max comes first: for r <= 2 the (2r)^2 weights stay in registers, for
//                r >= 3 they are computed again in the second loop, and only the taps of one row are unrolled: with every row
//                unrolled the compiler reported 99 .. 177 registers for r = 3 and 4, with one row 44 .. 57, as many as r = 2
//                takes (55 / 57), eight waves per SIMD in every instance.
//                A tile's rows go through LDS and leave as 16-byte (float) or 8-byte (uint16) stores where the output frame
//                starts on such a boundary and its width is a multiple of four; as elements, with the same bytes, elsewhere.
//                The pixels that got a depth are counted per workgroup and written, not added, to partial[frame][workgroup].
//   G2 count     filled[f] = the sum of partial[f][*], one workgroup per frame: no atomic, no reset, and every call writes
//                every count it reports (kernel nodes keep their order in a replayed graph; a memset node did not: R0 of
//                reg_kernels.hip)
// The tap window of a tile.  x0(i) = floorf(((float)i + 0.5f) * sx - 0.5f) does not decrease with i (every rounding is
// monotone), so the taps of a tile's pixels span the columns x0(i_first) - r + 1 .. x0(i_last) + r: x0(i_last) - x0(i_first) +
// 2r of them.  With sx <= 1 (out_w >= src_w, and a correctly rounded quotient of a <= b is <= 1) the exact difference of u over
// 31 pixels is at most 31, each of the three roundings of either u moves it by at most half an ulp <= 0.5 (u < 2^24), so the
// floors differ by at most 34 and the window holds at most 34 + 2r <= 42 columns; 7 + 3 + 2r <= 18 rows likewise.  The LDS
// arrays hold 44 x 20; kde_upsample_create evaluates every tile's window with these operations and refuses an object whose
// window would not fit, and the kernel clamps the number of taps it stages to the arrays.
// The rule is stated in kde_hip.h.  Every output pixel is a function of the source frame, the guide and its own coordinates,
// and the count an integer sum: the same bytes for any n, place in the batch and alignment.
#include "kde_internal.h"
#include "kde_device_math.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileW = kUpsampleTileW, kTileH = kUpsampleTileH;
constexpr int kWinW = kUpsampleWinW, kWinH = kUpsampleWinH;
static_assert(kTileW * kTileH == kThreads && kTileW == 32, "a thread per pixel of a tile, a tile row per half wave");

typedef unsigned u_v2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float tent(int q, float u, float r) { return fmaxf(1.0f - fabsf((float)q - u) / r, 0.0f); }

// G1: grid (groups of kUpsampleTilesPerGroup tiles, n), block 256
template <int R, bool GUARD>
__global__ __launch_bounds__(kThreads) void upsample_kernel(UpsampleLaunch L)
{
    constexpr int T = 2 * R;
    constexpr bool KEEP = R <= 2;                           // the weights of the arg-max loop stay in registers
    constexpr int ROWS = R <= 2 ? T : 1;                    // tap rows unrolled: all of them kept 99 .. 177 registers live for r >= 3
    __shared__ float s_range[768];
    __shared__ float s_z[kWinH * kWinW];
    __shared__ uint32_t s_c[kWinH * kWinW];
    __shared__ __attribute__((aligned(16))) float s_out[kThreads];
    __shared__ uint32_t s_count[kWaves];
    const int tid = (int)threadIdx.x, lx = tid & (kTileW - 1), ly = tid >> 5;
    const unsigned frame = blockIdx.y;
    const size_t opx = (size_t)L.ow * L.oh, spx = (size_t)L.sw * L.sh;
    const bool in_f32 = L.depth_format == KDE_DEPTH_F32, out_f32 = L.out_format == KDE_DEPTH_F32;
    const char* sframe = static_cast<const char*>(L.depth) + (size_t)frame * spx * (in_f32 ? sizeof(float) : sizeof(uint16_t));
    const uint8_t* gframe = L.bgr + (L.bgr_frames == 1 ? (size_t)0 : (size_t)frame) * opx * 3;
    char* oframe = static_cast<char*>(L.out) + (size_t)frame * opx * (out_f32 ? sizeof(float) : sizeof(uint16_t));
    const bool vec = (L.ow & 3) == 0 && (reinterpret_cast<uintptr_t>(oframe) & (out_f32 ? 15u : 7u)) == 0;
    for (int k = tid; k < kColourRange; k += kThreads) s_range[k] = L.range[k];
    const int tiles_x = (L.ow + kTileW - 1) / kTileW, tiles_y = (L.oh + kTileH - 1) / kTileH;
    const int ntiles = tiles_x * tiles_y;
    uint32_t count = 0;
    for (int t = 0; t < kUpsampleTilesPerGroup; t++) {
        const int tile = (int)blockIdx.x * kUpsampleTilesPerGroup + t;
        if (tile >= ntiles) break;                          // the same for every thread
        const int trow = tile / tiles_x, tcol = tile - trow * tiles_x;
        const int i0 = tcol * kTileW, j0 = trow * kTileH;
        const int i1 = min(i0 + kTileW - 1, L.ow - 1), j1 = min(j0 + kTileH - 1, L.oh - 1);
        const int xf = upsample_floor(i0, L.sx), yf = upsample_floor(j0, L.sy);
        const int wx0 = xf - R + 1, wy0 = yf - R + 1;
        const int tw = min(upsample_floor(i1, L.sx) - xf + T, kWinW), th = min(upsample_floor(j1, L.sy) - yf + T, kWinH);
        __syncthreads();                                    // the tile before this one has been read
        for (int idx = tid; idx < tw * th; idx += kThreads) {
            const int wy = idx / tw, wx = idx - wy * tw;
            const int qx = wx0 + wx, qy = wy0 + wy;
            float z = 0.0f;
            uint32_t c = 0u;
            if ((unsigned)qx < (unsigned)L.sw && (unsigned)qy < (unsigned)L.sh) {
                const size_t at = (size_t)qy * (unsigned)L.sw + (unsigned)qx;
                const float zz = load_depth(sframe, in_f32, at);
                if (zz > L.z_min && zz < L.z_max) {         // a NaN fails; an absent tap needs no colour
                    z = zz;
                    c = pack_bgr(gframe + ((size_t)L.gy_of[qy] * (unsigned)L.ow + (unsigned)L.gx_of[qx]) * 3);
                }
            }
            s_z[wy * kWinW + wx] = z;
            s_c[wy * kWinW + wx] = c;
        }
        __syncthreads();
        const int i = i0 + lx, j = j0 + ly;
        const bool active = i < L.ow && j < L.oh;
        float result = 0.0f;
        if (active) {
            const float u = ((float)i + 0.5f) * L.sx - 0.5f, v = ((float)j + 0.5f) * L.sy - 0.5f;
            const int x0 = (int)floorf(u), y0 = (int)floorf(v);
            float wxs[T];
#pragma unroll
            for (int a = 0; a < T; a++) wxs[a] = tent(x0 - R + 1 + a, u, (float)R);
            const uint32_t own = pack_bgr(gframe + ((size_t)j * (unsigned)L.ow + (unsigned)i) * 3);
            const int base = (y0 - yf) * kWinW + (x0 - xf);
            const float* zt = s_z + base;
            const uint32_t* ct = s_c + base;
            // the weight of tap (a, b) of this pixel, wy the tent of its row: 0 for an absent tap
            auto weight = [&](int a, int b, float wy, float z) {
                const float w = (wxs[a] * wy) * s_range[__builtin_amdgcn_sad_u8(own, ct[b * kWinW + a], 0u)];
                return z != 0.0f ? w : 0.0f;
            };
            float num = 0.0f, den = 0.0f;
            if (GUARD) {
                float kept[KEEP ? T * T : 1];
                float best = 0.0f, zref = 0.0f;
#pragma unroll ROWS
                for (int b = 0; b < T; b++) {
                    const float wy = tent(y0 - R + 1 + b, v, (float)R);
#pragma unroll
                    for (int a = 0; a < T; a++) {
                        const float z = zt[b * kWinW + a];
                        const float w = weight(a, b, wy, z);
                        if (KEEP) kept[b * T + a] = w;
                        if (w > best) {                     // the first of equal weights stays
                            best = w;
                            zref = z;
                        }
                    }
                }
#pragma unroll ROWS
                for (int b = 0; b < T; b++) {
                    const float wy = tent(y0 - R + 1 + b, v, (float)R);
#pragma unroll
                    for (int a = 0; a < T; a++) {
                        const float z = zt[b * kWinW + a];
                        float w = KEEP ? kept[b * T + a] : weight(a, b, wy, z);
                        if (fabsf(z - zref) > L.max_gap) w = 0.0f;
                        num = num + w * z;                  // a weight of 0 adds +0 to both: the sums of the remaining taps
                        den = den + w;
                    }
                }
            } else {
#pragma unroll ROWS
                for (int b = 0; b < T; b++) {
                    const float wy = tent(y0 - R + 1 + b, v, (float)R);
#pragma unroll
                    for (int a = 0; a < T; a++) {
                        const float z = zt[b * kWinW + a];
                        const float w = weight(a, b, wy, z);
                        num = num + w * z;
                        den = den + w;
                    }
                }
            }
            if (den > 0.0f) {                               // some tap remains: every remaining weight is > 0
                result = num / den;
                count++;
            }
        }
        if (vec) {                                          // the same for every thread
            s_out[tid] = result;
            __syncthreads();
            const int row = tid >> 3, seg = (tid & 7) * 4;
            if (tid < kTileH * (kTileW / 4) && j0 + row < L.oh && i0 + seg < L.ow) {    // ow % 4 == 0: the four pixels are inside
                const float4 q = *reinterpret_cast<const float4*>(&s_out[row * kTileW + seg]);
                const size_t at = (size_t)(j0 + row) * (unsigned)L.ow + (unsigned)(i0 + seg);
                if (out_f32) {
                    *reinterpret_cast<float4*>(oframe + at * sizeof(float)) = q;
                } else {
                    const u_v2 d = {(uint32_t)depth_to_u16(q.x) | ((uint32_t)depth_to_u16(q.y) << 16),
                                    (uint32_t)depth_to_u16(q.z) | ((uint32_t)depth_to_u16(q.w) << 16)};
                    *reinterpret_cast<u_v2*>(oframe + at * sizeof(uint16_t)) = d;
                }
            }
        } else if (active) {
            store_depth(oframe, out_f32, (size_t)j * (unsigned)L.ow + (unsigned)i, result);
        }
    }
    block_partials_u32(count, s_count);
    if (tid == 0) L.partial[(size_t)frame * gridDim.x + blockIdx.x] = block_sum_u32(s_count);
}

// G2: grid n, block 256
__global__ __launch_bounds__(kThreads) void upsample_count_kernel(const uint32_t* __restrict__ partial, unsigned groups,
                                                                  uint32_t* __restrict__ filled)
{
    __shared__ uint32_t s_count[kWaves];
    const uint32_t* p = partial + (size_t)blockIdx.x * groups;
    uint32_t count = 0;
    for (unsigned g = threadIdx.x; g < groups; g += kThreads) count += p[g];
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) count += (uint32_t)__shfl_xor((int)count, (int)off, 64);
    if ((threadIdx.x & 63u) == 0) s_count[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) filled[blockIdx.x] = (s_count[0] + s_count[1]) + (s_count[2] + s_count[3]);
}

template <int R>
void launch_r(const UpsampleLaunch& a, dim3 grid, hipStream_t s)
{
    if (a.max_gap > 0.0f) hipLaunchKernelGGL((upsample_kernel<R, true>), grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((upsample_kernel<R, false>), grid, dim3(kThreads), 0, s, a);
}

}  // namespace

unsigned upsample_groups(int ow, int oh)
{
    const long long tiles = (long long)((ow + kTileW - 1) / kTileW) * ((oh + kTileH - 1) / kTileH);
    return (unsigned)((tiles + kUpsampleTilesPerGroup - 1) / kUpsampleTilesPerGroup);
}

int launch_upsample(const UpsampleLaunch& a, hipStream_t s)
{
    const unsigned groups = upsample_groups(a.ow, a.oh);
    const dim3 grid(groups, (unsigned)a.n);
    switch (a.radius) {
    case 1: launch_r<1>(a, grid, s); break;
    case 2: launch_r<2>(a, grid, s); break;
    case 3: launch_r<3>(a, grid, s); break;
    case 4: launch_r<4>(a, grid, s); break;
    default: return fail(KDE_ERR_INVALID, "launch_upsample: radius %d", a.radius);
    }
    hipLaunchKernelGGL(upsample_count_kernel, dim3((unsigned)a.n), dim3(kThreads), 0, s, a.partial, groups, a.filled);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
