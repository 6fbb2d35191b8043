// holefill_kernels.hip — DepthHoleFilling: the holes of a depth frame filled from their valid neighbours, weighted by distance
// and by the resemblance of the guide colour, front by front: N passes, each of which reaches r pixels further into a hole.
// For n frames on the device.  No reference counterpart.  The rule is stated in kde_hip.h.
//   H1 fill   a workgroup of 256 threads owns one tile of 32 x 16 pixels, a thread the pixels (lx, ly) and (lx, ly + 8).  One
//             launch performs k <= 4 passes in LDS, so that N passes cost ceil(N / k) trips through HBM instead of N:
//             - The threads read their own pixels (the first launch sanitises the caller's depth, a later one reads the state
//               the launch before it wrote) and the waves ballot "one of mine is a hole".  A tile without a hole does no pass:
//               it moves its bytes (converted by the last launch) and is done -- no halo, no guide, no table.  How many
//               tiles of a sensor's frame that is has not been measured; with 1 % salt it is none of the first launch's.
//             - Otherwise the tile and a halo of k * r pixels are staged: the depth as a float with 0 for a hole or a cell
//               outside the frame, the guide as b | g << 8 | r << 16 | 1 << 24, so that k of the rule is one v_sad_u8 (bit
//               24 is set in every cell inside the frame, so it adds nothing between two of them, and a cell outside the
//               frame, whose word is 0, is never filled).
//             - Pass j = 1 .. k reads one LDS copy of the state and writes the other (a snapshot: no pixel of pass j sees
//               another pixel of pass j), for the cells within (k - j) * r of the tile.  Bounds: a cell of that region reads
//               taps within r of it, which lie within (k - j + 1) * r of the tile -- the region pass j - 1 wrote, or for j = 1
//               the staged halo k * r.  By induction every cell of the region of pass j holds what the whole-frame pass would
//               give it, and after pass k that region is the tile.  Cells outside the region of a pass go stale in the copy it
//               writes and are never read again, since the regions only shrink.
//             - The passes of a launch stop early once a pass leaves no hole in its region or fills none: the passes after it
//               would read an unchanged snapshot on smaller regions and fill nothing.  A tile that only has salt does one pass
//               (and one that finds nothing to do); the inside of a hole too wide to close does one that fills nothing.
//             - Only hole cells walk their taps; a valid cell is copied.  With the guard the taps are walked twice (zref, then
//               the sums), the weights computed again rather than kept: they are two LDS reads and a multiplication.
//             - pass_of of the tile's pixels sits in LDS during the launch and in the caller's (or the object's) array between
//               launches, in place: a pixel's entry is read and written by the workgroup that owns it and by no other.
//             - The last launch converts to the output format and counts, per workgroup, the pixels with 1 <= pass_of <= N and
//               those still 0, written (not added) to partial[frame][workgroup][2].
//   H2 count  filled[f], remaining[f] = the sums of partial[f][*], one workgroup per frame: no atomic, no reset, and every
//             call writes every count it reports (kernel nodes keep their order in a replayed graph; a memset node did not: R0
//             of reg_kernels.hip)
// Every pixel of every pass is a function of the snapshot before it, the guide and the tables, and the counts are integer
// sums: the same bytes for any n, place in the batch, pointer alignment and k.
#include "kde_internal.h"
#include "kde_device_math.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTileW = kHolefillTileW, kTileH = kHolefillTileH;
constexpr int kPerThread = kTileW * kTileH / kThreads;
static_assert(kTileW == 32 && kPerThread == 2, "a tile row per half wave, two pixels per thread");

// The new depth of the hole cell at zc / cc (its own cell of the snapshot and of the colour words, PW cells per row), or 0
// where the rule leaves it a hole.  GUARD 0: off, 1: zref is the heaviest tap, 2: the farthest.
template <int R, int PW, int GUARD>
__device__ __forceinline__ float fill_cell(const float* zc, const uint32_t* cc, const float* s_space, const float* s_range, int min_taps,
                                           float max_gap)
{
    constexpr int D = 2 * R + 1;
    const uint32_t own = cc[0];
    // the centre is a hole, so it is absent like any other: the loops need not skip it
    auto weight = [&](int dy, int dx) { return s_space[(dy + R) * D + dx + R] * s_range[__builtin_amdgcn_sad_u8(own, cc[dy * PW + dx], 0u)]; };
    int support = 0;
    float num = 0.0f, den = 0.0f;
    if (GUARD) {
        float best = 0.0f, zref = 0.0f;
#pragma unroll 1
        for (int dy = -R; dy <= R; dy++) {
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const float z = zc[dy * PW + dx];
                const float w = weight(dy, dx);
                const bool present = z != 0.0f && w > 0.0f;
                support += present;
                if (GUARD == 1) {
                    if (present && w > best) {              // the first of equal weights stays
                        best = w;
                        zref = z;
                    }
                } else if (present && z > zref) {
                    zref = z;
                }
            }
        }
        if (support < min_taps) return 0.0f;
#pragma unroll 1
        for (int dy = -R; dy <= R; dy++) {
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const float z = zc[dy * PW + dx];
                const float w = weight(dy, dx);
                if (z != 0.0f && w > 0.0f && !(fabsf(z - zref) > max_gap)) {
                    num = num + w * z;
                    den = den + w;
                }
            }
        }
    } else {
#pragma unroll 1
        for (int dy = -R; dy <= R; dy++) {
#pragma unroll
            for (int dx = -R; dx <= R; dx++) {
                const float z = zc[dy * PW + dx];
                const float w = weight(dy, dx);
                if (z != 0.0f && w > 0.0f) {
                    support++;
                    num = num + w * z;
                    den = den + w;
                }
            }
        }
        if (support < min_taps) return 0.0f;
    }
    const float v = num / den;                              // support >= 1: den > 0
    return v > 0.0f ? v : 0.0f;
}

// H1: grid (tiles of a frame, n), block 256
template <int R, int GUARD>
__global__ __launch_bounds__(kThreads) void holefill_kernel(HolefillLaunch L)
{
    constexpr int D = 2 * R + 1;
    constexpr int PW = kTileW + 2 * kHolefillMaxFuse * R, PH = kTileH + 2 * kHolefillMaxFuse * R;
    __shared__ float s_range[768];
    __shared__ float s_space[D * D];
    __shared__ float s_z[2][PW * PH];
    __shared__ uint32_t s_c[PW * PH];
    __shared__ uint8_t s_pass[kTileW * kTileH];
    __shared__ uint32_t s_count[2][kWaves];
    __shared__ uint32_t s_any[kWaves];
    const int tid = (int)threadIdx.x, lx = tid & (kTileW - 1), ly = tid >> 5;
    const unsigned frame = blockIdx.y;
    const int tiles_x = (L.w + kTileW - 1) / kTileW;
    const int trow = (int)blockIdx.x / tiles_x, tcol = (int)blockIdx.x - trow * tiles_x;
    const int x0 = tcol * kTileW, y0 = trow * kTileH;
    const size_t px = (size_t)L.w * L.h;
    const bool in_f32 = L.src_format == KDE_DEPTH_F32, out_f32 = L.dst_format == KDE_DEPTH_F32;
    const char* sframe = static_cast<const char*>(L.src) + (size_t)frame * px * (in_f32 ? sizeof(float) : sizeof(uint16_t));
    char* dframe = static_cast<char*>(L.dst) + (size_t)frame * px * (out_f32 ? sizeof(float) : sizeof(uint16_t));
    uint8_t* pframe = L.pass + (size_t)frame * px;
    // the state of pass p0 at a pixel of the frame: pass 0 of the rule in the first launch, the stored state later
    auto state_at = [&](size_t at) {
        const float d = load_depth(sframe, in_f32, at);
        if (!L.first) return d;
        return (d > L.z_min && d < L.z_max) ? d : 0.0f;     // a NaN fails
    };
    auto store = [&](size_t at, float z) { store_depth(dframe, out_f32, at, z); };

    float mine[kPerThread];
    bool inside[kPerThread];
    bool hole = false;
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        const int x = x0 + lx, y = y0 + ly + q * (kTileH / kPerThread);
        inside[q] = x < L.w && y < L.h;
        mine[q] = inside[q] ? state_at((size_t)y * (unsigned)L.w + (unsigned)x) : 1.0f;
        hole |= mine[q] == 0.0f;
    }
    const bool wave_hole = __ballot(hole) != 0ull;         // every lane votes: outside the branch below
    if ((tid & 63) == 0) s_any[tid >> 6] = wave_hole;
    __syncthreads();
    const bool any = ((s_any[0] | s_any[1]) | (s_any[2] | s_any[3])) != 0u;     // the same for every thread

    uint32_t filled = 0, remaining = 0;
    if (!any) {
#pragma unroll
        for (int q = 0; q < kPerThread; q++) {
            if (!inside[q]) continue;
            const size_t at = (size_t)(y0 + ly + q * (kTileH / kPerThread)) * (unsigned)L.w + (unsigned)(x0 + lx);
            store(at, mine[q]);
            if (L.first) pframe[at] = 0;
            else if (L.last) filled += pframe[at] != 0;     // no hole here: not 255
        }
    } else {
        const int halo = L.passes * R;                      // <= kHolefillMaxFuse * R
        const int sw = kTileW + 2 * halo, sh = kTileH + 2 * halo;
        const uint8_t* gframe = L.bgr + (L.bgr_frames == 1 ? (size_t)0 : (size_t)frame) * px * 3;
        // k of two cells of the frame is at most 765; against a cell outside the frame (word 0, bit 24 clear) the SAD reaches 766:
        // that tap is absent by its depth of 0, and the entries behind the table are 0 so that its weight is one too
        for (int k = tid; k < 768; k += kThreads) s_range[k] = k < kColourRange ? L.range[k] : 0.0f;
        if (tid < D * D) s_space[tid] = L.space[tid];
        for (int idx = tid; idx < sw * sh; idx += kThreads) {
            const int cy = idx / sw, cx = idx - cy * sw;
            const int x = x0 - halo + cx, y = y0 - halo + cy;
            float z = 0.0f;
            uint32_t c = 0u;
            if ((unsigned)x < (unsigned)L.w && (unsigned)y < (unsigned)L.h) {
                const size_t at = (size_t)y * (unsigned)L.w + (unsigned)x;
                z = state_at(at);
                c = pack_bgr(gframe + at * 3) | (1u << 24);
            }
            s_z[0][cy * PW + cx] = z;
            s_c[cy * PW + cx] = c;
        }
#pragma unroll
        for (int q = 0; q < kPerThread; q++) {
            const int row = ly + q * (kTileH / kPerThread);
            uint8_t p = 0;
            if (inside[q]) p = L.first ? (mine[q] == 0.0f ? (uint8_t)255 : (uint8_t)0) : pframe[(size_t)(y0 + row) * (unsigned)L.w + (unsigned)(x0 + lx)];
            s_pass[row * kTileW + lx] = p;
        }
        __syncthreads();
        int cur = 0;
        for (int j = 1; j <= L.passes; j++) {
            const int off = j * R;                          // the region of pass j starts this far inside the staged window
            const int rw = sw - 2 * off, rh = sh - 2 * off;
            const float* zin = s_z[cur];
            float* zout = s_z[cur ^ 1];
            bool gave = false, left = false;                // this thread filled a cell / saw a hole it could not fill
            for (int idx = tid; idx < rw * rh; idx += kThreads) {
                const int ry = idx / rw, rx = idx - ry * rw;
                const int cy = off + ry, cx = off + rx;
                const int cell = cy * PW + cx;
                float z = zin[cell];
                if (z == 0.0f && (s_c[cell] >> 24) != 0u) {
                    z = fill_cell<R, PW, GUARD>(zin + cell, s_c + cell, s_space, s_range, L.min_taps, L.max_gap);
                    const int tx = cx - halo, ty = cy - halo;
                    if (z != 0.0f && (unsigned)tx < (unsigned)kTileW && (unsigned)ty < (unsigned)kTileH) s_pass[ty * kTileW + tx] = (uint8_t)(L.p0 + j);
                    gave |= z != 0.0f;
                    left |= z == 0.0f;
                }
                zout[cell] = z;
            }
            // both are barriers; the region of pass j holds the tile, so the copy just written is a whole result
            const bool any_gave = __syncthreads_or(gave) != 0, any_left = __syncthreads_or(left) != 0;
            cur ^= 1;
            // No hole left in the region, or a pass that filled none of them: the passes that follow work on smaller regions
            // of an unchanged snapshot and fill nothing either.  Salt is gone after one pass, the inside of a wide hole never
            // starts.
            if (!any_gave || !any_left) break;              // the same for every thread
        }
#pragma unroll
        for (int q = 0; q < kPerThread; q++) {
            if (!inside[q]) continue;
            const int row = ly + q * (kTileH / kPerThread);
            const size_t at = (size_t)(y0 + row) * (unsigned)L.w + (unsigned)(x0 + lx);
            const float z = s_z[cur][(halo + row) * PW + halo + lx];
            const uint8_t p = s_pass[row * kTileW + lx];
            store(at, z);
            pframe[at] = p;
            filled += p != 0 && p != 255;
            remaining += z == 0.0f;
        }
    }
    if (!L.last) return;                                    // the same for every thread
#pragma unroll
    for (unsigned o = 32; o >= 1; o >>= 1) {
        filled += (uint32_t)__shfl_xor((int)filled, (int)o, 64);
        remaining += (uint32_t)__shfl_xor((int)remaining, (int)o, 64);
    }
    if ((tid & 63) == 0) {
        s_count[0][tid >> 6] = filled;
        s_count[1][tid >> 6] = remaining;
    }
    __syncthreads();
    if (tid < 2) L.partial[((size_t)frame * gridDim.x + blockIdx.x) * 2 + tid] = block_sum_u32(s_count[tid]);
}

// H2: grid n, block 256
__global__ __launch_bounds__(kThreads) void holefill_count_kernel(const uint32_t* __restrict__ partial, unsigned groups,
                                                                  uint32_t* __restrict__ filled, uint32_t* __restrict__ remaining)
{
    __shared__ uint32_t s_count[2][kWaves];
    const uint32_t* p = partial + (size_t)blockIdx.x * groups * 2;
    uint32_t a = 0, b = 0;
    for (unsigned g = threadIdx.x; g < groups; g += kThreads) {
        a += p[2 * g];
        b += p[2 * g + 1];
    }
#pragma unroll
    for (unsigned o = 32; o >= 1; o >>= 1) {
        a += (uint32_t)__shfl_xor((int)a, (int)o, 64);
        b += (uint32_t)__shfl_xor((int)b, (int)o, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        s_count[0][threadIdx.x >> 6] = a;
        s_count[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        filled[blockIdx.x] = (s_count[0][0] + s_count[0][1]) + (s_count[0][2] + s_count[0][3]);
        remaining[blockIdx.x] = (s_count[1][0] + s_count[1][1]) + (s_count[1][2] + s_count[1][3]);
    }
}

template <int R>
void launch_r(const HolefillLaunch& a, dim3 grid, hipStream_t s)
{
    if (!(a.max_gap > 0.0f)) hipLaunchKernelGGL((holefill_kernel<R, 0>), grid, dim3(kThreads), 0, s, a);
    else if (a.gap_rule == 0) hipLaunchKernelGGL((holefill_kernel<R, 1>), grid, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((holefill_kernel<R, 2>), grid, dim3(kThreads), 0, s, a);
}

}  // namespace

unsigned holefill_groups(int w, int h)
{
    return (unsigned)((long long)((w + kTileW - 1) / kTileW) * ((h + kTileH - 1) / kTileH));
}

int launch_holefill(const HolefillLaunch& call, hipStream_t s)
{
    if (call.radius < 1 || call.radius > kHolefillMaxRadius || call.fuse < 1 || call.fuse > kHolefillMaxFuse || call.iterations < 1)
        return fail(KDE_ERR_INVALID, "launch_holefill: radius %d, %d passes per launch, %d iterations", call.radius, call.fuse, call.iterations);
    HolefillLaunch a = call;
    const unsigned groups = holefill_groups(a.w, a.h);
    const dim3 grid(groups, (unsigned)a.n);
    const int launches = (a.iterations + a.fuse - 1) / a.fuse;
    a.src = call.depth;
    a.src_format = call.depth_format;
    for (int i = 0; i < launches; i++) {
        a.first = i == 0;
        a.last = i == launches - 1;
        a.p0 = i * a.fuse;
        a.passes = a.last ? a.iterations - a.p0 : a.fuse;
        a.dst = a.last ? call.out : static_cast<void*>(call.state[i & 1]);
        a.dst_format = a.last ? call.out_format : KDE_DEPTH_F32;
        switch (a.radius) {
        case 1: launch_r<1>(a, grid, s); break;
        case 2: launch_r<2>(a, grid, s); break;
        default: launch_r<3>(a, grid, s); break;
        }
        a.src = a.dst;
        a.src_format = KDE_DEPTH_F32;
    }
    hipLaunchKernelGGL(holefill_count_kernel, dim3((unsigned)a.n), dim3(kThreads), 0, s, a.partial, groups, a.filled, a.remaining);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
