// speckle_kernels.hip — DepthSpeckleFilter: the connected components of a depth frame under a depth-difference link, and the
// frame without the components smaller than min_size (flying pixels, speckles).  For n frames on the device.  No reference
// counterpart.  The rule is stated in kde_hip.h; the union-find is kde_union.h, which host code runs too.
//   S1 tile     a workgroup of 256 threads owns one tile of 32 x 16 pixels, a thread the pixels (lx, ly) and (lx, ly + 8).  It
//               stages the sanitised depth of the tile in LDS, computes each pixel's link bits towards its right, lower and (8)
//               two lower diagonal neighbours INSIDE the tile once, and labels the tile in LDS: one uf_union per link on a
//               table of 512 local indices with LDS atomic-min.  Local index order is raster order, so a local root is the
//               pixel of its local component with the smallest raster index.  It writes parent[p] = the raster index of p's
//               local root (-1 for an invalid pixel) and size[root] = the pixels of the local component.
//               Short paths: a tile without a valid pixel writes -1 and is done; a tile whose pixels are all valid and all
//               linked to their right and lower neighbours is one component by construction -- no union.
//               Block 0 of a frame zeroes capped[f]: no other block of this launch touches it, the later launches add to it.
//   S2 seam     one thread per pixel of the first column (x = 32 k) or first row (y = 16 k) of a tile, k >= 1.  A column pixel
//               looks at (x - 1, y) and, for 8, (x - 1, y - 1) and (x - 1, y + 1); a row pixel at (x, y - 1) and, for 8,
//               (x - 1, y - 1) and (x + 1, y - 1).  Two neighbours in different tiles differ in their tile column -- then one of
//               them is a column pixel and the other one of its three -- or only in their tile row -- then one is a row pixel and
//               the other one of its three: every pair across a seam or a corner is met (some twice: a union is idempotent).
//               Linked pairs are united in parent[] with global atomic-min (agent scope); the walks load with agent scope so
//               that they are rarely stale, and nothing rests on that (kde_union.h).
//   S3 resolve  one thread per pixel; a local root (S1 wrote size[p] != 0 there and 0 at every other valid pixel) that S2 gave a
//               parent adds its local size to its global root's: one atomic per local component.  parent[p] becomes the global
//               root (a plain store: a walk of another thread through p sees the old or the new value, both of which lead to
//               that root).  Skipped, with S2, for a frame of one tile.
//   S4 apply    per pixel: root, size, output, label; per workgroup the number removed and the kept roots, written (not added)
//               to partial[f][workgroup][0..1].  Reads its own pixel of the input before it writes it: in place is safe.
//   S5 count    removed[f], components[f] = sums of partial[f][*]; capped[f] += the tiles' caps (partial[f][*][2]).
// No workgroup waits for another: no cooperative launch, no flag, no spin.  Within a launch correctness rests on the values
// atomics return; between launches on the launch boundary.  Every loop strictly descends and has the hard cap kUnionCap.
// The labels are component minima and the sums are integer sums: the same bytes for any n, place in the batch, pointer
// alignment, tile shape and order of the atomics.
#include "kde_internal.h"
#include "kde_device_math.h"
#include "kde_union.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kTileW = kSpeckleTileW, kTileH = kSpeckleTileH;
constexpr int kCells = kTileW * kTileH;
constexpr int kPerThread = kCells / kThreads;
static_assert(kTileW == 32 && kPerThread == 2, "a tile row per half wave, two pixels per thread");

struct LdsOps {
    int* cell;
    __device__ int load(int i) const { return __hip_atomic_load(cell + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ int amin(int i, int v) const { return atomicMin(cell + i, v); }
};

struct GlobalOps {
    int32_t* cell;                                          // parent[] of one frame
    __device__ int load(int i) const { return __hip_atomic_load(cell + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ int amin(int i, int v) const { return atomicMin(cell + i, v); }
};

struct Frame {
    const char* src;
    bool f32;
    float z_min, z_max;
    __device__ float state(size_t at) const
    {
        const float d = load_depth(src, f32, at);
        return (d > z_min && d < z_max) ? d : 0.0f;         // a NaN fails
    }
};

__device__ __forceinline__ Frame frame_of(const SpeckleLaunch& L, unsigned frame)
{
    const bool f32 = L.depth_format == KDE_DEPTH_F32;
    const size_t px = (size_t)L.w * L.h;
    return Frame{static_cast<const char*>(L.depth) + (size_t)frame * px * (f32 ? sizeof(float) : sizeof(uint16_t)), f32, L.z_min, L.z_max};
}

// S1: grid (tiles of a frame, n), block 256
template <bool CONN8>
__global__ __launch_bounds__(kThreads) void speckle_tile_kernel(SpeckleLaunch L)
{
    __shared__ float s_z[kCells];
    __shared__ int s_lab[kCells];
    __shared__ uint32_t s_size[kCells];
    __shared__ uint32_t s_part[4];
    const int tid = (int)threadIdx.x, lx = tid & (kTileW - 1), ly = tid >> 5;
    const unsigned frame = blockIdx.y;
    const int tiles_x = (L.w + kTileW - 1) / kTileW;
    const int trow = (int)blockIdx.x / tiles_x, tcol = (int)blockIdx.x - trow * tiles_x;
    const int x0 = tcol * kTileW, y0 = trow * kTileH;
    const size_t px = (size_t)L.w * L.h;
    const Frame F = frame_of(L, frame);
    int32_t* parent = L.parent + (size_t)frame * px;
    uint32_t* size = L.size + (size_t)frame * px;
    uint32_t* part = L.partial + ((size_t)frame * gridDim.x + blockIdx.x) * 3;
    if (blockIdx.x == 0 && tid == 0) L.capped[frame] = 0;

    float z[kPerThread];
    bool inside[kPerThread];
    bool any = false;
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        const int row = ly + q * (kTileH / kPerThread), cell = row * kTileW + lx;
        const int x = x0 + lx, y = y0 + row;
        inside[q] = x < L.w && y < L.h;
        z[q] = inside[q] ? F.state((size_t)y * (unsigned)L.w + (unsigned)x) : 0.0f;
        any |= z[q] > 0.0f;
        s_z[cell] = z[q];
        s_lab[cell] = cell;
        s_size[cell] = 0;
    }
    if (!__syncthreads_or(any)) {                           // a barrier; the same for every thread
#pragma unroll
        for (int q = 0; q < kPerThread; q++)
            if (inside[q]) parent[(size_t)(y0 + ly + q * (kTileH / kPerThread)) * (unsigned)L.w + (unsigned)(x0 + lx)] = -1;
        if (tid == 0) part[2] = 0;
        return;
    }

    // link bits towards the neighbours inside the tile: 1 right, 2 down, 4 down-right, 8 down-left.  A cell outside the frame
    // holds 0 and links to nothing.
    unsigned bits[kPerThread];
    bool full = true;                                       // every pixel of mine valid and linked to what lies right of and below it
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        const int row = ly + q * (kTileH / kPerThread), cell = row * kTileW + lx;
        const bool has_r = lx + 1 < kTileW, has_d = row + 1 < kTileH;
        unsigned b = 0;
        if (has_r && linked(z[q], s_z[cell + 1], L.max_diff, L.rel_diff)) b |= 1u;
        if (has_d && linked(z[q], s_z[cell + kTileW], L.max_diff, L.rel_diff)) b |= 2u;
        if (CONN8) {
            if (has_r && has_d && linked(z[q], s_z[cell + kTileW + 1], L.max_diff, L.rel_diff)) b |= 4u;
            if (lx > 0 && has_d && linked(z[q], s_z[cell + kTileW - 1], L.max_diff, L.rel_diff)) b |= 8u;
        }
        bits[q] = b;
        if (inside[q]) {
            const bool need_r = has_r && x0 + lx + 1 < L.w, need_d = has_d && y0 + row + 1 < L.h;
            full &= z[q] > 0.0f && (!need_r || (b & 1u)) && (!need_d || (b & 2u));
        }
    }
    if (__syncthreads_and(full)) {                          // one component: its root is the tile's first pixel
        const int root = y0 * L.w + x0;
        const int tw = L.w - x0 < kTileW ? L.w - x0 : kTileW, th = L.h - y0 < kTileH ? L.h - y0 : kTileH;
#pragma unroll
        for (int q = 0; q < kPerThread; q++) {
            if (!inside[q]) continue;
            const size_t at = (size_t)(y0 + ly + q * (kTileH / kPerThread)) * (unsigned)L.w + (unsigned)(x0 + lx);
            parent[at] = root;
            size[at] = at == (size_t)root ? (uint32_t)(tw * th) : 0u;
        }
        if (tid == 0) part[2] = 0;
        return;
    }

    LdsOps lds{s_lab};
    bool capped = false;
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        const int cell = (ly + q * (kTileH / kPerThread)) * kTileW + lx;
        if (bits[q] & 1u) uf_union(lds, cell, cell + 1, capped);
        if (bits[q] & 2u) uf_union(lds, cell, cell + kTileW, capped);
        if (CONN8) {
            if (bits[q] & 4u) uf_union(lds, cell, cell + kTileW + 1, capped);
            if (bits[q] & 8u) uf_union(lds, cell, cell + kTileW - 1, capped);
        }
    }
    __syncthreads();
    int root[kPerThread];
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        const int cell = (ly + q * (kTileH / kPerThread)) * kTileW + lx;
        root[q] = cell;
        if (z[q] > 0.0f) {
            root[q] = uf_find(lds, cell, capped);
            atomicAdd(&s_size[root[q]], 1u);
        }
    }
    block_partials_u32(capped ? 1u : 0u, s_part);           // a barrier: s_size is complete behind it
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        if (!inside[q]) continue;
        const int row = ly + q * (kTileH / kPerThread), cell = row * kTileW + lx;
        const size_t at = (size_t)(y0 + row) * (unsigned)L.w + (unsigned)(x0 + lx);
        const int rrow = root[q] / kTileW, rcol = root[q] - rrow * kTileW;
        parent[at] = z[q] > 0.0f ? (y0 + rrow) * L.w + x0 + rcol : -1;
        if (z[q] > 0.0f) size[at] = root[q] == cell ? s_size[cell] : 0u;   // 0: not a local root (S3 reads it)
    }
    if (tid == 0) part[2] = block_sum_u32(s_part);
}

// S2: grid (ceil(seam pixels / 256), n), block 256
template <bool CONN8>
__global__ __launch_bounds__(kThreads) void speckle_seam_kernel(SpeckleLaunch L, unsigned column_pixels, unsigned seam_pixels)
{
    const unsigned idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= seam_pixels) return;
    const unsigned frame = blockIdx.y;
    const Frame F = frame_of(L, frame);
    GlobalOps g{L.parent + (size_t)frame * ((size_t)L.w * L.h)};
    const bool column = idx < column_pixels;
    int x, y;
    if (column) {
        x = (int)(idx / (unsigned)L.h + 1u) * kTileW;
        y = (int)(idx % (unsigned)L.h);
    } else {
        const unsigned j = idx - column_pixels;
        y = (int)(j / (unsigned)L.w + 1u) * kTileH;
        x = (int)(j % (unsigned)L.w);
    }
    const int p = y * L.w + x;
    const float zp = F.state((size_t)p);
    if (!(zp > 0.0f)) return;
    bool capped = false;
    for (int k = 0; k < (CONN8 ? 3 : 1); k++) {
        // k 0: the direct neighbour across the seam; 1, 2: the two diagonal ones
        const int d = k == 0 ? 0 : (k == 1 ? -1 : 1);
        const int nx = column ? x - 1 : x + d, ny = column ? y + d : y - 1;
        if ((unsigned)nx >= (unsigned)L.w || (unsigned)ny >= (unsigned)L.h) continue;
        const int q = ny * L.w + nx;
        if (linked(zp, F.state((size_t)q), L.max_diff, L.rel_diff)) uf_union(g, p, q, capped);
    }
    if (capped) atomicAdd(&L.capped[frame], 1u);
}

// S3: grid (ceil(pixels / 256), n), block 256
__global__ __launch_bounds__(kThreads) void speckle_resolve_kernel(SpeckleLaunch L)
{
    const size_t px = (size_t)L.w * L.h;
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= px) return;
    const unsigned frame = blockIdx.y;
    int32_t* parent = L.parent + (size_t)frame * px;
    const int32_t par = parent[at];
    if (par < 0 || par == (int32_t)at) return;              // no pixel of a component, or a global root
    uint32_t* size = L.size + (size_t)frame * px;
    const uint32_t local = size[at];                        // nothing is added to it: only global roots receive, and at is none
    if (local == 0) return;                                 // not a local root
    GlobalOps g{parent};
    bool capped = false;
    const int root = uf_find(g, (int)at, capped);
    atomicAdd(&size[root], local);
    parent[at] = root;
    if (capped) atomicAdd(&L.capped[frame], 1u);
}

// S4: grid (tiles of a frame, n), block 256
__global__ __launch_bounds__(kThreads) void speckle_apply_kernel(SpeckleLaunch L)
{
    __shared__ uint32_t s_count[2][4];
    const int tid = (int)threadIdx.x, lx = tid & (kTileW - 1), ly = tid >> 5;
    const unsigned frame = blockIdx.y;
    const int tiles_x = (L.w + kTileW - 1) / kTileW;
    const int trow = (int)blockIdx.x / tiles_x, tcol = (int)blockIdx.x - trow * tiles_x;
    const int x0 = tcol * kTileW, y0 = trow * kTileH;
    const size_t px = (size_t)L.w * L.h;
    const Frame F = frame_of(L, frame);
    const bool out_f32 = L.out_format == KDE_DEPTH_F32;
    char* dframe = static_cast<char*>(L.out) + (size_t)frame * px * (out_f32 ? sizeof(float) : sizeof(uint16_t));
    int32_t* lframe = L.labels ? L.labels + (size_t)frame * px : nullptr;
    GlobalOps g{L.parent + (size_t)frame * px};
    const uint32_t* size = L.size + (size_t)frame * px;
    uint32_t removed = 0, components = 0;
    bool capped = false;
#pragma unroll
    for (int q = 0; q < kPerThread; q++) {
        const int x = x0 + lx, y = y0 + ly + q * (kTileH / kPerThread);
        if (x >= L.w || y >= L.h) continue;
        const int p = y * L.w + x;
        const float z = F.state((size_t)p);
        int label = -1;
        if (z > 0.0f) {
            const int root = uf_find(g, p, capped);
            if (size[root] >= (uint32_t)L.min_size) {
                label = root;
                components += root == p;
            } else {
                removed++;
            }
        }
        store_depth(dframe, out_f32, (size_t)p, label >= 0 ? z : 0.0f);
        if (lframe) lframe[p] = label;
    }
    if (capped) atomicAdd(&L.capped[frame], 1u);
    removed = wave_sum_u32(removed);
    components = wave_sum_u32(components);
    if ((tid & 63) == 0) {
        s_count[0][tid >> 6] = removed;
        s_count[1][tid >> 6] = components;
    }
    __syncthreads();
    if (tid < 2) L.partial[((size_t)frame * gridDim.x + blockIdx.x) * 3 + tid] = block_sum_u32(s_count[tid]);
}

// S5: grid n, block 256
__global__ __launch_bounds__(kThreads) void speckle_count_kernel(const uint32_t* __restrict__ partial, unsigned groups, uint32_t* __restrict__ removed,
                                                                 uint32_t* __restrict__ components, uint32_t* __restrict__ capped)
{
    __shared__ uint32_t s_count[3][4];
    const uint32_t* p = partial + (size_t)blockIdx.x * groups * 3;
    uint32_t a = 0, b = 0, c = 0;
    for (unsigned g = threadIdx.x; g < groups; g += kThreads) {
        a += p[3 * g];
        b += p[3 * g + 1];
        c += p[3 * g + 2];
    }
    a = wave_sum_u32(a);
    b = wave_sum_u32(b);
    c = wave_sum_u32(c);
    if ((threadIdx.x & 63u) == 0) {
        s_count[0][threadIdx.x >> 6] = a;
        s_count[1][threadIdx.x >> 6] = b;
        s_count[2][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        removed[blockIdx.x] = block_sum_u32(s_count[0]);
        components[blockIdx.x] = block_sum_u32(s_count[1]);
        capped[blockIdx.x] += block_sum_u32(s_count[2]);    // what S2 .. S4 added since S1 zeroed it, plus the tiles' own
    }
}

}  // namespace

unsigned speckle_groups(int w, int h)
{
    return (unsigned)((long long)((w + kTileW - 1) / kTileW) * ((h + kTileH - 1) / kTileH));
}

int launch_speckle(const SpeckleLaunch& a, hipStream_t s)
{
    if (a.connectivity != 4 && a.connectivity != 8) return fail(KDE_ERR_INVALID, "launch_speckle: connectivity %d", a.connectivity);
    const bool conn8 = a.connectivity == 8;
    const unsigned groups = speckle_groups(a.w, a.h);
    const dim3 tiles(groups, (unsigned)a.n), block(kThreads);
    const unsigned tiles_x = (unsigned)((a.w + kTileW - 1) / kTileW), tiles_y = (unsigned)((a.h + kTileH - 1) / kTileH);
    const unsigned column_pixels = (tiles_x - 1) * (unsigned)a.h, seam_pixels = column_pixels + (tiles_y - 1) * (unsigned)a.w;
    const size_t px = (size_t)a.w * a.h;
    if (conn8) hipLaunchKernelGGL(speckle_tile_kernel<true>, tiles, block, 0, s, a);
    else hipLaunchKernelGGL(speckle_tile_kernel<false>, tiles, block, 0, s, a);
    if (seam_pixels) {
        const dim3 grid((seam_pixels + kThreads - 1) / kThreads, (unsigned)a.n);
        if (conn8) hipLaunchKernelGGL(speckle_seam_kernel<true>, grid, block, 0, s, a, column_pixels, seam_pixels);
        else hipLaunchKernelGGL(speckle_seam_kernel<false>, grid, block, 0, s, a, column_pixels, seam_pixels);
        hipLaunchKernelGGL(speckle_resolve_kernel, dim3((unsigned)((px + kThreads - 1) / kThreads), (unsigned)a.n), block, 0, s, a);
    }
    hipLaunchKernelGGL(speckle_apply_kernel, tiles, block, 0, s, a);
    hipLaunchKernelGGL(speckle_count_kernel, dim3((unsigned)a.n), block, 0, s, a.partial, groups, a.removed, a.components, a.capped);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
