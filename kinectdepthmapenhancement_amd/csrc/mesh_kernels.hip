// mesh_kernels.hip — OrganizedMesh: the triangle mesh of an organised depth grid for n frames.  The vertices are the dense
// cloud of cloud_kernels.hip (launch_cloud, as it is): the vertex index of a valid pixel is its rank in raster order.  Every
// pixel (x, y) with x < W - 1 and y < H - 1 owns the quad a = (x, y), b = (x + 1, y), c = (x, y + 1), d = (x + 1, y + 1), which
// gives 0, 1 or 2 of the four triangles T0 = (a, c, d), T1 = (a, d, b), T2 = (a, c, b), T3 = (b, c, d): a triangle needs its
// three corners valid and its three edges linked (depth_close, the link of the speckle filter); four valid corners are cut
// along a-d (T0, T1) or b-c (T2, T3), three valid corners leave the one triangle without the missing corner.
//   M1 classify  grid of C1: a thread owns a pixel octet (load_octet) and reads the z of the pixel behind it and of the nine
//                pixels below with plain loads.  It writes the octet's validity byte, one byte per pixel with the set of
//                triangles its quad gives, per 64-pixel group the vertices of the segment before it, and the segment's
//                triangle count.
//   M2 scan      launch_segment_scan (cloud_kernels.hip) over the triangle counts: offsets per segment, tri_count[f]
//   M3 emit      grid of C1, integer only: a thread reads its eight triangle bytes, the workgroup ranks its triangles (wave
//                scan and four wave totals), every triangle gets the ranks of its corners from the tables,
//                rank(j) = segment offset[j >> 11] + group rank[j >> 6] + popcount(mask[j >> 6] below bit j & 63),
//                the triples are staged in LDS in output order and stored as consecutive dwords.
// No workgroup waits for another inside a launch and no position comes from an atomic: the triangles are a function of the
// frame alone, for any batch size, place in the batch and pointer alignment.
#include "kde_internal.h"
#include "kde_device_math.h"
#include "kde_source_load.h"

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned kSegmentOctets = kCloudSegmentPixels / 8;
static_assert(kSegmentOctets == kThreads, "a thread owns one octet of its segment");
static_assert(kMeshGroupPixels == 64, "a group is one 64-bit validity word, eight lanes");
constexpr unsigned kSegmentTriangles = 2 * kCloudSegmentPixels;

__device__ __forceinline__ bool mesh_valid(float z, const CloudLaunch& c) { return z > c.z_min && z < c.z_max; }   // cloud_valid

// the z of pixel j of a frame as load_octet gives it; NaN beyond the frame
__device__ __forceinline__ float z_at(const char* frame, int format, unsigned j, unsigned px)
{
    if (j >= px) return NAN;
    if (format == KDE_SRC_POINTS_F32) return reinterpret_cast<const float*>(frame)[3 * (size_t)j + 2];
    if (format == KDE_SRC_DEPTH_F32) return reinterpret_cast<const float*>(frame)[j];
    return (float)reinterpret_cast<const uint16_t*>(frame)[j];
}

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, unsigned lane)
{
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// M1: grid (segments of a frame, n), block 256
template <bool NT>
__global__ __launch_bounds__(kThreads) void mesh_classify_kernel(MeshLaunch a)
{
    __shared__ float4 xch[kWaves][6 * 64];
    __shared__ uint32_t wave_v[kWaves], wave_t[kWaves];
    const CloudLaunch& c = a.cloud;
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned W = (unsigned)c.cam.width, px = W * (unsigned)c.cam.height;
    const unsigned seg = blockIdx.x, frame = blockIdx.y;
    const char* sframe = static_cast<const char*>(c.src) + (size_t)frame * px * source_element_size(c.format);
    const bool vec = (reinterpret_cast<uintptr_t>(sframe) & 15u) == 0;
    float P[24];
    load_octet<NT>(sframe, c.format, vec, seg * kSegmentOctets + wv * 64u, lane, px, c.cam, xch[wv], P);
    const unsigned oct = seg * kSegmentOctets + threadIdx.x, j0 = oct * 8;
    float top[9], bot[9];
#pragma unroll
    for (unsigned k = 0; k < 8; k++) top[k] = P[3 * k + 2];
    top[8] = z_at(sframe, c.format, j0 + 8, px);
#pragma unroll
    for (unsigned k = 0; k < 9; k++) bot[k] = z_at(sframe, c.format, j0 + W + k, px);
    bool vt[9], vb[9];
#pragma unroll
    for (unsigned k = 0; k < 9; k++) {
        vt[k] = mesh_valid(top[k], c);
        vb[k] = mesh_valid(bot[k], c);
    }
    unsigned x = j0 % W;
    uint32_t vbits = 0, nv = 0, nt = 0, code[2] = {0u, 0u};
#pragma unroll
    for (unsigned k = 0; k < 8; k++) {
        vbits |= vt[k] ? 1u << k : 0u;
        nv += vt[k] ? 1u : 0u;
        // the pixel owns a quad iff it is not in the last column and has a row below it
        const bool quad = x + 1 < W && j0 + k + W < px;
        const float za = top[k], zb = top[k + 1], zc = bot[k], zd = bot[k + 1];
        const bool va = vt[k], vb_ = vt[k + 1], vc = vb[k], vd = vb[k + 1];
        const bool four = va && vb_ && vc && vd;
        const bool bc = a.diagonal == KDE_MESH_DIAG_BC || (a.diagonal == KDE_MESH_DIAG_ADAPTIVE && fabsf(zb - zc) < fabsf(za - zd));
        // four corners: the two triangles of the cut; three: the only triangle whose corners are all valid passes below
        const unsigned cand = four ? (bc ? 12u : 3u) : 15u;
        const bool lab = va && vb_ && depth_close(za, zb, a.max_diff, a.rel_diff);
        const bool lac = va && vc && depth_close(za, zc, a.max_diff, a.rel_diff);
        const bool lbd = vb_ && vd && depth_close(zb, zd, a.max_diff, a.rel_diff);
        const bool lcd = vc && vd && depth_close(zc, zd, a.max_diff, a.rel_diff);
        const bool lad = va && vd && depth_close(za, zd, a.max_diff, a.rel_diff);
        const bool lbc = vb_ && vc && depth_close(zb, zc, a.max_diff, a.rel_diff);
        unsigned m = (lac && lcd && lad ? 1u : 0u) | (lad && lbd && lab ? 2u : 0u) | (lac && lbc && lab ? 4u : 0u) |
                     (lbc && lcd && lbd ? 8u : 0u);
        m = quad ? (m & cand) : 0u;
        nt += __popc(m);
        code[k >> 2] |= m << (8 * (k & 3));
        if (++x == W) x = 0;
    }
    const size_t tp = (size_t)gridDim.x * kCloudSegmentPixels;    // mesh_table_pixels(px)
    *reinterpret_cast<uint2*>(a.code + (size_t)frame * tp + j0) = make_uint2(code[0], code[1]);
    a.mask[(size_t)frame * (tp / 8) + oct] = (uint8_t)vbits;
    const uint32_t sv = wave_scan(nv, lane), st = wave_scan(nt, lane);
    if (lane == 63) {
        wave_v[wv] = sv;
        wave_t[wv] = st;
    }
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (unsigned w = 0; w < (unsigned)kWaves; w++) {
        if (w < wv) before += wave_v[w];
    }
    if ((lane & 7u) == 0) a.group_rank[(size_t)frame * (tp / kMeshGroupPixels) + (j0 >> 6)] = before + (sv - nv);
    if (threadIdx.x == 0) a.tri_seg[(size_t)frame * gridDim.x + seg] = (wave_t[0] + wave_t[1]) + (wave_t[2] + wave_t[3]);
}

// M3: grid (segments of a frame, n), block 256
template <bool NT>
__global__ __launch_bounds__(kThreads) void mesh_emit_kernel(MeshLaunch a)
{
    __shared__ uint32_t stage[3 * kSegmentTriangles];      // 48 KB: the segment's triples in output order
    __shared__ uint32_t wave_t[kWaves];
    const CloudLaunch& c = a.cloud;
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned W = (unsigned)c.cam.width, H = (unsigned)c.cam.height;
    const unsigned seg = blockIdx.x, segs = gridDim.x, frame = blockIdx.y;
    const size_t tp = (size_t)gridDim.x * kCloudSegmentPixels;    // mesh_table_pixels(px)
    const unsigned groups = (unsigned)(tp / kMeshGroupPixels);
    const unsigned j0 = (seg * kSegmentOctets + threadIdx.x) * 8;
    const uint2 cw = *reinterpret_cast<const uint2*>(a.code + (size_t)frame * tp + j0);
    const uint32_t nt = __popc(cw.x) + __popc(cw.y);
    const uint32_t st = wave_scan(nt, lane);
    if (lane == 63) wave_t[wv] = st;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (unsigned w = 0; w < (unsigned)kWaves; w++) {
        if (w < wv) before += wave_t[w];
    }
    const uint32_t total = (wave_t[0] + wave_t[1]) + (wave_t[2] + wave_t[3]);       // <= kSegmentTriangles
    if (nt) {
        const uint64_t* mask = reinterpret_cast<const uint64_t*>(a.mask + (size_t)frame * (tp / 8));
        const uint32_t* grank = a.group_rank + (size_t)frame * groups;
        const uint32_t* vseg = c.seg + (size_t)frame * segs;
        // a pixel with a triangle has a row below it: j0 + W lies inside the frame, so inside the tables
        const unsigned jt = j0, jb = j0 + W;
        uint32_t rank[2], win[2];
#pragma unroll
        for (unsigned r = 0; r < 2; r++) {
            const unsigned j = r ? jb : jt, g = j >> 6, sh = j & 63u;
            const uint64_t word = mask[g];
            rank[r] = vseg[j >> 11] + grank[g] + (uint32_t)__popcll(word & ((1ull << sh) - 1ull));
            uint64_t bits = word >> sh;
            if (sh > 55u && g + 1 < groups) bits |= mask[g + 1] << (64u - sh);
            win[r] = (uint32_t)bits & 0x1ffu;               // the validity of the nine pixels j .. j + 8
        }
        uint32_t* out = stage + 3 * (size_t)(before + (st - nt));
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            const unsigned m = ((k < 4 ? cw.x : cw.y) >> (8 * (k & 3))) & 0xffu;
            if (m == 0) continue;
            const uint32_t ia = rank[0] + __popc(win[0] & ((1u << k) - 1u)), ib = rank[0] + __popc(win[0] & ((2u << k) - 1u));
            const uint32_t ic = rank[1] + __popc(win[1] & ((1u << k) - 1u)), id = rank[1] + __popc(win[1] & ((2u << k) - 1u));
#pragma unroll
            for (unsigned t = 0; t < 4; t++) {
                if (!(m & (1u << t))) continue;
                const uint32_t v0 = t == 3 ? ib : ia;
                uint32_t v1 = t == 1 ? id : ic;
                uint32_t v2 = t == 0 || t == 3 ? id : ib;
                if (a.flip_winding) {
                    const uint32_t s = v1;
                    v1 = v2;
                    v2 = s;
                }
                out[0] = v0;
                out[1] = v1;
                out[2] = v2;
                out += 3;
            }
        }
    }
    __syncthreads();
    const size_t slot = 2 * (size_t)(W - 1) * (H - 1);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.triangles + (size_t)frame * slot + a.tri_seg[(size_t)frame * segs + seg]);
    for (unsigned i = threadIdx.x; i < 3 * total; i += kThreads) {
        if (NT) __builtin_nontemporal_store(stage[i], dst + i);
        else dst[i] = stage[i];
    }
}

}  // namespace

int launch_mesh(const MeshLaunch& a, hipStream_t s)
{
    const CloudLaunch& c = a.cloud;
    KDE_TRY(launch_cloud(c, s));
    const size_t px = (size_t)c.cam.width * c.cam.height;
    const unsigned segs = cloud_segments(px);
    const size_t esz = c.format == KDE_SRC_POINTS_F32 ? sizeof(kde_float3) : c.format == KDE_SRC_DEPTH_F32 ? sizeof(float) : sizeof(uint16_t);
    const size_t slot = 2 * (size_t)(c.cam.width - 1) * (c.cam.height - 1);
    const size_t bytes = px * c.n * (esz + sizeof(kde_cloud_point)) + px * c.bgr_frames * 3 + slot * c.n * sizeof(kde_mesh_triangle);
    const bool nt = past_cache(kSiteMesh, bytes);
    const dim3 grid(segs, (unsigned)c.n), block(kThreads);
    if (nt) hipLaunchKernelGGL(mesh_classify_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(mesh_classify_kernel<false>, grid, block, 0, s, a);
    KDE_TRY(launch_segment_scan(a.tri_seg, segs, a.tri_counts, c.n, s));
    if (nt) hipLaunchKernelGGL(mesh_emit_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(mesh_emit_kernel<false>, grid, block, 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
