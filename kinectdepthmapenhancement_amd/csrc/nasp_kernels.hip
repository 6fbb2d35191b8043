// nasp_kernels.hip — NormalAdaptiveSuperpixel on gfx950.
// Reference: SuperpixelSegmentation/NormalAdaptiveSuperpixel.cu:3-1103 (5 kernels); definition and the deviations
// NA1-NA5 in DESIGN.md ("Normal-adaptive superpixels").  Every output is bit-comparable with tools/nasp_ref.c.
//
// Re-architecture vs the reference:
//   initLD_NASP is folded into the first calculateLD_NASP (the previous assignment "own grid cell at 999999.9" is formed
//      in registers), as K5 is folded into K7.  A call with iteration = 0 has no first calculateLD_NASP: it runs
//      nasp_init_ld_kernel, so that LD is what the reference's initLD_NASP leaves (labels stay as they were, as there).
//   sampleInitialClusters_NASP: one wavefront per cluster, one candidate per lane; the 121 absolute taps (colour, normal
//      and the tap's bad-normal test) are staged in LDS once per workgroup.
//   calculateLD_NASP launches one 64-thread block per PIXEL in the reference; here one thread owns one pixel and walks its
//      64 candidate clusters in registers with the cluster table (40 B per cluster) in LDS.  The 64-way strict-'>' tree is
//      evaluated LITERALLY, depth first: leaves are visited in bit-reversed order and finished sub-trees are combined as a
//      binary counter carries, which needs a stack of six (distance, label) pairs instead of 64 -- the same 63 comparisons
//      on the same operands as the reference's tree, so NaN distances (NaN normals exist) need no separate argument.
//   analyzeClusters_NASP / calculateWeightedAverage keep the reference's summation order (per-thread serial, then a
//      256-way tree) so the float sums agree bit for bit; clusters are walked in XCD bands as K8's, and the two passes
//      of a cluster run in ONE workgroup, the record the first stores handed to the second through LDS.
//   The two expf of the weighted pass are host-built tables over their integer numerators (NA4); the acos test is a
//      comparison of its argument with a host-derived threshold (NA3).
#include "kde_internal.h"
#include "kde_device_math.h"
#include "kde_superpixel_device.h"

namespace kde {
namespace {

// (lt_mask / sel_f / sel_i, f2i_rz, tree256 and the record tail: kde_superpixel_device.h)
__device__ __forceinline__ bool ok3_and(const kde_float3& n) { return n.x != -1.0f && n.y != -1.0f && n.z != -1.0f; }   // .cu:57-62
__device__ __forceinline__ bool ok3_or(const kde_float3& n) { return n.x != -1.0f || n.y != -1.0f || n.z != -1.0f; }    // .cu:240-245

struct FramePtrs {
    const uint8_t* bgr;
    const kde_float3* pts;
    const kde_float3* nrm;
    kde_label_distance* ld;
    int32_t* labels;
    kde_superpixel* mean;
    kde_float3* centers;
    kde_float3* spn;
    float* variance;
};
__device__ __forceinline__ FramePtrs frame_ptrs(const NaspLaunch& a, unsigned frame)
{
    const size_t fpx = (size_t)frame * a.g.width * a.g.height, fk = (size_t)frame * a.g.rows * a.g.cols;
    return FramePtrs{a.bgr + fpx * 3, a.pts + fpx, a.nrm + fpx, a.ld + fpx, a.labels + fpx, a.mean + fk, a.centers + fk, a.spn + fk,
                     a.variance + fk};
}

// ---- sampleInitialClusters_NASP<64> (.cu:16-182) -----------------------------------------------------------------
// grid = (clusters, frames), one wavefront per cluster.  NA5: the record starts with size 0 and the variance with 0.
__global__ __launch_bounds__(64) void nasp_sample_kernel(NaspLaunch a)
{
    const DaspGeom& g = a.g;
    const FramePtrs f = frame_ptrs(a, blockIdx.y);
    const int lane = threadIdx.x;
    const int cluster = blockIdx.x;
    const int bx = cluster % g.cols, by = cluster / g.cols;
    const long npix = (long)g.width * g.height;
    // the 11 x 11 taps are addressed ABSOLUTELY (idx = yy*width + xx, .cu:54-65): the same 121 for every candidate
    __shared__ float tc[121][3];
    __shared__ float tn[121][3];
    __shared__ int tok[121];
    for (int i = lane; i < 121; i += 64) {
        const int yy = i / 11 - 5, xx = i % 11 - 5;
        const long idx = (long)yy * g.width + xx;
        float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
        kde_float3 n{0.0f, 0.0f, 0.0f};                          // NA1
        if (idx >= 0 && idx < npix) {
            t0 = (float)f.bgr[idx * 3];
            t1 = (float)f.bgr[idx * 3 + 1];
            t2 = (float)f.bgr[idx * 3 + 2];
            n = f.nrm[idx];
        }
        tc[i][0] = t0; tc[i][1] = t1; tc[i][2] = t2;
        tn[i][0] = n.x; tn[i][1] = n.y; tn[i][2] = n.z;
        tok[i] = ok3_and(n) ? 1 : 0;
    }
    __syncthreads();
    const int tx = lane & 7, ty = lane >> 3;
    int ax = bx * g.wx + g.wx / 2 + tx - 4;
    int ay = by * g.wy + g.wy / 2 + ty - 4;
    const size_t pa = (size_t)ay * g.width + ax;
    const float a0 = (float)f.bgr[pa * 3], a1 = (float)f.bgr[pa * 3 + 1], a2 = (float)f.bgr[pa * 3 + 2];
    const kde_float3 na = f.nrm[pa];
    const bool a_ok = ok3_and(na);
    float sumG = 0.0f;
    int count = 0;
    for (int i = 0; i < 121; i++) {                       // yy outer, xx inner: the reference's summation order
        const float d0 = a0 - tc[i][0], d1 = a1 - tc[i][1], d2 = a2 - tc[i][2];
        float gr = sqrt_int24(d0 * d0 + d1 * d1 + d2 * d2);        // integer-valued, <= 3 * 255^2: exact like sqrtf
        const float normal_diff = fabsf(na.x * tn[i][0] + na.y * tn[i][1] + na.z * tn[i][2]);
        const float scaled = gr * (1.0f - normal_diff);
        gr = (a_ok && tok[i]) ? scaled : gr;
        count += gr > 0.0f ? 1 : 0;
        sumG += gr;
    }
    float gradient = sumG / (float)count;
    // 64-element tree argmin, strict '>' (.cu:120-163); a lane >= step is not part of the level
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const float og = __shfl_down(gradient, step, 64);
        const int ox = __shfl_down(ax, step, 64);
        const int oy = __shfl_down(ay, step, 64);
        if (lane < step && gradient > og) {
            gradient = og;
            ax = ox;
            ay = oy;
        }
    }
    if (lane == 0) {
        const int id = by * (g.width / g.wx) + bx;
        const size_t ps = (size_t)ay * g.width + ax;
        kde_superpixel m;
        m.x = ax;
        m.y = ay;
        m.r = f.bgr[ps * 3];
        m.g = f.bgr[ps * 3 + 1];
        m.b = (uint8_t)(f.bgr[ps * 3] + 2);   // sic, .cu:173
        m.pad_ = 0;
        m.size = 0;                           // NA5
        f.mean[id] = m;
        f.centers[id] = f.pts[ps];
        f.spn[id] = f.nrm[ps];
        f.variance[id] = 0.0f;                // NA5
    }
}

// ---- calculateLD_NASP<64> (.cu:184-354) ----------------------------------------------------------------------------
struct NaspRec {          // LDS copy of one cluster: 40 B
    float r, g, b, cz;
    int xi, yi;
    float nx, ny, nz;
    int nok;              // the cluster normal passes the '||' test of .cu:243-245
};
constexpr int kNaspMaxLdsClusters = 1536;   // 60 KiB of LDS

__device__ __forceinline__ NaspRec make_rec(const kde_superpixel& m, const kde_float3& c, const kde_float3& n)
{
    NaspRec r;
    r.r = (float)m.r; r.g = (float)m.g; r.b = (float)m.b;
    r.cz = c.z;
    r.xi = m.x; r.yi = m.y;
    r.nx = n.x; r.ny = n.y; r.nz = n.z;
    r.nok = ok3_or(n) ? 1 : 0;
    return r;
}

// initLD_NASP (.cu:3-14) on its own, for a Segmentation of no iteration.  grid as nasp_calc_ld_kernel's: (ceil(W / 64),
// ceil(H / 4), frames), one thread per pixel.
__global__ __launch_bounds__(256) void nasp_init_ld_kernel(NaspLaunch a)
{
    const DaspGeom& g = a.g;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.width || y >= g.height) return;
    kde_label_distance o;
    o.l = (y / g.wy) * g.cols + (x / g.wx);
    o.d = 999999.9f;
    frame_ptrs(a, blockIdx.z).ld[(size_t)y * g.width + x] = o;
}

template <bool USE_LDS, bool FIRST>
__global__ __launch_bounds__(256) void nasp_calc_ld_kernel(NaspLaunch a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    NaspRec* recs = reinterpret_cast<NaspRec*>(smem);
    const DaspGeom& g = a.g;
    const FramePtrs f = frame_ptrs(a, blockIdx.z);
    const int nclusters = g.rows * g.cols;
    if (USE_LDS) {
        for (int i = threadIdx.x; i < nclusters; i += 256) recs[i] = make_rec(f.mean[i], f.centers[i], f.spn[i]);
        __syncthreads();
    }
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.width || y >= g.height) return;
    const size_t p = (size_t)y * g.width + x;
    const float c0 = (float)f.bgr[p * 3], c1 = (float)f.bgr[p * 3 + 1], c2 = (float)f.bgr[p * 3 + 2];
    const float z = f.pts[p].z;
    const kde_float3 pn = f.nrm[p];
    const bool pn_ok = ok3_or(pn);

    kde_label_distance cur;
    if (FIRST) {                                                // initLD_NASP (.cu:3-14)
        cur.l = (y / g.wy) * g.cols + (x / g.wx);
        cur.d = 999999.9f;
    } else {
        cur = f.ld[p];
    }
    const int ccx = cur.l % g.cols, ccy = cur.l / g.cols;      // C's truncating % and / (-1: unassigned)

    // the distance to cluster id (.cu:222-258); NA2: normal_distance is 0 where the reference leaves it uninitialised
    auto distance = [&](int id) {
        const NaspRec r = USE_LDS ? recs[id] : make_rec(f.mean[id], f.centers[id], f.spn[id]);
        const float e0 = c0 - r.r, e1 = c1 - r.g, e2 = c2 - r.b;
        const float color_distance = e0 * e0 + e1 * e1 + e2 * e2;
        // (x - mean.x wraps for a centre kept far below the image, as the reference's int subtraction does)
        const float px = (float)(int)((unsigned)x - (unsigned)r.xi), py = (float)(int)((unsigned)y - (unsigned)r.yi);
        const float n2 = px * px + py * py;
        // sqrt_int24 is sqrtf on integers below 2^24 (n2 < 2^24 as a float means the exact sum is that integer)
        float sq;
        if (__builtin_amdgcn_ballot_w64(!(n2 < 16777216.0f)) == 0) sq = sqrt_int24(n2);
        else sq = sqrtf(n2);
        const float spatial_distance = sq * a.win2;
        const bool valid = z > 50.0f && r.cz > 50.0f;
        const float depth_distance = valid ? fabsf(z - r.cz) : 0.0f;
        float normal_diff = pn.x * r.nx + pn.y * r.ny + pn.z * r.nz;
        normal_diff = normal_diff < 0.0f ? 0.0f : normal_diff;
        const float nd = (float)(65025.0 * (1.0 - (double)normal_diff));       // .cu:250: in double, rounded once
        const float normal_distance = (valid && pn_ok && r.nok) ? nd : 0.0f;
        return color_distance * a.kc + spatial_distance * a.ks + depth_distance * a.kd + normal_distance * a.kn;   // .cu:257
    };

    // The reference's 64-way tree (.cu:304-341) is a balanced binary tree over the leaves in BIT-REVERSED order (the last
    // level joins the even with the odd leaves, the first level leaf t with t + 32), each node keeping its left child unless
    // left > right.  Depth first: stack level b holds a finished sub-tree of 2^b leaves that waits for its right sibling.
    float sd[6];
    int sl[6];
    float fd = 0.0f;
    int fl = 0;
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int t = ((k & 1) << 5) | ((k & 2) << 3) | ((k & 4) << 1) | ((k & 8) >> 1) | ((k & 16) >> 3) | ((k & 32) >> 5);
        const int rx = ccx - 4 + (t & 7), ry = ccy - 4 + (t >> 3);
        const bool in = rx >= 0 && rx < g.cols && ry >= 0 && ry < g.rows;
        float d = cur.d;                                         // .cu:261-264 outside the grid
        int l = cur.l;
        if (__builtin_amdgcn_ballot_w64(in) != 0) {              // some lane of the wavefront has this candidate
            const int id = in ? ry * g.cols + rx : 0;
            const float dv = distance(id);
            d = in ? dv : d;
            l = in ? id : l;
        }
#pragma unroll
        for (int b = 0; b < 6; b++) {
            if (!((k >> b) & 1)) {
                if (b < 6) { sd[b] = d; sl[b] = l; }
                break;
            }
            const uint64_t take = lt_mask(d, sd[b]);             // left > right: the right child replaces the left
            d = sel_f(take, d, sd[b]);
            l = sel_i(take, l, sl[b]);
        }
        if (k == 63) { fd = d; fl = l; }
    }
    kde_label_distance o;
    o.l = fl;
    o.d = fd;
    if (z < 50.0f && a.reset_on) {            // .cu:348-353
        o.l = -1;
        o.d = 0.0f;
    }
    f.ld[p] = o;
    f.labels[p] = o.l;
}

// z of the point under a new cluster centre (.cu:635, :1014).  The reference indexes unchecked; a position outside the
// image (only an overflowing sum or a non-finite weight can produce one) reads z = 0
__device__ __forceinline__ bool center_point(const DaspGeom& g, const kde_float3* pts, int px, int py, kde_float3* out)
{
    if (px < 0 || px >= g.width || py < 0 || py >= g.height) return false;
    *out = pts[(size_t)py * g.width + px];
    return out->z > 50.0f;
}

struct ClusterWalk {        // which cluster of which frame a workgroup serves, in XCD bands (see K8)
    unsigned frame;
    int cluster_id;
};
__device__ __forceinline__ ClusterWalk cluster_walk(const DaspGeom& g)
{
    const unsigned ncl = (unsigned)(g.rows * g.cols);
    const unsigned gid = xcd_band_id(blockIdx.x, gridDim.x);
    ClusterWalk w;
    w.frame = gid / ncl;
    w.cluster_id = (int)(gid - w.frame * ncl);
    return w;
}

// A thread's rpx x rpy sub-window of the 2w x 2h scan around (mx, my), walked in the reference's order (yy outer, xx inner:
// the float sums depend on it): body(q, arx, ary, ox, oy) runs for every position inside the image whose label is
// cluster_id, (ox, oy) its offset from the centre.  The labels of up to CH positions of a row are fetched together before
// any of them is acted on, so a row costs one load round trip for its labels instead of one per position.
// 32-bit wrapping adds, as the reference's: a centre kept below the image scans rows that wrap to negative.
template <class Body>
__device__ __forceinline__ void walk_members(const DaspGeom& g, const int32_t* __restrict__ labels, int mx, int my, int tx, int ty,
                                             int rpx, int rpy, int cluster_id, Body&& body)
{
    constexpr int CH = 8;
    const int ox0 = (tx - 8) * rpx, oy0 = (ty - 8) * rpy;
    for (int yy = 0; yy < rpy; yy++) {
        const int ary = (int)((unsigned)my + (unsigned)(oy0 + yy));
        if (ary < 0 || ary >= g.height) continue;
        for (int xc = 0; xc < rpx; xc += CH) {
            int l[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) {
                const int arx = (int)((unsigned)mx + (unsigned)(ox0 + xc + k));
                const bool in = xc + k < rpx && arx >= 0 && arx < g.width;
                l[k] = in ? labels[(size_t)ary * g.width + arx] : -2;         // -2: never a cluster id
            }
#pragma unroll
            for (int k = 0; k < CH; k++) {
                if (l[k] != cluster_id) continue;
                const int arx = (int)((unsigned)mx + (unsigned)(ox0 + xc + k));
                body((size_t)ary * g.width + arx, arx, ary, ox0 + xc + k, oy0 + yy);
            }
        }
    }
}

struct ClusterRecord {      // what the weighted pass reads of its cluster
    kde_superpixel m;
    kde_float3 spn;
};

// ---- analyzeClusters_NASP<256> (.cu:356-685) -----------------------------------------------------------------------
// `labels` is the label map calculateLD_NASP writes next to its (distance, label) records: the same labels, 4 B per pixel.
// Thread 0 stores the new record (nothing for an empty cluster, .cu:624) and returns in *rec what the cluster's record
// now is; the other threads' *rec is untouched.  buf: 13 x 256 words.
__device__ __forceinline__ void analyze_pass(const NaspLaunch& a, const FramePtrs& f, int cluster_id, int tid, uint32_t (*buf)[256],
                                             const kde_superpixel& m0, ClusterRecord* rec)
{
    const DaspGeom& g = a.g;
    const int rpx = g.wx * 2 / 16 + 1, rpy = g.wy * 2 / 16 + 1;
    int iv[7] = {0, 0, 0, 0, 0, 0, 0};                      // r g b x y size npoints
    float fv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};     // X Y Z nx ny nz
    walk_members(g, f.labels, m0.x, m0.y, tid & 15, tid >> 4, rpx, rpy, cluster_id, [&](size_t q, int arx, int ary, int, int) {
        iv[0] += (int)f.bgr[q * 3];
        iv[1] += (int)f.bgr[q * 3 + 1];
        iv[2] += (int)f.bgr[q * 3 + 2];
        iv[3] = (int)((unsigned)iv[3] + (unsigned)arx);
        iv[4] = (int)((unsigned)iv[4] + (unsigned)ary);
        iv[5] += 1;
        const kde_float3 pt = f.pts[q];
        const kde_float3 n = f.nrm[q];
        if (pt.z > 50.0f && ok3_or(n)) {
            fv[0] += pt.x; fv[1] += pt.y; fv[2] += pt.z;
            fv[3] += n.x; fv[4] += n.y; fv[5] += n.z;
            iv[6] += 1;
        }
    });
    tree256<7, 6>(tid, buf, iv, fv);
    if (tid != 0) return;
    if (iv[5] == 0) {                              // .cu:623-624: nothing is stored
        rec->m = m0;
        rec->spn = f.spn[cluster_id];
        return;
    }
    const int size = iv[5], np = iv[6];
    const int mean_x = iv[3] / size, mean_y = iv[4] / size;
    int pix_x = mean_x, pix_y = mean_y;
    if (np != 0) {
        kde_float3 c;
        if (center_point(g, f.pts, pix_x, pix_y, &c)) {
            f.centers[cluster_id] = c;
        } else {
            c = mean3(fv[0], fv[1], fv[2], np);
            f.centers[cluster_id] = c;
            reproject_centre(c, a.intr, g.width, g.height, mean_x, mean_y, pix_x, pix_y);   // sic, .cu:652
        }
        rec->spn = mean3(fv[3], fv[4], fv[5], np);
    } else {
        rec->spn = kde_float3{-1.0f, -1.0f, -1.0f};
        f.centers[cluster_id] = kde_float3{0.0f, 0.0f, 0.0f};
    }
    f.spn[cluster_id] = rec->spn;
    rec->m.r = channel_mean(iv[0] / size);
    rec->m.g = channel_mean(iv[1] / size);
    rec->m.b = channel_mean(iv[2] / size);
    rec->m.pad_ = 0;
    rec->m.x = pix_x;
    rec->m.y = pix_y;
    rec->m.size = size;
    f.mean[cluster_id] = rec->m;
}

// ---- calculateWeightedAverage<256> (.cu:687-1068) ------------------------------------------------------------------
__device__ __forceinline__ float clamp255(float v)
{
    v = v > 255.0f ? 255.0f : v;
    return v < 0.0f ? 0.0f : v;
}
// NA4: the weight of integer numerator `num` (exact as a float below the table length); 0 beyond the table's end
__device__ __forceinline__ float table_weight(const float* __restrict__ tab, int n, float num)
{
    return num < (float)n ? tab[(int)num] : 0.0f;
}

// rec = the cluster's record as analyzeClusters_NASP left it.  buf: 14 x 256 words.
__device__ __forceinline__ void weighted_pass(const NaspLaunch& a, const FramePtrs& f, int cluster_id, int tid, uint32_t (*buf)[256],
                                              const ClusterRecord& rec)
{
    const DaspGeom& g = a.g;
    const int rpx = g.wx * 2 / 16 + 1, rpy = g.wy * 2 / 16 + 1;
    const kde_superpixel m0 = rec.m;
    const kde_float3 spn = rec.spn;
    const float mr = (float)m0.r, mg = (float)m0.g, mb = (float)m0.b;
    int iv[1] = {0};                // npoints
    float fv[13];                   // r g b x y size X Y Z nx ny nz variance
#pragma unroll
    for (int k = 0; k < 13; k++) fv[k] = 0.0f;
    walk_members(g, f.labels, m0.x, m0.y, tid & 15, tid >> 4, rpx, rpy, cluster_id, [&](size_t q, int arx, int ary, int ox, int oy) {
        const float c0 = (float)f.bgr[q * 3], c1 = (float)f.bgr[q * 3 + 1], c2 = (float)f.bgr[q * 3 + 2];
        const float e0 = c0 - mr, e1 = c1 - mg, e2 = c2 - mb;
        const float color_diff = e0 * e0 + e1 * e1 + e2 * e2;
        const float color_filter = table_weight(a.ctab, a.ctab_n, color_diff);             // .cu:769
        const float dx = (float)ox, dy = (float)oy;      // = (float)(arounds.x - mean.x): the wrapped sum minus mean.x
        const float spatial_diff = dx * dx + dy * dy;
        const float spatial_filter = table_weight(a.stab, a.stab_n, spatial_diff);         // .cu:772
        fv[0] += clamp255(c0 * color_filter * spatial_filter);
        fv[1] += clamp255(c1 * color_filter * spatial_filter);
        fv[2] += clamp255(c2 * color_filter * spatial_filter);
        fv[3] += (float)arx * color_filter * spatial_filter;
        fv[4] += (float)ary * color_filter * spatial_filter;
        fv[5] += color_filter * spatial_filter;
        const kde_float3 pt = f.pts[q];
        const kde_float3 n = f.nrm[q];
        if (pt.z > 50.0f && ok3_or(n)) {
            float normal_diff = n.x * spn.x + n.y * spn.y + n.z * spn.z;
            normal_diff = normal_diff < 0.0f ? 0.0f : normal_diff;
            if (normal_diff > a.acos_thr) {                                                // .cu:805, NA3
                fv[6] += pt.x; fv[7] += pt.y; fv[8] += pt.z;
                fv[9] += n.x; fv[10] += n.y; fv[11] += n.z;
                fv[12] += normal_diff;
                iv[0] += 1;
            }
        }
    });
    tree256<1, 13>(tid, buf, iv, fv);
    const float size = fv[5];
    if (tid != 0 || !(size != 0.0f)) return;       // .cu:1001-1002 (a NaN sum is != 0)
    const int np = iv[0];
    const int mean_x = f2i_rz(fv[3] / size), mean_y = f2i_rz(fv[4] / size);
    int pix_x = mean_x, pix_y = mean_y;
    if (np != 0) {
        kde_float3 c;
        if (center_point(g, f.pts, pix_x, pix_y, &c)) {
            f.centers[cluster_id] = c;
        } else {
            c = mean3(fv[6], fv[7], fv[8], np);
            f.centers[cluster_id] = c;
            reproject_centre(c, a.intr, g.width, g.height, mean_x, mean_y, pix_x, pix_y);   // sic, .cu:1031
        }
        kde_float3 n = mean3(fv[9], fv[10], fv[11], np);
        const float len = sqrtf(n.x * n.x + n.y * n.y + n.z * n.z);
        n.x /= len;
        n.y /= len;
        n.z /= len;
        f.spn[cluster_id] = n;
        f.variance[cluster_id] = fv[12] / (float)np;
    } else {
        f.spn[cluster_id] = kde_float3{-1.0f, -1.0f, -1.0f};
        f.centers[cluster_id] = kde_float3{0.0f, 0.0f, 0.0f};
        f.variance[cluster_id] = 0.0f;
    }
    kde_superpixel m;
    m.r = channel_mean(f2i_rz(fv[0] / size));
    m.g = channel_mean(f2i_rz(fv[1] / size));
    m.b = channel_mean(f2i_rz(fv[2] / size));
    m.pad_ = 0;
    m.x = pix_x;
    m.y = pix_y;
    m.size = f2i_rz(size);                         // .cu:1064
    f.mean[cluster_id] = m;
}

// analyzeClusters_NASP and calculateWeightedAverage in one workgroup per cluster.  The weighted pass reads the record the
// first pass has just written (mean, normal): it is handed over through LDS, which keeps the reference's
// store-then-reload order without a trip through global memory, and the second walk finds the cluster's pixels in cache.
// (Measured against two launches: 1-4 % faster per Segmentation, EXPERIMENTS.md.)
__global__ __launch_bounds__(256) void nasp_cluster_kernel(NaspLaunch a)
{
    const ClusterWalk w = cluster_walk(a.g);
    const FramePtrs f = frame_ptrs(a, w.frame);
    const int cluster_id = w.cluster_id;
    const int tid = threadIdx.x;
    __shared__ uint32_t buf[14][256];
    __shared__ ClusterRecord s_rec;
    ClusterRecord rec;
    rec.m = f.mean[cluster_id];
    analyze_pass(a, f, cluster_id, tid, buf, rec.m, &rec);
    if (tid == 0) s_rec = rec;
    __syncthreads();            // also: the first wavefront has finished reading buf
    rec = s_rec;
    weighted_pass(a, f, cluster_id, tid, buf, rec);
}

}  // namespace

int launch_nasp_sample(const NaspLaunch& a, hipStream_t s)
{
    hipLaunchKernelGGL(nasp_sample_kernel, dim3(a.g.rows * a.g.cols, a.n), dim3(64), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

// initLD_NASP alone: what a Segmentation with iteration = 0 leaves in LD
int launch_nasp_init_ld(const NaspLaunch& a, hipStream_t s)
{
    const dim3 grid(ceil_div(a.g.width, 64), ceil_div(a.g.height, 4), a.n);
    hipLaunchKernelGGL(nasp_init_ld_kernel, grid, dim3(256), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

// first = the step right after sampleInitialClusters_NASP (initLD_NASP is folded in)
int launch_nasp_calc_ld(const NaspLaunch& a, bool first, hipStream_t s)
{
    const int nclusters = a.g.rows * a.g.cols;
    const bool lds = nclusters <= kNaspMaxLdsClusters;
    const size_t bytes = lds ? (size_t)nclusters * sizeof(NaspRec) : 0;
    const dim3 grid(ceil_div(a.g.width, 64), ceil_div(a.g.height, 4), a.n);
    if (first) {
        if (lds) hipLaunchKernelGGL((nasp_calc_ld_kernel<true, true>), grid, dim3(256), bytes, s, a);
        else hipLaunchKernelGGL((nasp_calc_ld_kernel<false, true>), grid, dim3(256), 0, s, a);
    } else {
        if (lds) hipLaunchKernelGGL((nasp_calc_ld_kernel<true, false>), grid, dim3(256), bytes, s, a);
        else hipLaunchKernelGGL((nasp_calc_ld_kernel<false, false>), grid, dim3(256), 0, s, a);
    }
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

// analyzeClusters_NASP followed by calculateWeightedAverage
int launch_nasp_clusters(const NaspLaunch& a, hipStream_t s)
{
    hipLaunchKernelGGL(nasp_cluster_kernel, dim3((unsigned)(a.g.rows * a.g.cols * a.n)), dim3(256), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
