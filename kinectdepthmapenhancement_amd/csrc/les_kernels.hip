// les_kernels.hip — LabelEquivalenceSeg::labelImage (superpixel merging into planes) on gfx950.
// Reference: LabelEquivalenceSeg/LabelEquivalenceSeg.cu:8-282 (6 kernels, 22 full-frame launches and 4 fills per call);
// definition and the deviations L1-L7 in DESIGN.md ("Superpixel merging").  Every output is bit-comparable with
// tools/les_ref.c, which states the same result per pixel and per round.
//
// Re-architecture vs the reference (DESIGN.md proves the invariant this rests on: under L1-L3 the merged label of a pixel
// is at every step a function of its superpixel label alone, and input_nd is per superpixel by construction):
//   les_edges_kernel   one streaming pass over the label image: exact pixel counts c_A (integer adds: a per-workgroup LDS
//                      histogram, one add per wavefront where the 64 labels agree, then one global add per touched
//                      entry) and the DIRECTED adjacency "some pixel of A has an L2-neighbour in B" as a bit matrix
//                      (idempotent ORs, one per run of boundary pixels; most lanes see A == B on all four sides).
//   les_graph_kernel   one workgroup per frame, tables in LDS: initLabel per superpixel, compNormal once per edge (the
//                      surviving bits are written back and the non-empty words listed), then the rounds on the listed
//                      words (scan = integer min per table entry; barrier; L3 phase 1; barrier; phase 2), countKernel's
//                      test, and the L4 sums, one thread per merged label walking its members in ascending label order.
//                      It leaves counts and adjacency zeroed for the next call (no fill launches).
//   les_paint_kernel   one streaming pass that writes the per-pixel merged label and (n, d) from the two tables.
// No float atomics anywhere.
#include "kde_internal.h"

namespace kde {
namespace {

constexpr int kEdgeThreads = 256, kEdgePixPerThread = 8;
constexpr int kGraphThreads = 1024;
constexpr int kPaintThreads = 256, kPaintPixPerThread = 4;

__device__ __forceinline__ bool in_table(int label, int nc) { return (unsigned)label < (unsigned)nc; }   // L1

// ---- counts and adjacency --------------------------------------------------------------------------------------------
// grid = (ceil(W*H / 2048), frames).  L2: up and left clamp to the pixel itself (no edge), the right neighbour is linear
// index p + 1 in every column (column W-1 sees (0, y+1)), the down neighbour of the last row and any index >= W*H
// contribute nothing.
// One OR per run of boundary pixels instead of one per pixel: the edge A -> B of pixel p through one of its four sides is
// left to the previous pixel of the run (`prev`: the pixel before p along the boundary, its neighbour on that side `prev_nb`)
// when that pixel carries the same pair; the first pixel of every run issues it.
__device__ __forceinline__ void add_edge(uint32_t* adj, int wpr, int nc, int A, int B, bool has_prev, int prev, int prev_nb)
{
    if (B == A || !in_table(B, nc)) return;
    if (has_prev && prev == A && prev_nb == B) return;
    atomicOr(adj + (size_t)A * wpr + (B >> 5), 1u << (B & 31));
}

__global__ __launch_bounds__(kEdgeThreads) void les_edges_kernel(LesLaunch a)
{
    __shared__ int hist[kLesMaxClusters];
    const int tid = threadIdx.x, lane = tid & 63, f = blockIdx.y;
    const int W = a.width, H = a.height, npix = W * H, nc = a.nc;
    const int32_t* labels = a.labels + (size_t)f * npix;
    uint32_t* adj = a.adj + (size_t)f * nc * a.wpr;
    for (int i = tid; i < nc; i += kEdgeThreads) hist[i] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * (kEdgeThreads * kEdgePixPerThread);
    for (int k = 0; k < kEdgePixPerThread; k++) {
        const long long pl = base + k * kEdgeThreads + tid;
        const bool inside = pl < npix;
        const int p = inside ? (int)pl : 0;
        const int A = inside ? labels[p] : -1;
        const bool ok = inside && in_table(A, nc);
        // c_A: one LDS add per wavefront when its valid lanes agree on the label (the usual case inside a superpixel)
        const int A0 = __builtin_amdgcn_readfirstlane(A);
        const uint64_t okm = __ballot(ok), same = __ballot(ok && A == A0);
        if (same == okm) {
            if (okm && lane == __ffsll((long long)same) - 1) atomicAdd(&hist[A0], __popcll(same));
        } else if (ok) {
            atomicAdd(&hist[A], 1);
        }
        if (ok) {
            const int y = p / W, x = p - y * W;
            const bool up = y >= 1, left = x >= 1, right = p + 1 < npix, down = y + 1 < H;
            const int lu = up ? labels[p - W] : -1, ll = left ? labels[p - 1] : -1;
            if (up) add_edge(adj, a.wpr, nc, A, lu, left, ll, left ? labels[p - 1 - W] : -1);
            if (left) add_edge(adj, a.wpr, nc, A, ll, up, lu, up ? labels[p - W - 1] : -1);
            if (right) add_edge(adj, a.wpr, nc, A, labels[p + 1], up, lu, up ? labels[p - W + 1] : -1);
            if (down) add_edge(adj, a.wpr, nc, A, labels[p + W], left, ll, left ? labels[p - 1 + W] : -1);
        }
    }
    __syncthreads();
    int32_t* count = a.count + (size_t)f * nc;
    for (int i = tid; i < nc; i += kEdgeThreads)
        if (hist[i]) atomicAdd(&count[i], hist[i]);
}

// ---- the graph step --------------------------------------------------------------------------------------------------
// compNormal (.cu:37-43) with L6
__device__ __forceinline__ bool comp_normal(const float4& p, const float4& q, float thr, float max_dist)
{
    const float d = (p.x * q.x + p.y * q.y) + p.z * q.z;
    return d < 1.0f && d > thr && fabsf(p.w - q.w) < max_dist;
}

__global__ __launch_bounds__(kGraphThreads) void les_graph_kernel(LesLaunch a)
{
    __shared__ float4 s_nd[kLesMaxClusters];     // input_nd per superpixel
    __shared__ int s_m[kLesMaxClusters];         // merged label per superpixel
    __shared__ int s_ref[kLesMaxClusters];       // ref[0 .. nc): entries >= nc are never lowered nor read (labels < nc)
    __shared__ int s_plab[kLesMaxClusters];      // label of the pixel with linear index l (L3's eligibility), later c_A
    __shared__ int s_listn;
    const int tid = threadIdx.x, f = blockIdx.x, nc = a.nc, wpr = a.wpr;
    const size_t fk = (size_t)f * nc;
    const kde_float3* normals = a.normals + fk;
    const kde_float3* centers = a.centers + fk;
    const int32_t* labels = a.labels + (size_t)f * a.width * a.height;
    uint32_t* adj = a.adj + fk * wpr;
    int32_t* list = a.list + fk * wpr;

    // initLabel (.cu:8-35) per superpixel; L1 is applied where pixels are read (a pixel's label outside the table is -1)
    for (int A = tid; A < nc; A += kGraphThreads) {
        const kde_float3 n = normals[A], c = centers[A];
        const bool valid = n.x != -1.0f || n.y != -1.0f || n.z != -1.0f;
        s_nd[A] = valid ? make_float4(n.x, n.y, n.z, fabsf((n.x * c.x + n.y * c.y) + n.z * c.z)) : make_float4(5.0f, 5.0f, 5.0f, 5.0f);
        s_m[A] = valid ? A : -1;
        s_ref[A] = A;
        s_plab[A] = labels[A];                   // nc <= W*H
    }
    if (tid == 0) s_listn = 0;
    __syncthreads();

    // compNormal once per directed edge: keep the bits getMin (.cu:63-66) can ever take.  merged > -1 is decided by
    // initLabel for good (phase 2 maps labels > -1 to table entries, which are >= 0).
    for (int idx = tid; idx < nc * wpr; idx += kGraphThreads) {
        const uint32_t bits = adj[idx];
        if (!bits) continue;
        const int A = idx / wpr, w = idx - A * wpr;
        uint32_t keep = 0;
        if (s_m[A] > -1) {
            const float4 ndA = s_nd[A];
            for (uint32_t rest = bits; rest; rest &= rest - 1) {
                const int b = __ffs((int)rest) - 1, B = w * 32 + b;
                if (s_m[B] > -1 && comp_normal(s_nd[B], ndA, a.thr, a.max_dist)) keep |= 1u << b;
            }
        }
        if (keep != bits) adj[idx] = keep;
        if (keep) list[atomicAdd(&s_listn, 1)] = idx;
    }
    __syncthreads();
    const int listn = s_listn;

    for (int round = 0; round < a.iterations; round++) {
        // scanKernel (.cu:70-109): ref[merged] = min(ref[merged], smallest merged label among the kept neighbours)
        for (int e = tid; e < listn; e += kGraphThreads) {
            const int idx = list[e];
            const int A = idx / wpr, w = idx - A * wpr;
            const int l1 = s_m[A];
            int l2 = l1;
            for (uint32_t rest = adj[idx]; rest; rest &= rest - 1) l2 = min(l2, s_m[w * 32 + __ffs((int)rest) - 1]);
            if (l2 < l1) atomicMin(&s_ref[l1], l2);
        }
        __syncthreads();
        // analysisKernel (.cu:110-136), L3 phase 1: entry l is flattened if the PIXEL with linear index l has merged == label.
        // Roots are not rewritten and chains strictly decrease, so following a chain through an entry another thread has
        // already flattened ends at the same root.
        for (int l = tid; l < nc; l += kGraphThreads) {
            const int B = s_plab[l];
            if (B == -1 || (in_table(B, nc) && s_m[B] == B)) {
                int current = s_ref[l];
                do {
                    current = s_ref[current];
                } while (current != s_ref[current]);
                s_ref[l] = current;
            }
        }
        __syncthreads();
        // L3 phase 2
        for (int A = tid; A < nc; A += kGraphThreads)
            if (s_m[A] > -1) s_m[A] = s_ref[s_m[A]];
        __syncthreads();
    }

    // countKernel's test (.cu:172-174 reads .y twice): a superpixel whose normal starts (-1, -1, .) loses its label (L7)
    int32_t* count = a.count + fk;
    int32_t* mfin = a.mfin + fk;
    for (int A = tid; A < nc; A += kGraphThreads) {
        const float4 nd = s_nd[A];
        if (s_m[A] > -1 && !(nd.x != -1.0f || nd.y != -1.0f || nd.y != -1.0f)) s_m[A] = -1;
        mfin[A] = s_m[A];
        s_plab[A] = count[A];
        count[A] = 0;                            // the scratch is all zero again when the call ends (see launch_les_label_image)
    }
    for (int e = tid; e < listn; e += kGraphThreads) adj[list[e]] = 0;   // every other word was stored as 0 above or never set
    __syncthreads();

    // countKernel + calculate_nd (.cu:162-226) under L4: one thread per merged label M, members in ascending label order,
    // (float)c_A * value added in that order starting from the first product (L5: nothing carried over)
    for (int M = tid; M < nc; M += kGraphThreads) {
        int size = 0;
        bool first = true;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, cx = 0.0f, cy = 0.0f, cz = 0.0f;
        for (int A = 0; A < nc; A++) {
            if (s_m[A] != M || s_plab[A] == 0) continue;
            const float c = (float)s_plab[A];
            const float4 nd = s_nd[A];
            const kde_float3 ctr = centers[A];
            size += s_plab[A];
            if (first) {
                nx = c * nd.x; ny = c * nd.y; nz = c * nd.z;
                cx = c * ctr.x; cy = c * ctr.y; cz = c * ctr.z;
                first = false;
            } else {
                nx = nx + c * nd.x; ny = ny + c * nd.y; nz = nz + c * nd.z;
                cx = cx + c * ctr.x; cy = cy + c * ctr.y; cz = cz + c * ctr.z;
            }
        }
        float4 mnd = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float var = 0.0f;
        bool vfirst = true;
        if (!first) {
            const float s = (float)size;
            mnd.x = nx / s; mnd.y = ny / s; mnd.z = nz / s;
            const float ox = cx / s, oy = cy / s, oz = cz / s;
            mnd.w = fabsf((mnd.x * ox + mnd.y * oy) + mnd.z * oz);
            for (int A = 0; A < nc; A++) {
                if (s_m[A] != M || s_plab[A] == 0) continue;
                const float4 nd = s_nd[A];
                float v = (nd.x * mnd.x + nd.y * mnd.y) + nd.z * mnd.z;
                v /= s;
                const float pv = (float)s_plab[A] * v;
                var = vfirst ? pv : var + pv;
                vfirst = false;
            }
        }
        a.mnd[fk + M] = mnd;
        a.variance[fk + M] = var;
        a.size[fk + M] = size;
    }
}

// ---- per-pixel outputs -----------------------------------------------------------------------------------------------
// grid = (ceil(W*H / 1024), frames).  L5: merged_nd is (0,0,0,0) where the merged label is -1.
__global__ __launch_bounds__(kPaintThreads) void les_paint_kernel(LesLaunch a)
{
    const int f = blockIdx.y, npix = a.width * a.height, nc = a.nc;
    const size_t fpx = (size_t)f * npix, fk = (size_t)f * nc;
    const long long base = (long long)blockIdx.x * (kPaintThreads * kPaintPixPerThread);
    for (int k = 0; k < kPaintPixPerThread; k++) {
        const long long p = base + k * kPaintThreads + threadIdx.x;
        if (p >= npix) return;
        const int A = a.labels[fpx + p];
        const int m = in_table(A, nc) ? a.mfin[fk + A] : -1;
        a.merged_label[fpx + p] = m;
        a.merged_nd[fpx + p] = m > -1 ? a.mnd[fk + m] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

}  // namespace

int launch_les_label_image(const LesLaunch& a, hipStream_t s)
{
    const long long npix = (long long)a.width * a.height;
    // Counts and adjacency are all zero on entry: zeroed at create, and the graph step clears what it has consumed (no
    // fill per call; the two share an allocation with nothing else, so whatever n and nc the previous call had, zero is
    // zero in every layout).
    hipLaunchKernelGGL(les_edges_kernel, dim3((unsigned)((npix + kEdgeThreads * kEdgePixPerThread - 1) / (kEdgeThreads * kEdgePixPerThread)), a.n),
                       dim3(kEdgeThreads), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(les_graph_kernel, dim3(a.n), dim3(kGraphThreads), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(les_paint_kernel, dim3((unsigned)((npix + kPaintThreads * kPaintPixPerThread - 1) / (kPaintThreads * kPaintPixPerThread)), a.n),
                       dim3(kPaintThreads), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
