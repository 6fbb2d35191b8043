// normal_kernels.hip — NormalMapGenerator::generateNormalMap (NormalEstimation/NormalMapGenerator.cu:397-411, 513-524) with
// its SmoothingAreaMapGenerator and IntegralImageGenerator stages, for any frame size, batched, with no host round trip.
//
//   CM:        N1 prep (DCI map + per-frame max of DDSA) -> N2 distance transform + final smoothing map
//              -> per chunk of frames: N3 row prefix sums, N4 column prefix sums, N5 covariance normal + rest normal
//   BILATERAL: N6 neighbour cross product (no DCI, DT or sums)
//
// Points come in millimetres and are scaled on the fly, v = p / 1000.0f per component (:505-511); the reference's
// verticeMap copy is never materialised.  Semantics (definitions N1, N2, the DT quirks) are in DESIGN.md, "Normal
// estimation"; tools/normals_ref.c restates them on the CPU.
#include "kde_internal.h"

#include <cfloat>

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kBandRows = 64;            // N2: output rows per workgroup
constexpr float kDtCapC = 47.0f;         // N2: frames whose largest DDSA exceeds this take the uncapped path

__device__ __forceinline__ kde_float3 metres(kde_float3 p) { return {p.x / 1000.0f, p.y / 1000.0f, p.z / 1000.0f}; }

// N1: a neighbour outside [0, W*H) of the frame reads the point (0,0,0)
__device__ __forceinline__ kde_float3 rd(const kde_float3* f, long long npx, long long i)
{
    if (i < 0 || i >= npx) return {0.0f, 0.0f, 0.0f};
    return metres(f[i]);
}

__device__ __forceinline__ float zm(const kde_float3* f, long long npx, long long i)
{
    return (i < 0 || i >= npx) ? 0.0f : f[i].z / 1000.0f;
}

// float <-> int key whose signed order is the float order (for atomicMax)
__device__ __forceinline__ int f2key(float x)
{
    const int i = __float_as_int(x);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __forceinline__ float key2f(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

// SmoothingAreaMapGenerator.cu:12-31, one thread's tests
__device__ __forceinline__ bool fires(const kde_float3* f, long long npx, long long j, long long step, float fac)
{
    if (j < 0 || j >= npx) return false;
    const float zc = f[j].z / 1000.0f, zn = zm(f, npx, j + step);
    const float thr = (fac * (fabsf(zc) + 1.0f)) * 2.0f;
    return fabsf(zc - zn) > thr || zc == 0.0f || zn == 0.0f;
}

// ---- N1: DCI (definition N1) and C = max DDSA per frame ------------------------------------------------------------
// grid (ceil(W*H / 256), n)
__global__ __launch_bounds__(kThreads) void normals_prep_kernel(const kde_float3* __restrict__ pts, int W, int H, float fac,
                                                                float s, uint8_t* __restrict__ dci, int* __restrict__ cmax)
{
    const long long npx = (long long)W * H;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const kde_float3* f = pts + (size_t)blockIdx.y * npx;
    int key = INT_MIN;
    if (i < npx) {
        const bool zero = fires(f, npx, i, 1, fac) || fires(f, npx, i, W, fac) || fires(f, npx, i - 1, 1, fac) ||
                          fires(f, npx, i - W, W, fac);
        dci[(size_t)blockIdx.y * npx + i] = zero ? 0 : 255;
        key = f2key(s + (f[i].z / 1000.0f) / 10.0f);
    }
    for (int o = 32; o >= 1; o >>= 1) key = max(key, __shfl_xor(key, o));
    if ((threadIdx.x & 63) == 0 && key != INT_MIN) atomicMax(cmax + blockIdx.y, key);
}

// ---- N2: distance transform (SmoothingAreaMapGenerator.cu:40-92) and FS (:95-122) ----------------------------------
// The forward pass is the float recurrence T[r][c] = min(T0[r][c], ul, u, ur, T[r][c-1] + 1.0f) over rows 1..H-1 and
// columns 1..W-1, serial in both directions.  It is evaluated exactly, in parallel, from three facts:
//  * x -> fl(x + 1.0f) and x -> fl(x + 1.4f) are monotone, so clamping every T0 at C commutes with the recurrence:
//    min(T, C) of the clamped run equals min(T, C) of the original;
//  * with C = the frame's largest DDSA, FS = (T < DDSA ? T : DDSA) is the same for T and min(T, C);
//  * each step adds at least 1 (fl(x + 1) >= k + 1 for x >= k, k integral), so a chain of K = ceil(C) + 1 steps from any
//    value >= 0 exceeds C.  With the clamp, T[r][c] depends only on the K rows above and the K columns to its left.
// So a workgroup owns kBandRows output rows and starts K rows earlier from the initial map (any start value >= the
// true one is harmless after K rows), and each lane owns a run of columns of a row and starts K columns to its left
// from C.  C < 0 clamps everything to C, which is exact too.  A frame with C > kDtCapC (a far outlier) is done by its
// first workgroup alone with no warm-up limit: rows from 1 and every lane's scan from column 1 -- the serial order.
// The backward pass never advances its row pointers (:75-91): all H-1 sweeps sweep row H-2 against row H-1, and
// after one sweep T[c] <= min(lower terms, T[c+1] + 1) holds at every c, so the repeats change nothing.  The
// workgroup that owns row H-1 sweeps once, right to left, with the same lane warm-up; it also owns FS of row H-2.
// grid (ceil(H / kBandRows), n); scratch: two rows of W floats per workgroup.
__global__ __launch_bounds__(kThreads) void normals_dt_kernel(const kde_float3* __restrict__ pts, const uint8_t* __restrict__ dci,
                                                              const int* __restrict__ cmax, int W, int H, float s,
                                                              float* __restrict__ scratch, float* __restrict__ fs)
{
    const long long npx = (long long)W * H;
    const size_t base = (size_t)blockIdx.y * npx;
    const kde_float3* f = pts + base;
    const uint8_t* d = dci + base;
    float* out = fs + base;
    const float C = key2f(cmax[blockIdx.y]);
    const float big = (float)(W + H);
    const bool capped = C <= kDtCapC;
    long long K;
    int R0, R1;
    if (capped) {
        K = C <= 0.0f ? 1 : (long long)ceilf(C) + 1;
        R0 = blockIdx.x * kBandRows;
        R1 = min(H, R0 + kBandRows);
    } else {
        if (blockIdx.x != 0) return;
        K = 1ll << 40;
        R0 = 0;
        R1 = H;
    }
    const bool owns_last = R1 == H;
    float* prev = scratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * W;
    float* cur = prev + W;
    auto t0 = [&](long long r, long long c) { return fminf(d[r * W + c] ? big : 0.0f, C); };
    auto put = [&](long long r, long long c, float t) {
        const float ddsa = s + (f[r * W + c].z / 1000.0f) / 10.0f;
        out[r * W + c] = t < ddsa ? t : ddsa;
    };
    long long rx = R0;                                      // first row that must come out exact
    if (owns_last && H >= 2 && H - 2 < rx) rx = H - 2;
    const long long rs = rx - K > 1 ? rx - K : 1;
    for (long long c = threadIdx.x; c < W; c += kThreads) {
        prev[c] = t0(rs - 1, c);
        if (rs - 1 == 0 && R0 == 0 && H != 2) put(0, c, prev[c]);   // row 0 never changes
    }
    __syncthreads();

    // forward pass: lane l owns columns [cs, ce) of 1..W-1
    const long long L = (W - 1 + kThreads - 1) / kThreads;
    const long long cs = 1 + threadIdx.x * L, ce = min((long long)W, cs + L);
    for (long long r = rs; r < R1; ++r) {
        const bool write = r >= R0 && r != H - 2;
        const float col0 = t0(r, 0);                         // column 0 never changes; it is also upRight at c = W-1
        if (cs < W) {
            const long long c_begin = cs - K > 1 ? cs - K : 1;
            float t = c_begin == 1 ? col0 : C;
            float pl = prev[c_begin - 1], pc = prev[c_begin];
            for (long long c = c_begin; c < ce; ++c) {
                const float pr = c + 1 < W ? prev[c + 1] : col0;
                const float upLeft = pl + 1.4f, up = pc + 1.0f, upRight = pr + 1.4f, left = t + 1.0f;
                const float a = upLeft < up ? upLeft : up;
                const float b = left < upRight ? left : upRight;
                const float m = a < b ? a : b;
                const float center = t0(r, c);
                t = m < center ? m : center;
                if (c >= cs) {
                    cur[c] = t;
                    if (write) put(r, c, t);
                }
                pl = pc;
                pc = pr;
            }
        }
        if (threadIdx.x == 0) {
            cur[0] = col0;
            if (write) put(r, 0, col0);
        }
        __syncthreads();
        float* tmp = prev;
        prev = cur;
        cur = tmp;
    }
    // now prev = row H-1 and cur = row H-2 (forward values) in the workgroup that owns row H-1
    if (!owns_last || H < 2) return;
    const float* next = prev;
    const float* row = cur;
    const long long r = H - 2;
    // backward sweep: lane l owns columns [bs, be) of 0..W-2, scanned right to left from be - 1 + K
    const long long bs = threadIdx.x * L, be = min((long long)W - 1, bs + L);
    if (bs < W - 1) {
        const long long c_begin = be - 1 + K < W - 2 ? be - 1 + K : W - 2;
        float t = c_begin == W - 2 ? row[W - 1] : C;
        for (long long c = c_begin; c >= bs; --c) {
            const float lowerLeft = (c >= 1 ? next[c - 1] : row[W - 1]) + 1.4f;   // next_row[-1] is current_row[W-1]
            const float lower = next[c] + 1.0f, lowerRight = next[c + 1] + 1.4f, right = t + 1.0f;
            const float a = lowerLeft < lower ? lowerLeft : lower;
            const float b = right < lowerRight ? right : lowerRight;
            const float m = a < b ? a : b;
            const float center = row[c];
            t = m < center ? m : center;
            if (c < be) put(r, c, t);
        }
    }
    if (threadIdx.x == 0) put(r, W - 1, row[W - 1]);
}

// ---- N3 / N4: inclusive integral images (IntegralImageGenerator.cu) -------------------------------------------------
// The count of z != 0 (exact, uint32) and x, y, z, xx, xy, xz, yy, yz, zz in double, each float widened before the
// product (:102-110, 330-343).  Summed along each row from column 0, then down each column: the order of the CPU
// checker, so window sums are bit-identical to it.  Planes: [channel][frame][H][W].
__device__ __forceinline__ double channel_value(kde_float3 v, int ch)
{
    const double x = v.x, y = v.y, z = v.z;
    switch (ch) {
    case 0: return x;
    case 1: return y;
    case 2: return z;
    case 3: return x * x;
    case 4: return x * y;
    case 5: return x * z;
    case 6: return y * y;
    case 7: return y * z;
    default: return z * z;
    }
}

// one thread per (channel, frame, row); channel 9 is the count
__global__ __launch_bounds__(kThreads) void normals_rowscan_kernel(const kde_float3* __restrict__ pts, int W, int H, int nf,
                                                                   uint32_t* __restrict__ cnt, double* __restrict__ sums)
{
    const long long rows = (long long)nf * H;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= rows * 10) return;
    const int ch = (int)(t / rows);
    const long long fr_row = t - ch * rows;
    const size_t off = (size_t)fr_row * W;
    const kde_float3* p = pts + off;
    if (ch == 9) {
        uint32_t acc = 0;
        for (int c = 0; c < W; ++c) {
            acc += p[c].z / 1000.0f != 0.0f ? 1u : 0u;
            cnt[off + c] = acc;
        }
        return;
    }
    double* o = sums + (size_t)ch * rows * W + off;
    double acc = 0.0;
    for (int c = 0; c < W; ++c) {
        const double v = channel_value(metres(p[c]), ch);
        acc = c == 0 ? v : acc + v;
        o[c] = acc;
    }
}

// one thread per (channel, frame, column): I[r][c] = I[r-1][c] + I[r][c], in place
__global__ __launch_bounds__(kThreads) void normals_colscan_kernel(int W, int H, int nf, uint32_t* __restrict__ cnt,
                                                                   double* __restrict__ sums)
{
    const long long cols = (long long)nf * W;
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= cols * 10) return;
    const int ch = (int)(t / cols);
    const long long fc = t - ch * cols;
    const long long fr = fc / W, c = fc - fr * W;
    const size_t off = (size_t)fr * H * W + c;
    if (ch == 9) {
        uint32_t* p = cnt + off;
        for (int r = 1; r < H; ++r) p[(size_t)r * W] = p[(size_t)(r - 1) * W] + p[(size_t)r * W];
        return;
    }
    double* p = sums + (size_t)ch * nf * H * W + off;
    for (int r = 1; r < H; ++r) p[(size_t)r * W] = p[(size_t)(r - 1) * W] + p[(size_t)r * W];
}

// ---- N5: covariance normal (NormalMapGenerator.cu:135-302) + rest normal (:304-354) ---------------------------------
__device__ void roots2(double b, double c, double* r)
{
    r[0] = 0.0f;
    double d = (b * b - 4.0f * c);
    if (d < 0.0) d = 0.0f;
    const double sd = sqrt(d);
    r[2] = 0.5f * (b + sd);
    r[1] = 0.5f * (b - sd);
}

__device__ void roots3(const double* m, double* r)
{
    const double c0 = m[0] * m[4] * m[8] + 2.0f * m[1] * m[2] * m[5] - m[0] * m[5] * m[5] - m[4] * m[2] * m[2] -
                      m[8] * m[1] * m[1];
    const double c1 = m[0] * m[4] - m[1] * m[1] + m[0] * m[8] - m[2] * m[2] + m[4] * m[8] - m[5] * m[5];
    const double c2 = m[0] + m[4] + m[8];
    if (fabs(c0) < FLT_EPSILON) {
        roots2(c2, c1, r);
        return;
    }
    // the reference's float-typed constants: 1.0f/3.0f and sqrt(3.0f) evaluated in float, then widened
    const double s_inv3 = (double)(1.0f / 3.0f);
    const double s_sqrt3 = (double)sqrtf(3.0f);
    const double c2_over_3 = c2 * s_inv3;
    double a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.0) a_over_3 = 0.0f;
    const double half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
    double q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.0) q = 0.0f;
    const double rho = sqrt(-a_over_3);
    const double theta = atan2(sqrt(-q), half_b) * s_inv3;
    const double cos_theta = cos(theta);
    const double sin_theta = sin(theta);
    r[0] = c2_over_3 + 2.0f * rho * cos_theta;
    r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
    double t;
    if (r[0] >= r[1]) t = r[1], r[1] = r[0], r[0] = t;
    if (r[1] >= r[2]) {
        t = r[2], r[2] = r[1], r[1] = t;
        if (r[0] >= r[1]) t = r[1], r[1] = r[0], r[0] = t;
    }
    if (r[0] <= 0) roots2(c2, c1, r);
}

__device__ void eigen_vector(const double* m, double* vec)
{
    double sm[9];
    double scale = -100.0;
    for (int i = 0; i < 9; ++i) {
        const double t = fabs(m[i]);
        if (t > scale) scale = t;
    }
    if (scale <= DBL_MIN) scale = 1.0;
    for (int i = 0; i < 9; ++i) sm[i] = m[i] / scale;
    double r[3];
    roots3(sm, r);
    sm[0] -= r[0], sm[4] -= r[0], sm[8] -= r[0];
    const double v1[3] = {sm[1] * sm[5] - sm[2] * sm[4], sm[2] * sm[3] - sm[0] * sm[5], sm[0] * sm[4] - sm[1] * sm[3]};
    const double v2[3] = {sm[1] * sm[8] - sm[2] * sm[7], sm[2] * sm[6] - sm[0] * sm[8], sm[0] * sm[7] - sm[1] * sm[6]};
    const double v3[3] = {sm[4] * sm[8] - sm[5] * sm[7], sm[5] * sm[6] - sm[3] * sm[8], sm[3] * sm[7] - sm[4] * sm[6]};
    const double l1 = sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2]);
    const double l2 = sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]);
    const double l3 = sqrt(v3[0] * v3[0] + v3[1] * v3[1] + v3[2] * v3[2]);
    const double* pv;
    double l;
    if (l1 >= l2 && l1 >= l3) pv = v1, l = l1;
    else if (l2 >= l1 && l2 >= l3) pv = v2, l = l2;
    else pv = v3, l = l3;
    vec[0] = pv[0] / l;
    vec[1] = pv[1] / l;
    vec[2] = pv[2] / l;
}

// the neighbour cross product of computeRestNormalGPU (rest = true: with the d_h / d_v test) and
// computeNormalBilateralGPU; writes n only where the reference does.  pow(a, 2) is a * a (precedent Q9).
__device__ __forceinline__ void cross_normal(const kde_float3* f, long long npx, int W, long long i, bool rest, float* n)
{
    const int r = zm(f, npx, i + 1) == 0.0f ? -1 : 1;
    const kde_float3 c = metres(f[i]);
    const kde_float3 ph01 = rd(f, npx, i + r), ph02 = c, pv01 = rd(f, npx, i + (long long)r * W), pv02 = c;
    const float vhx = ph01.x - ph02.x, vhy = ph01.y - ph02.y, vhz = ph01.z - ph02.z;
    const float vvx = pv01.x - pv02.x, vvy = pv01.y - pv02.y, vvz = pv01.z - pv02.z;
    bool ok = ph02.z != 0.0f;
    if (rest) {
        const float ax = ph01.x - c.x, ay = ph01.y - c.y, az = ph01.z - c.z;
        const float bx = pv01.x - c.x, by = pv01.y - c.y, bz = pv01.z - c.z;
        const float d_h = sqrtf(ax * ax + ay * ay + az * az);
        const float d_v = sqrtf(bx * bx + by * by + bz * bz);
        ok = ok && d_h < c.z * 0.01f && d_v < c.z * 0.01f;
    }
    if (ok) {
        n[0] = vhz * vvy - vhy * vvz;
        n[1] = -(vhx * vvz - vhz * vvx);
        n[2] = vhy * vvx - vhx * vvy;
        const float norm = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (norm > 0.0f) n[0] /= -norm, n[1] /= -norm, n[2] /= -norm;
    }
}

__device__ __forceinline__ double corner(const double* p, int W, int r, int c) { return (r < 0 || c < 0) ? 0.0 : p[(size_t)r * W + c]; }
__device__ __forceinline__ uint32_t corner(const uint32_t* p, int W, int r, int c) { return (r < 0 || c < 0) ? 0u : p[(size_t)r * W + c]; }

// grid (ceil(W*H / 256), nf): the frames of one chunk; pts / fs / out point at the chunk's first frame
__global__ __launch_bounds__(kThreads) void normals_cm_kernel(const kde_float3* __restrict__ pts, const float* __restrict__ fs,
                                                              const uint32_t* __restrict__ cnt, const double* __restrict__ sums,
                                                              int W, int H, int border, kde_float3* __restrict__ out)
{
    const long long npx = (long long)W * H;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= npx) return;
    const int nf = gridDim.y;
    const size_t base = (size_t)blockIdx.y * npx;
    const kde_float3* f = pts + base;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    float n[3] = {-1.0f, -1.0f, -1.0f};
    const float sm = fs[base + i];
    // computeNormalCM_GPU: border, FS <= 2, N2 (a window that leaves the frame), cont == 0 are bad points
    if (!(x <= border || x >= W - border || y <= border || y >= H - border) && sm > 2.0f && (double)sm < 2147483647.0) {
        const int rw = (int)sm, r2 = rw >> 1;
        const long long c0 = (long long)x - r2, c1 = c0 - 1 + rw, r0 = (long long)y - r2, r1 = r0 - 1 + rw;
        if (c0 >= 0 && r0 >= 0 && c1 <= W - 1 && r1 <= H - 1) {
            const int u = (int)c0 - 1, v = (int)r0 - 1, ue = (int)c1, ve = (int)r1;
            const uint32_t* pc = cnt + base;
            const unsigned cont = corner(pc, W, ve, ue) + corner(pc, W, v, u) - corner(pc, W, ve, u) - corner(pc, W, v, ue);
            if (cont != 0) {
                double S[9];
                for (int k = 0; k < 9; ++k) {
                    const double* p = sums + (size_t)k * nf * npx + base;
                    S[k] = corner(p, W, ve, ue) + corner(p, W, v, u) - corner(p, W, ve, u) - corner(p, W, v, ue);
                }
                const double dc = (double)cont;
                double m[9];
                m[0] = S[3] - (S[0] * S[0] / dc);
                m[1] = m[3] = S[4] - (S[0] * S[1] / dc);
                m[2] = m[6] = S[5] - (S[0] * S[2] / dc);
                m[4] = S[6] - (S[1] * S[1] / dc);
                m[5] = m[7] = S[7] - (S[1] * S[2] / dc);
                m[8] = S[8] - (S[2] * S[2] / dc);
                double e[3];
                eigen_vector(m, e);
                if (e[2] < 0.0f) n[0] = (float)e[0], n[1] = (float)-e[1], n[2] = (float)e[2];
                else n[0] = (float)-e[0], n[1] = (float)e[1], n[2] = (float)-e[2];
            }
        }
    }
    // computeRestNormalGPU: bad points get the neighbour normal, then every non-bad normal has x and z negated
    const bool bad = n[0] == -1.0f && n[1] == -1.0f && n[2] == -1.0f;
    if (bad) cross_normal(f, npx, W, i, true, n);
    if (!(n[0] == -1.0f && n[1] == -1.0f && n[2] == -1.0f)) {
        n[0] *= -1.0f;
        n[2] *= -1.0f;
    }
    out[base + i] = {n[0], n[1], n[2]};
}

// ---- N6: computeNormalBilateralGPU (:355-395) --------------------------------------------------------------------
// grid (ceil(W*H / 256), n)
__global__ __launch_bounds__(kThreads) void normals_bilateral_kernel(const kde_float3* __restrict__ pts, int W, int H,
                                                                     kde_float3* __restrict__ out)
{
    const long long npx = (long long)W * H;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= npx) return;
    const size_t base = (size_t)blockIdx.y * npx;
    const kde_float3* f = pts + base;
    float n[3] = {-1.0f, -1.0f, -1.0f};
    if (f[i].z / 1000.0f != 0.0f) {
        cross_normal(f, npx, W, i, false, n);
        n[0] *= -1.0f;
        n[2] *= -1.0f;
    }
    out[base + i] = {n[0], n[1], n[2]};
}

inline unsigned blocks_for(long long items) { return (unsigned)((items + kThreads - 1) / kThreads); }

}  // namespace

int normals_dt_bands(int height) { return ceil_div(height, kBandRows); }

// frames per pass of N3-N5: the integral images (76 B per pixel) of at most 2^22 pixels, at least one frame
int normals_chunk_frames(int width, int height, int max_batch)
{
    const long long per = (long long)width * height;
    long long c = ((long long)1 << 22) / per;
    if (c < 1) c = 1;
    if (c > max_batch) c = max_batch;
    return (int)c;
}

int launch_normals(const NormalsLaunch& a, hipStream_t s)
{
    const long long npx = (long long)a.width * a.height;
    const unsigned gx = blocks_for(npx);
    if (a.method == KDE_NORMALS_BILATERAL) {
        normals_bilateral_kernel<<<dim3(gx, a.n), kThreads, 0, s>>>(a.pts, a.width, a.height, a.out);
        KDE_HIP_TRY(hipGetLastError());
        return KDE_OK;
    }
    KDE_HIP_TRY(hipMemsetAsync(a.cmax, 0x80, sizeof(int) * a.n, s));   // 0x80808080: below every DDSA's key
    normals_prep_kernel<<<dim3(gx, a.n), kThreads, 0, s>>>(a.pts, a.width, a.height, a.factor, a.smoothing, a.dci, a.cmax);
    KDE_HIP_TRY(hipGetLastError());
    normals_dt_kernel<<<dim3(normals_dt_bands(a.height), a.n), kThreads, 0, s>>>(a.pts, a.dci, a.cmax, a.width, a.height,
                                                                                 a.smoothing, a.dt_scratch, a.fs);
    KDE_HIP_TRY(hipGetLastError());
    const int border = (int)a.smoothing;   // NormalMapGenerator.cu:404
    for (int f0 = 0; f0 < a.n; f0 += a.chunk_frames) {
        const int nf = a.n - f0 < a.chunk_frames ? a.n - f0 : a.chunk_frames;
        const size_t off = (size_t)f0 * npx;
        normals_rowscan_kernel<<<blocks_for((long long)nf * a.height * 10), kThreads, 0, s>>>(a.pts + off, a.width, a.height,
                                                                                             nf, a.cnt, a.sums);
        KDE_HIP_TRY(hipGetLastError());
        normals_colscan_kernel<<<blocks_for((long long)nf * a.width * 10), kThreads, 0, s>>>(a.width, a.height, nf, a.cnt,
                                                                                            a.sums);
        KDE_HIP_TRY(hipGetLastError());
        normals_cm_kernel<<<dim3(gx, nf), kThreads, 0, s>>>(a.pts + off, a.fs + off, a.cnt, a.sums, a.width, a.height,
                                                            border, a.out + off);
        KDE_HIP_TRY(hipGetLastError());
    }
    return KDE_OK;
}

}  // namespace kde
