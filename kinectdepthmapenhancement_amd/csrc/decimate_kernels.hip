// decimate_kernels.hip — DepthDecimation: n depth frames (and, in a call of its own, their BGR guides) made k times smaller each
// way, k = 2 .. 8: an output pixel is the lower median, or the guarded mean, of the valid samples of its k x k block, the guide
// the rounded mean of the block's colours.  The reference has no such step: every class of it runs at the size it is given.
//   D1 decimate  a workgroup takes a tile of 32 x TH output pixels (TH = 8 for k <= 4, 4 above: 256 or 128 threads), a thread
//                one pixel.  The tile's 32k x TH*k source samples are read once, row by row, as the aligned 16-byte pieces
//                that lie inside a row's part of the tile -- whatever the alignment of the frame and of its rows -- and as
//                elements at a row's two ends; four loads of a thread are issued before the first is used.  A piece lands in
//                LDS as floats, 0 where the sample is not z > z_min && z < z_max (a valid depth is > z_min >= 0, so 0 means
//                absent), at the place that keeps its alignment: row r starts `off` elements into its LDS row, off = the
//                elements between the 16-byte boundary below the row's first sample and that sample, so every piece is one
//                16- or 32-byte LDS write.  A tile that reaches over the frame's right or bottom edge is zeroed first: what
//                does not exist is absent.  No thread loads from global memory with a stride.
//                A thread then reads its block from LDS (k = 3, 5, 6, 7, where a block never lines up with a piece, regroup
//                here), counts the valid samples, takes their smallest and largest bit pattern -- positive finite floats
//                order as their uint32 bits -- and selects the lower median in registers: Batcher's odd-even merge sort of
//                the bit patterns, absent samples as 0xffffffff, the block padded to a power of two with constants the
//                compiler folds away; sorted[(m - 1) / 2] by a select chain.  No spill (26 .. 83 registers for k = 2 .. 8).
//                A most-significant-bit-first radix select was built beside it and took 1.1 to 2 times as long at every
//                k (EXPERIMENTS.md has the table); it is gone.
//                The mean reads the block again from LDS in tap order.  Fast paths, same bytes: the mean without a guard never
//                selects; with the guard a wavefront selects only if one of its blocks spans more than max_gap, since
//                |z - zmed| <= zmax - zmin for every valid z.
//                Filled and mixed pixels are counted per workgroup and written, not added, to partial[frame][workgroup].
//   D2 count     filled[f], mixed[f] = the sums of partial[f][*], one workgroup per frame: no atomic, no reset, every call
//                writes every count it reports (kernel nodes keep their order in a replayed graph; a memset node did not)
//   D3 colour    the same tiling and the same loads for the guide: bytes into LDS, a thread sums its block per channel
// Bounds.  A row's part of a tile is the byte range [b0, b1) inside the frame; a 16-byte load is issued only where
// b0 <= address and address + 16 <= b1, an element load only inside [b0, b1).  LDS row r holds off + 32k elements with
// off <= 15 / element size, inside its stride of 32k + 8 (32k * 3 + 16 bytes for the guide).
// The rule is stated in kde_hip.h.  Every output pixel is a function of its own block and the counts are integer sums: the
// same bytes for any n, place in the batch and alignment.
#include "kde_internal.h"
#include "kde_device_math.h"

namespace kde {
namespace {

constexpr int kTileW = 32;
constexpr int kAhead = 4;                       // the loads a thread issues before it uses the first
constexpr int tile_h(int k) { return k <= 4 ? 8 : 4; }
constexpr int pow2_at_least(int n) { return n <= 1 ? 1 : 2 * pow2_at_least((n + 1) / 2); }

typedef uint32_t u_v4 __attribute__((ext_vector_type(4)));
typedef float f_v4 __attribute__((ext_vector_type(4)));

// ---- Batcher's odd-even merge sort of N2 = 2^q values as a list of compare-exchanges -----------------------------------
template <int N2>
struct Network {
    static constexpr int kMax = N2 * 9 + 1;     // 543 exchanges for 64, 191 for 32, 63 for 16, 19 for 8, 5 for 4
    short a[kMax], b[kMax];
    int count;
    constexpr Network() : a{}, b{}, count(0)
    {
        for (int p = 1; p < N2; p <<= 1)
            for (int k = p; k >= 1; k >>= 1)
                for (int j = k % p; j + k < N2; j += 2 * k)
                    for (int i = 0; i < k && i + j + k < N2; i++)
                        if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                            a[count] = (short)(i + j);
                            b[count] = (short)(i + j + k);
                            count++;
                        }
    }
};

// v[0 .. N) sorted ascending as far as the lower median needs; t = (m - 1) / 2 <= (N - 1) / 2
template <int N>
__device__ __forceinline__ uint32_t select_network(const uint32_t (&v)[N], int t)
{
    constexpr int N2 = pow2_at_least(N);
    constexpr Network<N2> net{};
    uint32_t s[N2];
#pragma unroll
    for (int i = 0; i < N2; i++) s[i] = i < N ? v[i] : 0xffffffffu;
#pragma unroll
    for (int c = 0; c < net.count; c++) {
        const uint32_t lo = min(s[net.a[c]], s[net.b[c]]), hi = max(s[net.a[c]], s[net.b[c]]);
        s[net.a[c]] = lo;
        s[net.b[c]] = hi;
    }
    uint32_t r = s[0];
#pragma unroll
    for (int i = 1; i <= (N - 1) / 2; i++) r = t == i ? s[i] : r;
    return r;
}

// ---- staging: the tile's part of `rows` source rows into LDS ----------------------------------------------------------------
// Row r of the tile is the bytes [b0, b1) = row_bytes(r) .. + cols * E; piece c of it is the 16 bytes at (b0 & ~15) + 16c.
// PIECES: the pieces a full tile row can touch at any alignment.  put(r, first_element_of_the_piece, the 16 bytes) stores a
// whole piece, put1(r, element, address) one element; both get the element's index counted from the 16-byte boundary below b0.
template <int THREADS, int E, int ROW_ELEMS, class Put, class Put1>
__device__ __forceinline__ void stage_rows(const char* tile0, size_t row_pitch, int cols, int rows, Put put, Put1 put1)
{
    constexpr int PIECES = ROW_ELEMS * E / 16 + 1;
    static_assert((ROW_ELEMS * E) % 16 == 0, "a full tile row is a whole number of pieces");
    const int total = rows * PIECES;
    for (int base = (int)threadIdx.x; base < total; base += THREADS * kAhead) {
        u_v4 q[kAhead];
        int kind[kAhead];                               // 0 nothing, 1 a whole piece (loaded), 2 an end of the row
#pragma unroll
        for (int u = 0; u < kAhead; u++) {
            const int idx = base + u * THREADS;
            kind[u] = 0;
            q[u] = u_v4{0u, 0u, 0u, 0u};
            if (idx < total) {
                const int r = idx / PIECES, c = idx - r * PIECES;
                const uintptr_t b0 = reinterpret_cast<uintptr_t>(tile0) + (size_t)r * row_pitch, b1 = b0 + (size_t)cols * E;
                const uintptr_t at = (b0 & ~(uintptr_t)15) + 16u * (unsigned)c;
                if (at >= b0 && at + 16 <= b1) {
                    q[u] = *reinterpret_cast<const u_v4*>(at);
                    kind[u] = 1;
                } else if (at < b1 && at + 16 > b0) {
                    kind[u] = 2;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kAhead; u++) {
            const int idx = base + u * THREADS;
            const int r = idx / PIECES, c = idx - r * PIECES;
            if (kind[u] == 1) {
                put(r, c * (16 / E), q[u]);
            } else if (kind[u] == 2) {
                const uintptr_t b0 = reinterpret_cast<uintptr_t>(tile0) + (size_t)r * row_pitch, b1 = b0 + (size_t)cols * E;
                const uintptr_t floor0 = b0 & ~(uintptr_t)15, at = floor0 + 16u * (unsigned)c;
                const uintptr_t lo = at > b0 ? at : b0, hi = at + 16 < b1 ? at + 16 : b1;
                for (uintptr_t p = lo; p < hi; p += E) put1(r, (int)((p - floor0) / E), p);
            }
        }
    }
}

// D1: grid (tiles, n), block 32 * tile_h(K)
template <int K>
__global__ __launch_bounds__(kTileW * tile_h(K)) void decimate_kernel(DecimateLaunch L)
{
    constexpr int TH = tile_h(K), THREADS = kTileW * TH, COLS = kTileW * K, ROWS = TH * K, N = K * K;
    constexpr int STRIDE = COLS + 8;                        // off <= 7 elements in front of a row
    __shared__ __attribute__((aligned(32))) float s_z[ROWS * STRIDE];
    __shared__ uint32_t s_count[THREADS / 64];
    const int tid = (int)threadIdx.x, lx = tid & (kTileW - 1), ly = tid >> 5;
    const unsigned frame = blockIdx.y;
    const int tiles_x = (L.ow + kTileW - 1) / kTileW;
    const int trow = (int)blockIdx.x / tiles_x, tcol = (int)blockIdx.x - trow * tiles_x;
    const int i0 = tcol * kTileW, j0 = trow * TH;           // i0 < ow and j0 < oh: x0 < sw and y0 < sh
    const int x0 = i0 * K, y0 = j0 * K;
    const int cols = min(COLS, L.sw - x0), rows = min(ROWS, L.sh - y0);
    const bool in_f32 = L.depth_format == KDE_DEPTH_F32, out_f32 = L.out_format == KDE_DEPTH_F32;
    const size_t spx = (size_t)L.sw * L.sh, opx = (size_t)L.ow * L.oh;
    const size_t esz = in_f32 ? sizeof(float) : sizeof(uint16_t);
    const char* sframe = static_cast<const char*>(L.depth) + (size_t)frame * spx * esz;
    const char* tile0 = sframe + ((size_t)y0 * (unsigned)L.sw + (unsigned)x0) * esz;
    const size_t pitch = (size_t)L.sw * esz;
    char* oframe = static_cast<char*>(L.out) + (size_t)frame * opx * (out_f32 ? sizeof(float) : sizeof(uint16_t));
    const float z_min = L.z_min, z_max = L.z_max;

    if (cols < COLS || rows < ROWS) {                       // the same for every thread: what does not exist is absent
        for (int k = tid; k < ROWS * STRIDE; k += THREADS) s_z[k] = 0.0f;
        __syncthreads();
    }
    auto keep = [&](float z) { return (z > z_min && z < z_max) ? z : 0.0f; };   // a NaN fails
    if (in_f32) {
        stage_rows<THREADS, 4, COLS>(
            tile0, pitch, cols, rows,
            [&](int r, int e, u_v4 q) {
                const f_v4 z = {keep(__uint_as_float(q.x)), keep(__uint_as_float(q.y)), keep(__uint_as_float(q.z)), keep(__uint_as_float(q.w))};
                *reinterpret_cast<f_v4*>(&s_z[r * STRIDE + e]) = z;
            },
            [&](int r, int e, uintptr_t p) { s_z[r * STRIDE + e] = keep(*reinterpret_cast<const float*>(p)); });
    } else {
        stage_rows<THREADS, 2, COLS>(
            tile0, pitch, cols, rows,
            [&](int r, int e, u_v4 q) {
                const f_v4 a = {keep((float)(q.x & 0xffffu)), keep((float)(q.x >> 16)), keep((float)(q.y & 0xffffu)), keep((float)(q.y >> 16))};
                const f_v4 b = {keep((float)(q.z & 0xffffu)), keep((float)(q.z >> 16)), keep((float)(q.w & 0xffffu)), keep((float)(q.w >> 16))};
                *reinterpret_cast<f_v4*>(&s_z[r * STRIDE + e]) = a;
                *reinterpret_cast<f_v4*>(&s_z[r * STRIDE + e + 4]) = b;
            },
            [&](int r, int e, uintptr_t p) { s_z[r * STRIDE + e] = keep((float)*reinterpret_cast<const uint16_t*>(p)); });
    }
    __syncthreads();

    // this thread's block: rows ly * K .., elements off(row) + lx * K ..
    const float* blk[K];
#pragma unroll
    for (int b = 0; b < K; b++) {
        const int r = ly * K + b;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(tile0) + (size_t)r * pitch;
        const int off = (int)(b0 & 15u) / (int)esz;
        blk[b] = s_z + r * STRIDE + off + lx * K;
    }
    uint32_t v[N];
    uint32_t lo = 0xffffffffu, hi = 0u;
    int m = 0;
#pragma unroll
    for (int b = 0; b < K; b++)
#pragma unroll
        for (int a = 0; a < K; a++) {
            const uint32_t bits = __float_as_uint(blk[b][a]);
            // keep() stored +0 for every sample that is not valid, and a valid one is > z_min >= 0, so its pattern is not 0 -- for
            // z_min == 0 that includes the denormals, which this build does not flush (the Makefile says why); a build that
            // flushed them would have to compare in keep() alone
            const bool ok = bits != 0u;
            v[b * K + a] = ok ? bits : 0xffffffffu;
            m += ok ? 1 : 0;
            lo = min(lo, v[b * K + a]);
            hi = max(hi, bits);
        }
    const bool guard = L.max_gap > 0.0f;
    const bool mixed = guard && m >= 1 && (__uint_as_float(hi) - __uint_as_float(lo)) > L.max_gap;
    const bool mean = L.mode == KDE_DECIMATE_MEAN;
    uint32_t med = lo;                                       // any valid sample where the median is not needed
    if (!mean || __any(mixed ? 1 : 0)) {
        const int t = (m - 1) >> 1;
        med = select_network<N>(v, t);
    }
    const float zmed = __uint_as_float(med);
    const bool filled = m >= L.min_valid;                    // min_valid >= 1
    float result = 0.0f;
    if (filled) {
        if (!mean) {
            result = zmed;
        } else {
            float num = 0.0f;
            int cnt = 0;
#pragma unroll
            for (int b = 0; b < K; b++)
#pragma unroll
                for (int a = 0; a < K; a++) {
                    const float z = blk[b][a];
                    const bool pass = z != 0.0f && (!mixed || fabsf(z - zmed) <= L.max_gap);
                    num = num + (pass ? z : 0.0f);          // +0 leaves a sum of positive depths as it is
                    cnt += pass ? 1 : 0;
                }
            result = num / (float)cnt;
        }
    }
    const int i = i0 + lx, j = j0 + ly;
    if (i < L.ow && j < L.oh) store_depth(oframe, out_f32, (size_t)j * (unsigned)L.ow + (unsigned)i, result);
    // a pixel outside the frame has m == 0: neither filled nor mixed
    uint32_t packed = wave_sum_u32((filled ? 1u : 0u) | (mixed ? 1u << 16 : 0u));
    if ((tid & 63) == 0) s_count[tid >> 6] = packed;
    __syncthreads();
    if (tid == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; w++) sum += s_count[w];
        uint32_t* p = L.partial + ((size_t)frame * gridDim.x + blockIdx.x) * 2;
        p[0] = sum & 0xffffu;
        p[1] = sum >> 16;
    }
}

// D2: grid n, block 256
__global__ __launch_bounds__(256) void decimate_count_kernel(const uint32_t* __restrict__ partial, unsigned groups, uint32_t* __restrict__ filled,
                                                             uint32_t* __restrict__ mixed)
{
    __shared__ uint32_t s_f[4], s_m[4];
    const uint32_t* p = partial + (size_t)blockIdx.x * groups * 2;
    uint32_t f = 0, m = 0;
    for (unsigned g = threadIdx.x; g < groups; g += 256) {
        f += p[2 * (size_t)g];
        m += p[2 * (size_t)g + 1];
    }
    f = wave_sum_u32(f);
    m = wave_sum_u32(m);
    if ((threadIdx.x & 63u) == 0) {
        s_f[threadIdx.x >> 6] = f;
        s_m[threadIdx.x >> 6] = m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        filled[blockIdx.x] = block_sum_u32(s_f);
        mixed[blockIdx.x] = block_sum_u32(s_m);
    }
}

// D3: grid (tiles, n), block 32 * tile_h(K)
template <int K>
__global__ __launch_bounds__(kTileW * tile_h(K)) void decimate_color_kernel(DecimateLaunch L)
{
    constexpr int TH = tile_h(K), THREADS = kTileW * TH, COLS = kTileW * K, ROWS = TH * K;
    constexpr int STRIDE = COLS * 3 + 16;                   // off <= 15 bytes in front of a row
    __shared__ __attribute__((aligned(16))) uint8_t s_c[ROWS * STRIDE];
    const int tid = (int)threadIdx.x, lx = tid & (kTileW - 1), ly = tid >> 5;
    const unsigned frame = blockIdx.y;
    const int tiles_x = (L.ow + kTileW - 1) / kTileW;
    const int trow = (int)blockIdx.x / tiles_x, tcol = (int)blockIdx.x - trow * tiles_x;
    const int i0 = tcol * kTileW, j0 = trow * TH;
    const int x0 = i0 * K, y0 = j0 * K;
    const int cols = min(COLS, L.sw - x0), rows = min(ROWS, L.sh - y0);
    const size_t spx = (size_t)L.sw * L.sh, opx = (size_t)L.ow * L.oh;
    const uint8_t* tile0 = L.bgr + ((size_t)frame * spx + (size_t)y0 * (unsigned)L.sw + (unsigned)x0) * 3;
    const size_t pitch = (size_t)L.sw * 3;
    stage_rows<THREADS, 1, COLS * 3>(
        reinterpret_cast<const char*>(tile0), pitch, cols * 3, rows,
        [&](int r, int e, u_v4 q) { *reinterpret_cast<u_v4*>(&s_c[r * STRIDE + e]) = q; },
        [&](int r, int e, uintptr_t p) { s_c[r * STRIDE + e] = *reinterpret_cast<const uint8_t*>(p); });
    __syncthreads();
    const int i = i0 + lx, j = j0 + ly;
    if (i >= L.ow || j >= L.oh) return;
    const int bw = min(K, L.sw - i * K), bh = min(K, L.sh - j * K);     // the pixels of the block that exist: >= 1 each way
    uint32_t s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int b = 0; b < K; b++) {
        if (b < bh) {
            const int r = ly * K + b;
            const uintptr_t b0 = reinterpret_cast<uintptr_t>(tile0) + (size_t)r * pitch;
            const uint8_t* px = s_c + r * STRIDE + (int)(b0 & 15u) + lx * K * 3;
#pragma unroll
            for (int a = 0; a < K; a++)
                if (a < bw) {
                    s0 += px[a * 3];
                    s1 += px[a * 3 + 1];
                    s2 += px[a * 3 + 2];
                }
        }
    }
    const uint32_t c = (uint32_t)(bw * bh);
    uint8_t* o = L.out_bgr + ((size_t)frame * opx + (size_t)j * (unsigned)L.ow + (unsigned)i) * 3;
    if (c == (uint32_t)(K * K)) {                           // a division by a constant
        o[0] = (uint8_t)((2 * s0 + K * K) / (2 * K * K));
        o[1] = (uint8_t)((2 * s1 + K * K) / (2 * K * K));
        o[2] = (uint8_t)((2 * s2 + K * K) / (2 * K * K));
    } else {
        o[0] = (uint8_t)((2 * s0 + c) / (2 * c));
        o[1] = (uint8_t)((2 * s1 + c) / (2 * c));
        o[2] = (uint8_t)((2 * s2 + c) / (2 * c));
    }
}

template <int K>
void launch_k(const DecimateLaunch& a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((decimate_kernel<K>), grid, dim3(kTileW * tile_h(K)), 0, s, a);
}

template <int K>
void launch_color_k(const DecimateLaunch& a, dim3 grid, hipStream_t s)
{
    hipLaunchKernelGGL((decimate_color_kernel<K>), grid, dim3(kTileW * tile_h(K)), 0, s, a);
}

}  // namespace

unsigned decimate_groups(int ow, int oh, int factor)
{
    const int th = tile_h(factor);
    return (unsigned)((ow + kTileW - 1) / kTileW) * (unsigned)((oh + th - 1) / th);
}

int launch_decimate(const DecimateLaunch& a, hipStream_t s)
{
    const unsigned groups = decimate_groups(a.ow, a.oh, a.factor);
    const dim3 grid(groups, (unsigned)a.n);
    switch (a.factor) {
    case 2: launch_k<2>(a, grid, s); break;
    case 3: launch_k<3>(a, grid, s); break;
    case 4: launch_k<4>(a, grid, s); break;
    case 5: launch_k<5>(a, grid, s); break;
    case 6: launch_k<6>(a, grid, s); break;
    case 7: launch_k<7>(a, grid, s); break;
    case 8: launch_k<8>(a, grid, s); break;
    default: return fail(KDE_ERR_INVALID, "launch_decimate: factor %d", a.factor);
    }
    hipLaunchKernelGGL(decimate_count_kernel, dim3((unsigned)a.n), dim3(256), 0, s, a.partial, groups, a.filled, a.mixed);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

int launch_decimate_color(const DecimateLaunch& a, hipStream_t s)
{
    const dim3 grid(decimate_groups(a.ow, a.oh, a.factor), (unsigned)a.n);
    switch (a.factor) {
    case 2: launch_color_k<2>(a, grid, s); break;
    case 3: launch_color_k<3>(a, grid, s); break;
    case 4: launch_color_k<4>(a, grid, s); break;
    case 5: launch_color_k<5>(a, grid, s); break;
    case 6: launch_color_k<6>(a, grid, s); break;
    case 7: launch_color_k<7>(a, grid, s); break;
    case 8: launch_color_k<8>(a, grid, s); break;
    default: return fail(KDE_ERR_INVALID, "launch_decimate_color: factor %d", a.factor);
    }
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
