// temporal_kernels.hip — DepthTemporalFilter: a per-pixel running depth over consecutive frames that follows a surface, starts
// again at a jump, holds over short dropouts and forgets where the guide's colour changed.  The state (value, hist) lives in the
// object between calls.  No reference counterpart.  The rule is stated in kde_hip.h.
//   T1 filter   a thread owns P consecutive pixels (flat raster index: a frame is one row of width * height pixels to it).  It
//               reads their two state words once, walks the n frames in time order with the state in registers and writes the
//               state once: 16 B of state traffic per pixel and call, whatever n is.  The addresses of the frames ahead do not
//               depend on the state, so the loads of a chunk of U frames (depth and guide) are issued before the arithmetic of
//               the chunk's first frame; the frames left over behind the last whole chunk go one at a time.  Depth and guide are
//               read once (streaming loads), the output is written once (streaming stores when the call moves more than the
//               cache holds).  A thread whose P elements are all inside the frame and start on a boundary of their access loads
//               and stores them as 16 / 8 / 4-byte accesses (4 floats, 8 uint16, 12 guide bytes as three dwords), every other
//               thread one element at a time: the values are the same either way.  A thread reads its own pixels of frames
//               t .. t + U - 1 before it writes them: exactly in place is safe.
//               Counts: the four per-frame counts of a thread (at most P each) are packed in two words of 16-bit fields and summed
//               over the wavefront (at most 64 P = 512 per field); lane 0 writes them (not adds) to partial[t][wavefront].  No LDS,
//               no barrier, no atomics: a wavefront never waits for another.
//   T2 count    smoothed[f], jumped[f], held[f], changed[f] = the sums of partial[f][*], one workgroup per frame.
//   reset       both state words of every pixel to 0: a launch, not a memset node.
// Every sum is an integer sum and every pixel's chain of operations is the rule's: the same bytes for any n, any cut of the
// sequence into calls, pointer alignment, P and U.
#include "kde_internal.h"
#include "kde_device_math.h"

#include <type_traits>

namespace kde {
namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerGroup = kThreads / 64;

template <typename T, int N>
struct VecOf {
    typedef T type __attribute__((ext_vector_type(N)));
};

// P consecutive elements from p, `count` of them inside the frame (the others read as 0).  NT: a streaming load.
template <typename T, int P, bool NT>
__device__ __forceinline__ void load_group(const T* p, int count, T (&v)[P])
{
    constexpr int kBytes = P * (int)sizeof(T);
    constexpr int kVec = kBytes > 16 ? 16 : kBytes;         // bytes of one access
    constexpr int kPer = kVec / (int)sizeof(T);             // its elements
    if constexpr (kPer > 1) {
        if (count == P && reinterpret_cast<uintptr_t>(p) % kVec == 0) {
            typedef typename VecOf<T, kPer>::type V;
#pragma unroll
            for (int i = 0; i < P / kPer; i++) {
                const V* q = reinterpret_cast<const V*>(p) + i;
                const V x = NT ? __builtin_nontemporal_load(q) : *q;
#pragma unroll
                for (int j = 0; j < kPer; j++) v[i * kPer + j] = x[j];
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < P; i++) v[i] = i < count ? (NT ? __builtin_nontemporal_load(p + i) : p[i]) : T(0);
}

template <typename T, int P>
__device__ __forceinline__ void store_group(T* p, int count, const T (&v)[P], bool nt)
{
    constexpr int kBytes = P * (int)sizeof(T);
    constexpr int kVec = kBytes > 16 ? 16 : kBytes;
    constexpr int kPer = kVec / (int)sizeof(T);
    if constexpr (kPer > 1) {
        if (count == P && reinterpret_cast<uintptr_t>(p) % kVec == 0) {
            typedef typename VecOf<T, kPer>::type V;
#pragma unroll
            for (int i = 0; i < P / kPer; i++) {
                V x;
#pragma unroll
                for (int j = 0; j < kPer; j++) x[j] = v[i * kPer + j];
                V* q = reinterpret_cast<V*>(p) + i;
                if (nt) __builtin_nontemporal_store(x, q);
                else *q = x;
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < P; i++) {
        if (i >= count) continue;
        if (nt) __builtin_nontemporal_store(v[i], p + i);
        else p[i] = v[i];
    }
}

// the colours of P consecutive pixels as b | g << 8 | r << 16, from p = the first pixel's b
template <int P>
__device__ __forceinline__ void load_colours(const uint8_t* p, int count, uint32_t (&c)[P])
{
    if constexpr ((3 * P) % 4 == 0) {
        if (count == P && reinterpret_cast<uintptr_t>(p) % 4 == 0) {
            constexpr int kWords = 3 * P / 4;
            uint32_t w[kWords];
#pragma unroll
            for (int k = 0; k < kWords; k++) w[k] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p) + k);
#pragma unroll
            for (int i = 0; i < P; i++) {
                const int k = (24 * i) / 32, s = (24 * i) % 32;           // pixel i starts at bit s of word k
                const int k1 = s > 8 ? k + 1 : k;                         // and ends in word k1
                uint32_t x = w[k] >> s;
                if (s > 8) x |= w[k1] << (32 - s);
                c[i] = x & 0xFFFFFFu;
            }
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < P; i++) {
        c[i] = 0;
        if (i < count)
            c[i] = (uint32_t)__builtin_nontemporal_load(p + 3 * i) | ((uint32_t)__builtin_nontemporal_load(p + 3 * i + 1) << 8) |
                   ((uint32_t)__builtin_nontemporal_load(p + 3 * i + 2) << 16);
    }
}

struct Rule {
    float alpha, max_diff, rel_diff, z_min, z_max;
    int persist_min, color_thresh;
    bool scene;                                             // step 2 runs: color_thresh < 765 (and a guide, which the kernel knows)
};

// Steps 1 .. 5 of the rule for one pixel and one frame: each float operation on its own (-ffp-contract=off).  cnt_a gathers
// smoothed | jumped << 16, cnt_b held | changed << 16.
template <bool GUIDE>
__device__ __forceinline__ float temporal_step(const Rule& R, float d, uint32_t c, float& value, uint32_t& hist, uint32_t& cnt_a, uint32_t& cnt_b)
{
    const float z = (d > R.z_min && d < R.z_max) ? d : 0.0f;     // a NaN fails
    // Every branch of the rule is a select: the float operations of a branch not taken are computed and dropped (nothing traps),
    // and the counts are added unconditionally, so no pixel makes its wavefront diverge.
    if (GUIDE) {
        const uint32_t s = hist >> 8;
        const int db = (int)(c & 255u) - (int)(s & 255u), dg = (int)((c >> 8) & 255u) - (int)((s >> 8) & 255u),
                  dr = (int)(c >> 16) - (int)(s >> 16);
        const bool fire = R.scene && abs(db) + abs(dg) + abs(dr) > R.color_thresh;
        cnt_b += (fire && value > 0.0f) ? 0x10000u : 0u;
        value = fire ? 0.0f : value;
        hist = fire ? hist & ~0xFFu : hist;
    }
    const float prev = value;
    const uint32_t low = hist & 0xFFu;
    const bool valid = z > 0.0f, has = prev > 0.0f;
    const float m = R.rel_diff * fminf(z, prev);
    const float t = R.max_diff + m;
    const float diff = z - prev;
    const bool link = valid && has && fabsf(diff) <= t;
    const float step = R.alpha * diff;
    const float blend = prev + step;
    const bool hold = !valid && has && R.persist_min >= 1 && (int)__popc(low) >= R.persist_min;
    const float out = valid ? (link ? blend : z) : (hold ? prev : 0.0f);
    cnt_a += (link ? 1u : 0u) + ((valid && has && !link) ? 0x10000u : 0u);
    cnt_b += hold ? 1u : 0u;
    hist = (GUIDE ? c << 8 : hist & ~0xFFu) | (((low << 1) | (valid ? 1u : 0u)) & 0xFFu);
    value = out;
    return out;
}

// T1: grid ceil(ceil(pixels / P) / 256), block 256
template <int P, int U, bool IN_F32, bool GUIDE>
__global__ __launch_bounds__(kThreads) void temporal_kernel(TemporalLaunch L)
{
    typedef typename std::conditional<IN_F32, float, uint16_t>::type In;
    const size_t px = (size_t)L.w * L.h;
    const size_t first = ((size_t)blockIdx.x * kThreads + threadIdx.x) * P;
    const int count = first >= px ? 0 : (px - first < (size_t)P ? (int)(px - first) : P);
    const size_t at = count ? first : 0;                    // a thread behind the frame touches nothing and adds 0 to the sums
    const bool out_f32 = L.out_format == KDE_DEPTH_F32;
    const bool nt = L.nt_store != 0;
    const In* in = static_cast<const In*>(L.depth) + at;
    const uint8_t* bgr = GUIDE ? L.bgr + at * 3 : nullptr;
    float* out32 = static_cast<float*>(L.out) + at;
    uint16_t* out16 = static_cast<uint16_t*>(L.out) + at;
    const unsigned waves = gridDim.x * kWavesPerGroup, wave = blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
    const Rule R{L.alpha, L.max_diff, L.rel_diff, L.z_min, L.z_max, L.persist_min, L.color_thresh, L.color_thresh < 765};

    float value[P];
    uint32_t hist[P];
    load_group<float, P, false>(L.value + at, count, value);
    load_group<uint32_t, P, false>(L.hist + at, count, hist);

    // UU frames from t0: every load first, then the frames in time order
    auto chunk = [&](auto uu, int t0) {
        constexpr int UU = decltype(uu)::value;
        In d[UU][P];
        uint32_t c[UU][P];
#pragma unroll
        for (int u = 0; u < UU; u++) {
            const size_t frame = (size_t)(t0 + u) * px;
            load_group<In, P, true>(in + frame, count, d[u]);
            if (GUIDE) load_colours<P>(bgr + frame * 3, count, c[u]);
        }
#pragma unroll
        for (int u = 0; u < UU; u++) {
            const size_t frame = (size_t)(t0 + u) * px;
            uint32_t cnt_a = 0, cnt_b = 0;
            float o[P];
#pragma unroll
            for (int i = 0; i < P; i++)     // a pixel behind the frame has d = 0 and no state: it counts nothing and is never stored
                o[i] = temporal_step<GUIDE>(R, (float)d[u][i], GUIDE ? c[u][i] : 0u, value[i], hist[i], cnt_a, cnt_b);
            if (out_f32) {
                store_group<float, P>(out32 + frame, count, o, nt);
            } else {
                uint16_t q[P];
#pragma unroll
                for (int i = 0; i < P; i++) q[i] = depth_to_u16(o[i]);
                store_group<uint16_t, P>(out16 + frame, count, q, nt);
            }
            cnt_a = wave_sum_u32(cnt_a);
            cnt_b = wave_sum_u32(cnt_b);
            if ((threadIdx.x & 63u) == 0) {
                uint32_t* part = L.partial + ((size_t)(t0 + u) * waves + wave) * 2;
                part[0] = cnt_a;
                part[1] = cnt_b;
            }
        }
    };
    int t = 0;
    for (; t + U <= L.n; t += U) chunk(std::integral_constant<int, U>{}, t);
    for (; t < L.n; t++) chunk(std::integral_constant<int, 1>{}, t);

    store_group<float, P>(L.value + at, count, value, false);
    store_group<uint32_t, P>(L.hist + at, count, hist, false);
}

// T2: grid n, block 256
__global__ __launch_bounds__(kThreads) void temporal_count_kernel(const uint32_t* __restrict__ partial, unsigned waves, uint32_t* __restrict__ counts,
                                                                  int max_batch)
{
    __shared__ uint32_t s_count[4][4];
    const uint32_t* p = partial + (size_t)blockIdx.x * waves * 2;
    uint32_t v[4] = {0, 0, 0, 0};
    for (unsigned g = threadIdx.x; g < waves; g += kThreads) {
        const uint32_t a = p[2 * g], b = p[2 * g + 1];
        v[0] += a & 0xFFFFu;
        v[1] += a >> 16;
        v[2] += b & 0xFFFFu;
        v[3] += b >> 16;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        v[k] = wave_sum_u32(v[k]);
        if ((threadIdx.x & 63u) == 0) s_count[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 4) counts[(size_t)threadIdx.x * max_batch + blockIdx.x] = block_sum_u32(s_count[threadIdx.x]);
}

__global__ __launch_bounds__(kThreads) void temporal_reset_kernel(float* __restrict__ value, uint32_t* __restrict__ hist, size_t px)
{
    const size_t at = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (at >= px) return;
    value[at] = 0.0f;
    hist[at] = 0u;
}

template <int P, int U>
void launch_filter(const TemporalLaunch& a, unsigned groups, hipStream_t s)
{
    const dim3 grid(groups), block(kThreads);
    const bool f32 = a.depth_format == KDE_DEPTH_F32;
    if (a.bgr) {
        if (f32) hipLaunchKernelGGL((temporal_kernel<P, U, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((temporal_kernel<P, U, false, true>), grid, block, 0, s, a);
    } else {
        if (f32) hipLaunchKernelGGL((temporal_kernel<P, U, true, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((temporal_kernel<P, U, false, false>), grid, block, 0, s, a);
    }
}

template <int P>
void launch_filter_p(const TemporalLaunch& a, unsigned groups, hipStream_t s)
{
    if (a.unroll == 4) launch_filter<P, 4>(a, groups, s);
    else if (a.unroll == 2) launch_filter<P, 2>(a, groups, s);
    else launch_filter<P, 1>(a, groups, s);
}

}  // namespace

unsigned temporal_waves(size_t px, int pixels)
{
    const size_t threads = (px + (size_t)pixels - 1) / (size_t)pixels;
    return (unsigned)((threads + kThreads - 1) / kThreads) * kWavesPerGroup;
}

// The choice among P = 1, 2, 4, 8 and U = 1, 2, 4, measured at 64 x VGA, 8 x 1080p and one frame of each (EXPERIMENTS.md, "Depth
// temporal filter").  The time loop is a chain per thread, so only the number of wavefronts covers its latency: the largest P
// that still leaves 4000 of them (four per SIMD) -- 1 at VGA, 8 at 1080p.  A call of one frame has no chain and is short: 1000
// wavefronts are enough there, and fewer, larger threads issue less -- 4 at VGA, 8 at 1080p.  Loading 4 frames ahead pays with
// small threads; with P = 8 it costs registers (120 and more) and gains nothing.  U never reaches beyond n.
void temporal_shape(size_t px, int n, int* pixels, int* unroll)
{
    const size_t want = n == 1 ? 1000 : 4000;
    int p = 8;
    while (p > 1 && temporal_waves(px, p) < want) p >>= 1;
    const int u = p == 8 ? 1 : 4;
    *pixels = p;
    *unroll = u <= n ? u : (n >= 2 ? 2 : 1);
}

int launch_temporal(const TemporalLaunch& a, hipStream_t s)
{
    if (!(a.pixels == 1 || a.pixels == 2 || a.pixels == 4 || a.pixels == 8) || !(a.unroll == 1 || a.unroll == 2 || a.unroll == 4))
        return fail(KDE_ERR_INVALID, "launch_temporal: shape %d x %d", a.pixels, a.unroll);
    const unsigned waves = temporal_waves((size_t)a.w * a.h, a.pixels), groups = waves / kWavesPerGroup;
    if (a.pixels == 8) launch_filter_p<8>(a, groups, s);
    else if (a.pixels == 4) launch_filter_p<4>(a, groups, s);
    else if (a.pixels == 2) launch_filter_p<2>(a, groups, s);
    else launch_filter_p<1>(a, groups, s);
    hipLaunchKernelGGL(temporal_count_kernel, dim3((unsigned)a.n), dim3(kThreads), 0, s, a.partial, waves, a.counts, a.max_batch);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

int launch_temporal_reset(float* value, uint32_t* hist, size_t px, hipStream_t s)
{
    hipLaunchKernelGGL(temporal_reset_kernel, dim3((unsigned)((px + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, value, hist, px);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

}  // namespace kde
