// jbf_fast.hip — tuned gfx950 variants of K1 (joint_bilateral_filtering,
// JointBilateralFilter/JointBilateralFilter.cu:4-83) for the common windows.
//
// The kernel is VALU/transcendental-bound (2 exp per tap against 11 B/pixel of traffic), so the work
// per (pixel, tap) is cut to the minimum the reference's semantics allow:
//   * colour distance as |a|^2 + |b|^2 - 2 a.b with ONE v_dot4_u32_u8 per tap on packed BGRX; -|b|^2 is
//     staged in LDS pre-biased so that the integer result IS the bit pattern of a float, i.e. no int->float convert:
//     scalar kernels (a.b << 1) + bias (one v_lshl_add_u32 per tap) = 2^23 + 2^18 - |b|^2 + 2 a.b; packed kernels take 2^23's
//     bits as the dot product's accumulator and double + bias BOTH taps of a pair with one exact v_pk_fma_f32;
//   * weights live in the log2 domain: arg1 = log2(S_ij) - kc*cd, arg2 = arg1 - kd*(d_q - avg)^2, one
//     v_exp_f32 per tap and pass; pass-1 arguments stay in registers for pass 2 (windows <= 7);
//   * taps that are invalid (depth <= 50 mm or outside the image) cost no branch or select: the scalar kernels
//     give them a bias of 0xFF000000 (-1.7e38, weight exactly 0); the packed kernels stage them with depth 0 and the colour-code
//     term -2^126 (kInvalidHBits): weight exactly 0 in the bodies without the colour rule, which therefore carry no validity
//     factor (plain packed adds into the sums of weights), while the bodies with the colour rule multiply the weight by
//     v = clamp(2 d) = 0 inside the accumulating fma;
//   * the reference's "a factor that underflowed to exactly 0 is not multiplied in" rule (Q1) is decided
//     on the ARGUMENT (integer colour distance / |d_q - avg|) against host-computed thresholds, so it does
//     not depend on how small numbers are rounded by the exp hardware; in the packed kernels the decision is
//     a {0,1} mask produced by the VOP3P clamp bit (no v_cmp / v_cndmask);
//   * every weight is formed at 2^24 times its value (kScaleLog2 is folded into the log2(S) table on the host, so it
//     costs nothing): v_exp_f32 flushes results below 2^-126, which at this scale is exactly the float32
//     underflow-to-zero point 2^-150 of the reference's product S*cf*df -- weights the reference still represents
//     (as denormals) are kept with full precision, weights it rounds to 0 vanish here too, and the two decisions
//     "sum of weights > 0" / "denominator == 0" (JointBilateralFilter.cu:39,76) fall where the reference's fall.
//     The scale cancels in both quotients;
//   * each thread owns PX horizontally adjacent pixels and walks the window row by row from registers.
// Depth + guide + |b|^2 tiles (with halo) are staged once per workgroup in LDS; the workgroup->tile map
// keeps each XCD on a contiguous band of tiles so halos are shared in that XCD's L2.
#include "kde_internal.h"
#include "kde_device_math.h"
#include "kde_device_packed.h"

#include <type_traits>

namespace kde {
namespace {

constexpr uint32_t kMagic = 0x4B000000u;      // float 2^23
constexpr uint32_t kOff = 1u << 18;           // keeps 2 a.b - |b|^2 + kOff positive (|b|^2 <= 195075 < 2^18)
constexpr uint32_t kInvalidBias = 0xFF000000u; // as a float: -1.7e38; as an unsigned int: above every valid code
constexpr float kBiasF = 8388608.0f + 262144.0f;
// packed kernels: bits of the float -(2^24 - 2^18); as the accumulator of dot4(c, c, .) it gives the bits of -(2^24 - 2^18 + |c|^2)
// (2^23 <= 2^24 - 2^18 + |c|^2 < 2^24: the sum stays in the mantissa field of one binade)
constexpr uint32_t kNegHBits = 0xCB7C0000u;
// packed kernels: h_q of an INVALID pixel (depth <= 50 mm or outside the image), -2^126 (about -FLT_MAX / 4).  It swallows every
// colour term it meets (2 (2^23 + a.b), -(2^18 + |a|^2): all below 2^25 in magnitude) and stays finite, so
//   bodies without the colour rule: -cd = -2^126 and a1 = fma(-2^126, kc, ls) <= -kc 2^126 + 24 < -8000 for every kc the tuned
//     kernels serve (kc > 1e-34 > 2^-113, kMinKc below): v_exp_f32 returns exactly 0, in pass 2 as well (a2 <= a1) -- the tap
//     leaves every sum by itself;
//   bodies with it: m = clamp(-2^126 + cd_skip) = 0, a1 = fma(-2^126, kc * 0, ls) = ls, finite (-inf here would give NaN): the
//     tap is removed by its validity factor v = clamp(2 d) = 0, as before.
constexpr uint32_t kInvalidHBits = 0xFE800000u;
constexpr double kMinKc = 1.0e-34;            // jbf_fast_supported: smaller kc (sigma_c above 8.49e16) runs the generic kernel
static_assert(kMinKc * 0x1p126 > 8000.0, "the invalid-tap marker must drive exp2 to 0 for every kc served");
constexpr double kScaleLog2 = 24.0;           // weights are summed at 2^24 scale (see the header comment)

struct FastArgs {
    const float* depth;
    const uint8_t* guide;
    float* out;
    int width, height, n;
    int tiles_x, tiles_y;
    FastDiv24 div_tiles, div_tx;   // workgroup -> (frame, tile row, tile column) by multiplication (kde_device_math.h)
    float kc;        // log2(e) / (2 sigma_c^2)
    float sd;        // sqrt(log2(e) / (2 sigma_d^2))
    float t_skip;    // depth factor skipped when |d_q - avg| * sd >= t_skip
    float t2_skip;   // t_skip^2 (3e38 when nothing is skipped) for the packed-arithmetic form of the rule
    int cd_skip;     // colour factor skipped when cd >= cd_skip
    int vec4;        // width % 4 == 0 and 16-byte aligned frames: the packed kernels load 4-pixel groups
    KDE_STAGE(float* stage_avg; unsigned* stage_counters; int stage_force;)   // tools/hooks/libkde_hip_stage.so only
    // log2 of the spatial table (zeros of the table -> factor skipped -> log2 = 0).  Scalar kernels read
    // tab[i*WIN + j]; packed kernels read the pair (ls[i][j of p0], ls[i][j of p1]) of unit u at
    // tab[(i*WIN + u)*2 .. +1], so the addend of the argument fma is one aligned SGPR pair.
    // 21 x 21 x 2 floats.  The whole struct is the kernel's argument block and stays below HIP's 4 KB limit for it (window 23
    // would need 4232 bytes for the table alone): windows 23..31 read the same pairs from tab_dev, a device copy the handle
    // uploaded once (still wave-uniform addresses: scalar loads)
    const float* tab_dev;
    __attribute__((aligned(8))) float tab[882];
};

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_udot4(a, b, c, false);
}


template <int WIN, int PX, int BX, int BY, bool CACHE, bool CSKIP>
__global__ __launch_bounds__(BX* BY) void jbf_fast_kernel(const FastArgs a)
{
    constexpr int R = WIN / 2;
    constexpr int NT = BX * BY;
    constexpr int TW = BX * PX, TH = BY;
    constexpr int LW = TW + 2 * R, LH = TH + 2 * R;
    constexpr int P = LW;              // row pitch in dwords
    constexpr int SEG = PX + 2 * R;    // row segment a thread needs
    __shared__ float s_d[LH * P];
    __shared__ uint32_t s_c[LH * P];
    __shared__ uint32_t s_n[LH * P];

    // ---- workgroup -> (tile, frame): XCD k works on the k-th contiguous eighth of the tile list ----
    const unsigned id = xcd_band_id(blockIdx.x, gridDim.x);
    const unsigned tiles = (unsigned)a.tiles_x * a.tiles_y;
    const unsigned frame_i = fastdiv24(id, a.div_tiles);
    const unsigned tile = id - frame_i * tiles;
    const int tyi = (int)fastdiv24(tile, a.div_tx), txi = tile - tyi * a.tiles_x;
    const int x0 = txi * TW, y0 = tyi * TH;

    const size_t frame = (size_t)frame_i * a.width * a.height;
    const float* __restrict__ depth = a.depth + frame;
    const uint8_t* __restrict__ guide = a.guide + frame * 3;
    const int tid = threadIdx.x;

    for (int i = tid; i < LW * LH; i += NT) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = x0 + lx - R, gy = y0 + ly - R;
        float d = 0.0f;
        uint32_t c = 0;
        if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height) {
            const size_t q = (size_t)gy * a.width + gx;
            d = depth[q];
            c = load_bgrx(guide, q);
        }
        const bool valid = d > 50.0f;
        s_d[ly * P + lx] = valid ? d : 0.0f;
        s_c[ly * P + lx] = c;
        s_n[ly * P + lx] = valid ? (kMagic + kOff) - dot4(c, c, 0) : kInvalidBias;
    }
    __syncthreads();

    const int tx = tid % BX, ty = tid / BX;
    const int xb = x0 + tx * PX, y = y0 + ty;
    if (xb >= a.width || y >= a.height) return;

    uint32_t cc[PX];
    float cA[PX], skipA[PX];
    uint32_t thrU[PX];
#pragma unroll
    for (int k = 0; k < PX; k++) {
        cc[k] = s_c[(ty + R) * P + tx * PX + R + k];
        const uint32_t na = dot4(cc[k], cc[k], 0);
        cA[k] = -a.kc * (kBiasF + (float)na);                              // exact integer < 2^24, one rounding
        // cA carries that one rounding error into every tap of this pixel as a common factor 2^delta, which
        // cancels in sum(f*d)/sum(f) -- provided a SKIPPED colour factor (exactly 1) carries it too:
        skipA[k] = __builtin_fmaf(kBiasF + (float)na, a.kc, cA[k]);        // = delta (exact product error)
        thrU[k] = CSKIP ? (kMagic + kOff) + na - (uint32_t)a.cd_skip : 0;   // u <= thrU  <=>  cd >= cd_skip
    }

    float arg[CACHE ? WIN * WIN * PX : 1];
    float wsum[PX], wgt[PX];
#pragma unroll
    for (int k = 0; k < PX; k++) wsum[k] = wgt[k] = 0.0f;

    // one tap of pass 1: returns the log2-domain argument of S*cf (or -huge for an invalid tap)
    auto arg1_of = [&](uint32_t cq, uint32_t nq, int k, float ls) -> float {
        // u = bits of the float 2^23 + 2^18 + 2 a.b - |b|^2  (v_dot4_u32_u8 + v_lshl_add_u32)
        const uint32_t u = (dot4(cq, cc[k], 0) << 1) + nq;
        float a1 = __builtin_fmaf(__uint_as_float(u), a.kc, cA[k]);          // = -kc * cd
        if (CSKIP) a1 = (u <= thrU[k]) ? skipA[k] : a1;   // Q1: underflowed colour factor skipped (invalid codes compare above)
        return a1 + ls;
    };

    auto pass1_row = [&](int i) {
        float dr[SEG];
        uint32_t cr[SEG], nr[SEG];
        const int rb = (ty + i) * P + tx * PX;
#pragma unroll
        for (int q = 0; q < SEG; q++) {
            dr[q] = s_d[rb + q];
            cr[q] = s_c[rb + q];
            nr[q] = s_n[rb + q];
        }
#pragma unroll
        for (int j = 0; j < WIN; j++) {
            const float ls = a.tab[i * WIN + j];
#pragma unroll
            for (int k = 0; k < PX; k++) {
                const float a1 = arg1_of(cr[j + k], nr[j + k], k, ls);
                if (CACHE) arg[(i * WIN + j) * PX + k] = a1;
                const float f = __builtin_amdgcn_exp2f(a1);
                wsum[k] = __builtin_fmaf(dr[j + k], f, wsum[k]);
                wgt[k] += f;
            }
        }
    };
    if (CACHE) {
#pragma unroll
        for (int i = 0; i < WIN; i++) pass1_row(i);
    } else {
#pragma unroll 1
        for (int i = 0; i < WIN; i++) pass1_row(i);
    }

    float c2[PX], num[PX], den[PX];
#pragma unroll
    for (int k = 0; k < PX; k++) {
        c2[k] = wsum[k] / wgt[k];                // window average; wgt == 0 handled at the store
        num[k] = den[k] = 0.0f;
    }

    auto pass2_row = [&](int i) {
        float dr[SEG];
        uint32_t cr[SEG], nr[SEG];
        const int rb = (ty + i) * P + tx * PX;
#pragma unroll
        for (int q = 0; q < SEG; q++) {
            dr[q] = s_d[rb + q];
            if (!CACHE) {
                cr[q] = s_c[rb + q];
                nr[q] = s_n[rb + q];
            }
        }
#pragma unroll
        for (int j = 0; j < WIN; j++) {
            const float ls = CACHE ? 0.0f : a.tab[i * WIN + j];
#pragma unroll
            for (int k = 0; k < PX; k++) {
                const float a1 = CACHE ? arg[(i * WIN + j) * PX + k] : arg1_of(cr[j + k], nr[j + k], k, ls);
                // (d_q - avg) first, THEN scale: fma(d_q, sd, -avg*sd) loses ~ulp(avg*sd) and that error is
                // not common to the taps of a pixel
                const float t = (dr[j + k] - c2[k]) * a.sd;
                float a2 = __builtin_fmaf(-t, t, a1);
                a2 = (__builtin_fabsf(t) >= a.t_skip) ? a1 : a2;     // Q1: underflowed depth factor is skipped
                const float f = __builtin_amdgcn_exp2f(a2);
                num[k] = __builtin_fmaf(dr[j + k], f, num[k]);
                den[k] += f;
            }
        }
    };
    if (CACHE) {
#pragma unroll
        for (int i = 0; i < WIN; i++) pass2_row(i);
    } else {
#pragma unroll 1
        for (int i = 0; i < WIN; i++) pass2_row(i);
    }

    float* __restrict__ o = a.out + frame + (size_t)y * a.width + xb;
#pragma unroll
    for (int k = 0; k < PX; k++) {
        float r = 0.0f;
        if (wgt[k] > 0.0f) r = (den[k] == 0.0f) ? 0.0f : num[k] / den[k];
        if (xb + k < a.width) o[k] = r;
        KDE_STAGE(if (a.stage_avg && xb + k < a.width) a.stage_avg[frame + (size_t)y * a.width + xb + k] = c2[k];)
    }
}


// ---------------------------------------------------------------------------------------------------
// Packed-math form.  A wave64 f32 VALU instruction costs 4 cycles on a gfx950 SIMD whether it is scalar
// or v_pk_*_f32, so every float add/mul/fma below works on a PAIR of horizontally adjacent pixels
// (p0 = even column, p1 = p0 + 1) and is written on 2-vectors; the row segment arrives from LDS as
// aligned 64-bit pairs (col 2m, col 2m+1).  A "unit" = one tap for each pixel of the pair, chosen so that
// both taps sit in ONE aligned pair of the segment:
//    straight  (j even):  p0 tap j   = lo(m),  p1 tap j     = hi(m)
//    swapped   (j odd>1): p0 tap j   = hi(m),  p1 tap j - 2 = lo(m)      (op_sel swap, no data movement)
//    leftover:            p0 tap 1   = hi(m0), p1 tap WIN-2 = lo(m1)     (one v_pk_mov_b32)
// The spatial weight costs nothing per tap: log2(S[i][j]) of the unit's two taps is the (SGPR-pair) addend of
// the argument fma.
// Per unit (= 2 taps), window 11, in 4-cycle issue slots (v_exp_f32 counts 2):
//   pass 1: 2 v_dot4 + 2 v_exp + 7 packed (2 a.b + h, -cd, mask, mask*kc, arg fma, 2 accumulating fma)        = 13.3
//           (the two masks only with the colour rule; without it the second accumulating fma is a packed add)
//   pass 2: the same argument (7) + 2 v_exp + 8 packed (d-avg, *sd, T2-t^2, mask, t*mask, arg fma, 2 acc.)   = 19.3
// (the select form of the Q1 rules cost 17 + 24: profiles/r01_sweep_k1_clamp_form.log has the A/B.  Until the colour code
//  took its packed-fma form each tap paid a v_lshl_add_u32 of its own, (a.b << 1) + bias: 14.3 + 20.3; in a tile without
//  rules 10.64 + 13.64 instructions per unit became 9.73 + 12.73, EXPERIMENTS.md Part I item 12.)
// The leftover unit's two biases sit in different pairs: two scalar v_fma_f32 instead of v_pk_mov_b32 + v_pk_fma_f32.
// ---------------------------------------------------------------------------------------------------
// f2 / u2, the clamp forms and the unit pickers: kde_device_packed.h

// packed 16-bit minimum / maximum (v_pk_min_u16 / v_pk_max_u16) on the two halves of a dword
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
// Reduction of an idempotent, commutative op (min / max) over the 64 lanes of a wavefront with DPP moves, one per step:
// lanes 1 and 2 apart inside every quad, quads 1 and 2 apart inside every row of 16 (row_ror), then row_bcast:15 into rows 1
// and 3 and row_bcast:31 into rows 2 and 3 -- lane 63 holds the result, returned in a scalar register.  A lane the move does
// not write keeps its own value (op(v, v) = v).  All 64 lanes must be active.
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ uint32_t dpp_mov(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWS, 0xf, false);
}
template <class Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t v, Op op)
{
    v = op(v, dpp_mov<0xb1>(v));           // quad_perm:[1,0,3,2]
    v = op(v, dpp_mov<0x4e>(v));           // quad_perm:[2,3,0,1]
    v = op(v, dpp_mov<0x124>(v));          // row_ror:4
    v = op(v, dpp_mov<0x128>(v));          // row_ror:8
    v = op(v, dpp_mov<0x142, 0xa>(v));     // row_bcast:15
    v = op(v, dpp_mov<0x143, 0xc>(v));     // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// Instances whose invalid taps get their weight 0 through the colour code (kInvalidHBits) and whose LDS planes are interleaved
// by rows (EXPERIMENTS.md Part I item 14): the recomputing kernels up to window 21.  Left in the earlier form, because the
// new one costs them an occupancy step or scratch (profiles/k1_invalid_taps_registers.md): the windows that keep their pass-1
// arguments (5: 88 bytes of scratch; 7: 142 -> 193 VGPRs), windows >= 23 (128 -> 132 VGPRs with the colour rule), two pairs per
// thread without the colour rule from window 17 on (122 -> 130 VGPRs at 17, 48 more bytes of scratch at 19 / 21), and window 9
// with one pair and no colour rule (12 bytes of scratch under its 8-wave bound).
constexpr bool pk_invalid_by_code(int win, int np, bool cache, bool cskip)
{
    if (cache || win > 21) return false;
    if (!cskip && ((np == 2 && win >= 17) || (np == 1 && win == 9))) return false;
    return true;
}

// second launch bound = waves per SIMD the register allocator must leave room for: the four rule-specialised bodies
// below share one kernel, and without it the window-19 instance grew from 131 to 182 VGPRs (3 -> 2 waves per SIMD)
// (windows >= 23: at least 3 waves per SIMD, i.e. <= 168 VGPRs -- without the bound the instances without the colour rule
//  came out at 228 / 248 registers, 2 waves per SIMD)
// CR = window rows whose pass-1 arguments are kept for pass 2: all of them with CACHE (the windows <= 7), none otherwise
// (recomputed).  r05's partial form (0 < CR < WIN at windows 9..13) was measured slower and removed (EXPERIMENTS.md).
// Window 5 with the arguments kept: at least 5 waves per SIMD (<= 96 VGPRs); without the bound the instances come out
// between 88 and 99 registers, on either side of that allocation step.  (The window-11 default needs no bound: 96 VGPRs, 5
// waves per SIMD; asking for 5 there, or for the step above at windows 11 / 13 with one pair per thread, made the
// scheduler spill 12-40 bytes.)
constexpr int pk_min_waves(int win, int np, bool cache, bool cskip, bool elide_on)
{
    if (win >= 23) return 3;
    if (win == 5 && np == 1 && cache) return 5;
    // one pair per thread, no colour rule, rule body chosen per wavefront: without a bound the two bodies' schedules come out 20-34
    // registers above the same instances with the colour rule (82 / 92 / 106 / 116 VGPRs at windows 9 / 11 / 13 / 15); window 11
    // spills 28-32 bytes when asked for the 7 waves it had and takes 6 (74-76 VGPRs), like its twins with the colour rule
    if (np == 1 && !cskip && elide_on && !cache && win >= 9 && win <= 15) return win == 9 ? 8 : win == 11 ? 6 : 5;
    return 1;
}

// WTX = threads of one wavefront along x: a wavefront owns WTX x (64 / WTX) threads = (WTX * 2 NP) x (64 / WTX) pixels of the
// tile.  WTX = BX is the plain row-major mapping (16x16 threads, two pairs each: 64x4 pixels per wavefront); WTX = 8 makes the
// wavefronts 8x8 threads (32x8 pixels at two pairs per thread), the squarer footprint the per-wavefront rule elision below
// wants (the window-11 built-in kernel; a tile BX = 8 threads wide has that footprint by itself).
template <int WIN, int NP, int BX, int BY, bool CACHE, bool CSKIP, bool VL, bool ELIDE_ON = true, int WTX = BX>
__global__ __launch_bounds__(BX* BY) __attribute__((amdgpu_waves_per_eu(pk_min_waves(WIN, NP, CACHE, CSKIP, ELIDE_ON))))
void jbf_pk_kernel(const FastArgs a)
{
    constexpr int CR = CACHE ? WIN : 0;      // cached rows: all or none
    constexpr int R = WIN / 2;
    constexpr int PX = 2 * NP;
    constexpr int NT = BX * BY;
    constexpr int WTY = 64 / WTX, WAVES_X = BX / WTX;
    static_assert(NT % 64 == 0 && 64 % WTX == 0 && BX % WTX == 0 && BY % WTY == 0, "whole wavefronts, each a WTX x WTY block of threads");
    constexpr int TW = BX * PX, TH = BY;
    constexpr int LH = TH + 2 * R;
    // LDS column 0 is image column o = xb0 - RA with xb0 = (tile index)*TW - S1.  S1 shifts the tiles one
    // column left when R is odd so that a thread's first window column (xb - R) is even (pairs stay aligned),
    // and RA >= R is chosen so that o is a multiple of 4: the loader then moves 4-pixel groups with
    // 16-byte depth loads and 12-byte colour loads that are aligned in the image.
    // VL = false keeps the plain geometry (RA = R, one pixel per loader iteration) for A/B measurements.
    // (S1 = 1 would shift the tiles one column left for odd radii to keep the pairs 8-byte aligned; measured
    //  slower than unaligned pair reads because of the extra, nearly empty tile column it costs)
    constexpr int S1 = 0;
    constexpr int RA = !VL ? R : ((R + 3) / 4 * 4);
    // SH: with the vector loader an odd RA - R (radii 5, 9: windows 11, 19) would start every thread's row segment on an odd
    // LDS column and turn the ds_read_b64 of the pass loops into pairs of ds_read_b32 (measured 5-19 % slower in r02).
    // The staged rows are therefore shifted right by one dword: the global loads stay 16-byte / 12-byte groups aligned in
    // the image, the LDS writes of a group become four single dwords, and the pass loops keep their 64-bit reads.
    constexpr int SH = VL ? ((RA - R) & 1) : 0;
    constexpr bool ALIGNED = ((RA - R + SH) % 2) == 0;     // row segments start on an even LDS column
    constexpr int G = (RA + TW + R + 3) / 4;          // 4-pixel groups per staged row (vector loader)
    constexpr int P = VL ? (SH + 4 * G + 1) / 2 * 2 : (TW + 2 * R);   // row pitch in dwords (even; a multiple of 4 when SH == 0)
    constexpr int SEGP = NP + R;                      // aligned pairs in the row segment of a thread
    static_assert(RA >= R && P % 2 == 0 && (!VL || ((RA + S1) % 4 == 0 && TW % 4 == 0 && (SH != 0 || P % 4 == 0))), "tile geometry");
    // BYCODE instances (pk_invalid_by_code): ONE array, the three planes interleaved by rows: staged row ly = depth | colour | h_q,
    // P dwords each, at ly * RP.  All the 64-bit pairs a thread reads in one window row then lie within 3 P dwords (< 2040 bytes) of
    // ONE address register, inside the offset fields of ds_read2_b64.  (As three arrays the planes are 0x2150 bytes apart at window
    // 11: beyond those fields, a v_add_u32 per plane and pair group in every row trip of this VALU-bound kernel.)  The others keep
    // three arrays, RP = P.  The same number of bytes either way.
    constexpr bool BYCODE = pk_invalid_by_code(WIN, NP, CACHE, CSKIP);
    constexpr int RP = BYCODE ? 3 * P : P;
    // (an array that an instance does not reference takes no LDS)
    __shared__ __attribute__((aligned(16))) float s_d[LH * P];
    __shared__ __attribute__((aligned(16))) uint32_t s_c[LH * P];
    __shared__ __attribute__((aligned(16))) float s_n[LH * P];            // h_q = -(2^24 - 2^18 + |b|^2), see unit_arg
    __shared__ __attribute__((aligned(16))) uint32_t s_rows[3 * LH * P];  // BYCODE; h_q of an invalid pixel: -2^126
    // l_d / l_c / l_n(ly * RP + column): the element of the plane, in whichever arrays the instance uses (constant conditions:
    // only the chosen arrays are referenced)
#define l_d(k) (*(BYCODE ? reinterpret_cast<float*>(s_rows) + (k) : s_d + (k)))
#define l_c(k) (*(BYCODE ? s_rows + P + (k) : s_c + (k)))
#define l_n(k) (*(BYCODE ? reinterpret_cast<float*>(s_rows) + 2 * P + (k) : s_n + (k)))

    const unsigned id = xcd_band_id(blockIdx.x, gridDim.x);
    const unsigned tiles = (unsigned)a.tiles_x * a.tiles_y;
    const unsigned frame_i = fastdiv24(id, a.div_tiles);
    const unsigned tile = id - frame_i * tiles;
    const int tyi = (int)fastdiv24(tile, a.div_tx), txi = tile - tyi * a.tiles_x;
    const int x0 = txi * TW - S1, y0 = tyi * TH;
    const int o = x0 - RA;

    const size_t frame = (size_t)frame_i * a.width * a.height;
    const float* __restrict__ depth = a.depth + frame;
    const uint8_t* __restrict__ guide = a.guide + frame * 3;
    const int tid = threadIdx.x;

    // ELIDE: windows >= 9 pick their rule body per wavefront (below, after the staging barrier).
    // (Only for windows >= 9: at windows 5 and 7 a thread has 25 / 49 units of work and the statistics cost more than
    //  the elided instructions return -- measured 33.9 vs 28.8 us on one 1080p frame at window 5.)
    // ELIDE_ON = false ("-noelide" variants): the same kernel without the statistics and with the full-rule body everywhere --
    // the data-independent floor of the window, measured next to the default by bench.py
    constexpr bool ELIDE = WIN >= 9 && ELIDE_ON;

    if (!VL) {
        for (int i = tid; i < P * LH; i += NT) {
            const int ly = i / P, lx = i - ly * P;
            const int gx = o + lx, gy = y0 - R + ly;
            float d = 0.0f;
            uint32_t c = 0;
            const bool inside = gx >= 0 && gx < a.width && gy >= 0 && gy < a.height;
            if (inside) {
                const size_t q = (size_t)gy * a.width + gx;
                d = depth[q];
                c = load_bgrx(guide, q);
            }
            const bool valid = d > 50.0f;
            const int li = ly * RP + lx;
            l_d(li) = valid ? d : 0.0f;
            l_c(li) = c;
            l_n(li) = __uint_as_float((!BYCODE || valid) ? dot4(c, c, kNegHBits) : kInvalidHBits);
        }
    }
    for (int g = tid; VL && g < G * LH; g += NT) {
        const int ly = g / G, gi = g - ly * G;
        const int gx = o + 4 * gi, gy = y0 - R + ly;
        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t c[4] = {0u, 0u, 0u, 0u};
        if (gy >= 0 && gy < a.height) {
            const size_t q = (size_t)gy * a.width + gx;
            if (a.vec4 && gx >= 0 && gx + 3 < a.width) {
                const float4 dv = *reinterpret_cast<const float4*>(depth + q);
                const uint32_t* cp = reinterpret_cast<const uint32_t*>(guide + q * 3);
                const uint32_t w0 = cp[0], w1 = cp[1], w2 = cp[2];      // 4 packed BGR pixels
                d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
                c[0] = w0 & 0xffffffu;
                c[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
                c[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
                c[3] = w2 >> 8;
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (gx + k >= 0 && gx + k < a.width) {
                        d[k] = depth[q + k];
                        c[k] = load_bgrx(guide, q + k);
                    }
                }
            }
        }
        float nn[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const bool valid = d[k] > 50.0f;
            d[k] = valid ? d[k] : 0.0f;
            nn[k] = __uint_as_float((!BYCODE || valid) ? dot4(c[k], c[k], kNegHBits) : kInvalidHBits);
        }
        const int li = ly * RP + 4 * gi + SH;
        if constexpr (SH == 0) {
            *reinterpret_cast<float4*>(&l_d(li)) = make_float4(d[0], d[1], d[2], d[3]);
            *reinterpret_cast<uint4*>(&l_c(li)) = make_uint4(c[0], c[1], c[2], c[3]);
            *reinterpret_cast<float4*>(&l_n(li)) = make_float4(nn[0], nn[1], nn[2], nn[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                l_d(li + k) = d[k];
                l_c(li + k) = c[k];
                l_n(li + k) = nn[k];
            }
        }
    }
    __syncthreads();

    // wavefront -> its WTX x WTY block of threads.  Everything derived from `wave` is wave-uniform (scalar registers, scalar branches)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int tx0 = WTX * (wave % WAVES_X), ty0 = WTY * (wave / WAVES_X);
    const int tx = tx0 + lane % WTX, ty = ty0 + lane / WTX;
    if (x0 + tx0 * PX >= a.width || y0 + ty0 >= a.height) return;      // the whole wavefront lies outside the image

    // Rule elision (wave-uniform): the reference's "factor that underflowed to 0 is skipped" tests (Q1) cost 2 packed
    // instructions per unit and pass for the colour rule and 3 per unit for the depth rule.  Neither can trip anywhere
    // in this wavefront's pixels when the value ranges of its REGION -- its pixels plus R on every side: each centre and each
    // tap the wavefront can touch -- stay below the thresholds:
    //   colour: cd(p, q) <= sum_c (max_c - min_c)^2 over the region's in-image pixels            < cd_skip
    //   depth:  |d_q - avg_p| <= max - min of the region's valid depths (avg_p is a mean of them), x sd  < t_skip
    // Each wavefront reduces the statistics of its own region from LDS and branches on them; no barrier follows, so the
    // wavefronts of one workgroup may run different bodies.  (Until EXPERIMENTS.md Part I item 13 the decision was one per
    // workgroup, on statistics the loader gathered: the 74-pixel-wide region of a 64x16 tile holds a vertical edge of the
    // content far more often than a 42x18 one.)
    bool tile_c = CSKIP, tile_d = true;
    if constexpr (ELIDE) {
        constexpr int RWP = (WTX * PX + 2 * R) / 2, RH = WTY + 2 * R;     // region: RWP aligned pairs x RH rows
        constexpr int NE = RWP * RH;
        const int sxw = SH + RA - R + tx0 * PX;                            // its first LDS column (even), first LDS row = ty0
        const int gx0 = x0 + tx0 * PX - R, gy0 = y0 + ty0 - R;             // the same corner in the image
        // Positive floats order like their bit patterns.  dmin is taken over bits - 1, so that 0 (= invalid) sorts last.
        uint32_t dmin = 0xffffffffu, dmax = 0u;
        // colour: channels as packed 16-bit lanes, (b, r) of every pixel in one register, g of a pair of pixels in another
        uint32_t brmin = 0x00ff00ffu, brmax = 0u, ggmin = 0x00ff00ffu, ggmax = 0u;
        auto scan = [&](auto masked_tag) {
            constexpr bool MASKED = decltype(masked_tag)::value;
            // element e = lane + 64 k of the region, row-major over its pairs: (row, pair, LDS index) advance by 64 elements per step
            constexpr int QY = 64 / RWP, QP = 64 % RWP;
            int ry = lane / RWP, rp = lane - ry * RWP;
            int li = (ty0 + ry) * RP + sxw + 2 * rp;
#pragma unroll
            for (int k = 0; k < (NE + 63) / 64; k++) {
                if (k > 0) {
                    const bool wrap = rp + QP >= RWP;
                    rp += wrap ? QP - RWP : QP;
                    ry += wrap ? QY + 1 : QY;
                    li += wrap ? (QY + 1) * RP + 2 * (QP - RWP) : QY * RP + 2 * QP;
                }
                if (64 * k + 63 < NE || lane + 64 * k < NE) {
                    const u2 d = *reinterpret_cast<const u2*>(&l_d(li));
                    dmin = min(dmin, min(d.x - 1u, d.y - 1u));
                    dmax = max(dmax, max(d.x, d.y));
                    if constexpr (CSKIP) {       // (instances without the colour rule need no colour statistics)
                        const u2 c = *reinterpret_cast<const u2*>(&l_c(li));
                        uint32_t lo0 = c.x, lo1 = c.y, hi0 = c.x, hi1 = c.y;
                        if constexpr (MASKED) {      // pixels staged from outside the image (zeros) do not count
                            const bool iny = (unsigned)(gy0 + ry) < (unsigned)a.height;
                            const bool in0 = iny & ((unsigned)(gx0 + 2 * rp) < (unsigned)a.width);
                            const bool in1 = iny & ((unsigned)(gx0 + 2 * rp + 1) < (unsigned)a.width);
                            lo0 = in0 ? lo0 : 0x00ffffffu;
                            lo1 = in1 ? lo1 : 0x00ffffffu;
                            hi0 = in0 ? hi0 : 0u;
                            hi1 = in1 ? hi1 : 0u;
                        }
                        brmin = pk_min_u16(pk_min_u16(brmin, lo0 & 0x00ff00ffu), lo1 & 0x00ff00ffu);
                        brmax = pk_max_u16(pk_max_u16(brmax, hi0 & 0x00ff00ffu), hi1 & 0x00ff00ffu);
                        // v_perm_b32 gathers the bytes (0, g of the second pixel, 0, g of the first)
                        ggmin = pk_min_u16(ggmin, __builtin_amdgcn_perm(lo1, lo0, 0x0c050c01u));
                        ggmax = pk_max_u16(ggmax, __builtin_amdgcn_perm(hi1, hi0, 0x0c050c01u));
                    }
                }
            }
        };
        // (depths staged from outside the image are 0 = invalid by themselves: only the colours need the mask)
        if (!CSKIP || (gx0 >= 0 && gx0 + 2 * RWP <= a.width && gy0 >= 0 && gy0 + RH <= a.height)) scan(std::false_type{});
        else scan(std::true_type{});
        const uint32_t w_dmin = wave_reduce(dmin, [](uint32_t p, uint32_t q) { return min(p, q); }) + 1u;   // 0: no valid depth
        const uint32_t w_dmax = wave_reduce(dmax, [](uint32_t p, uint32_t q) { return max(p, q); });
        if constexpr (CSKIP) {
            const uint32_t w_brmin = wave_reduce(brmin, pk_min_u16), w_brmax = wave_reduce(brmax, pk_max_u16);
            const uint32_t w_ggmin = wave_reduce(ggmin, pk_min_u16), w_ggmax = wave_reduce(ggmax, pk_max_u16);
            const int bmin = w_brmin & 0xffffu, bmax = w_brmax & 0xffffu, rmin = w_brmin >> 16, rmax = w_brmax >> 16;
            const int gmin = min(w_ggmin & 0xffffu, w_ggmin >> 16), gmax = max(w_ggmax & 0xffffu, w_ggmax >> 16);
            const int rb = bmax - bmin, rg = gmax - gmin, rr = rmax - rmin;
            if (bmax >= bmin) tile_c = rb * rb + rg * rg + rr * rr >= a.cd_skip;
        }
        if (w_dmax == 0u) {
            tile_d = false;                       // no valid depth in the region: every tap has weight 0
        } else {
            const float range = __uint_as_float(w_dmax) - __uint_as_float(w_dmin);
            // avg_p is a float32 quotient of float32 sums: it can leave [dmin, dmax] by the rounding of those sums, at most
            // about (taps + 8) / 2 ulps of dmax -- an absolute slack that a purely relative margin on the range does not cover
            // when the depths are large and sigma_d is small (1e4 mm at sigma_d = 1 mm)
            const float slack = __uint_as_float(w_dmax) * (float)(WIN * WIN + 8) * 0x1p-24f;
            tile_d = !((range * 1.0001f + slack) * a.sd < a.t_skip);
        }
    }
    KDE_STAGE(if (a.stage_force) { tile_c = CSKIP; tile_d = true; })
    KDE_STAGE(if (a.stage_counters && lane == 0) {
        // the body the dispatch below picks for this wavefront: bit 0 = colour rule compiled in, bit 1 = depth rule
        // (one count per wavefront that owns at least one pixel)
        int body;
        if constexpr (!ELIDE) body = (CSKIP ? 1 : 0) + 2;
        else if constexpr (WIN >= 15) body = ((CSKIP && tile_c) || tile_d) ? (CSKIP ? 1 : 0) + 2 : 0;
        else body = ((CSKIP && tile_c) ? 1 : 0) + (tile_d ? 2 : 0);
        atomicAdd(&a.stage_counters[body], 1u);
    })

    const int xb = x0 + tx * PX, y = y0 + ty;
    if (xb >= a.width || y >= a.height) return;
    const int sx = SH + RA - R + tx * PX;  // LDS column of this thread's first window column (even)

    uint32_t cc[PX];
    f2 negC[NP];          // -(2^18 + |a|^2): w + negC = -cd exactly (integers < 2^24)
#pragma unroll
    for (int pp = 0; pp < NP; pp++) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int k = 2 * pp + h;
            cc[k] = l_c((ty + R) * RP + sx + R + k);
            const uint32_t na = dot4(cc[k], cc[k], 0);
            negC[pp][h] = -((float)kOff + (float)na);
        }
    }

    f2 kc2 = bcast(a.kc);
    asm volatile("" : "+v"(kc2));   // keep kc in a VGPR pair: the fma's only scalar operand is then the log2(S) SGPR pair
    f2 arg[CR > 0 ? CR * WIN * NP : 1];
    f2 wsum[NP], wgt[NP];
#pragma unroll
    for (int pp = 0; pp < NP; pp++) wsum[pp] = wgt[pp] = bcast(0.0f);

    // Q1 rules as packed arithmetic on {0,1} masks made by the clamp bit:
    //   colour: m = clamp(cd_skip - cd) is 1 for cd < cd_skip and 0 otherwise (integers), a1 = fma(-cd, kc*m, ls)
    //   depth:  q = T2 - t^2 (one rounding, sign exact), m = clamp(q * 2^100), a2 = fma(-(t*m), t, a1)
    //   invalid taps: depth 0 and h_q = -2^126 (kInvalidHBits).  Without the colour rule the weight is exactly 0 by itself;
    //   with it the argument stays finite and the tap enters the sums with v = clamp(2 d) = 0
    const f2 Tc = bcast((float)a.cd_skip);
    const f2 T2 = bcast(a.t2_skip);
    const f2 kBig = bcast(0x1p100f);

    // argument (log2 domain, without the row factor) of S*cf for the two taps of unit u of pair pp
    auto unit_arg = [&](auto cs_tag, const u2* cp, const f2* np, int pp, int i, int u) -> f2 {
        constexpr bool CS = decltype(cs_tag)::value;
        uint32_t c0, c1;
        pair_unit_pick(cp, WIN, u, pp, c0, c1);
        const f2 hq = pair_unit_pick(np, WIN, u, pp);
        // the dot product's accumulator input adds 2^23's bit pattern: the result IS the float 2^23 + a.b (a.b < 2^18)
        const f2 ab = f2{__uint_as_float(dot4(c0, cc[2 * pp], kMagic)), __uint_as_float(dot4(c1, cc[2 * pp + 1], kMagic))};
        // w = 2 (2^23 + a.b) - (2^24 - 2^18 + |b|^2) = 2 a.b - |b|^2 + 2^18 for both taps in ONE packed fma: an integer in
        // [67069, 652294], so its rounding changes nothing; w + negC = -cd exactly; then ONE rounding in the argument fma:
        // a1 = log2(S[i][j]) - kc*cd
        f2 w;
        if (u == WIN - 1) {
            // leftover: its two h_q sit in different pairs.  Two scalar fmas write the halves of the result pair directly; the
            // packed form needs a v_pk_mov_b32 into a pair of its own first (same instruction count, two more live registers:
            // 74 instead of 72 VGPRs at window 11 with one pair per thread).  The empty asm only keeps the vectoriser from
            // re-packing them; it emits no instruction.
            float w0 = __builtin_fmaf(ab.x, 2.0f, hq.x), w1 = __builtin_fmaf(ab.y, 2.0f, hq.y);
            asm("" : "+v"(w0));
            asm("" : "+v"(w1));
            w = f2{w0, w1};
        } else {
            w = pk_fma(ab, bcast(2.0f), hq);
        }
        const f2 ncd = w + negC[pp];
        f2 lsj;
        if constexpr (WIN > 21) {
            // the device copy is read through the CONSTANT address space: never written while the kernel runs, wave-uniform
            // address -> one s_load per pair, into the SGPR pair the argument fma takes (a plain global pointer made the
            // compiler issue per-lane global_load_dwordx4 and hold the pairs in VGPRs: 248 instead of ~150 registers)
            typedef const f2 __attribute__((address_space(4)))* cf2p;
            lsj = *(cf2p)(uintptr_t)(a.tab_dev + (i * WIN + u) * 2);
        } else {
            lsj = *reinterpret_cast<const f2*>(&a.tab[(i * WIN + u) * 2]);
        }
        if (CS) return pk_fma(ncd, pk_add_clamp(ncd, Tc) * kc2, lsj);   // Q1: underflowed colour factor skipped
        return pk_fma(ncd, kc2, lsj);
    };
    auto unit_depth = [&](const f2* dp, int pp, int u) -> f2 { return pair_unit_pick(dp, WIN, u, pp); };

    auto pass1_row = [&](auto cs_tag, auto keep_tag, int i) {
        constexpr bool VP = decltype(cs_tag)::value || !BYCODE;   // validity pairs: where an invalid tap's weight is not 0 by itself
        constexpr bool KEEP = decltype(keep_tag)::value;
        f2 dp[SEGP], vp[VP ? SEGP : 1];       // validity pairs: only where the colour rule runs (kInvalidHBits)
        u2 cp[SEGP];
        f2 np[SEGP];
        const int rb = (ty + i) * RP + sx;
#pragma unroll
        for (int m = 0; m < SEGP; m++) {
            dp[m] = ALIGNED ? *reinterpret_cast<const f2*>(&l_d(rb + 2 * m)) : f2{l_d(rb + 2 * m), l_d(rb + 2 * m + 1)};
            cp[m] = ALIGNED ? *reinterpret_cast<const u2*>(&l_c(rb + 2 * m)) : u2{l_c(rb + 2 * m), l_c(rb + 2 * m + 1)};
            np[m] = ALIGNED ? *reinterpret_cast<const f2*>(&l_n(rb + 2 * m)) : f2{l_n(rb + 2 * m), l_n(rb + 2 * m + 1)};
            if constexpr (VP) vp[m] = pk_add_clamp(dp[m], dp[m]);      // 1 for a valid tap (d > 50), 0 for d == 0
        }
#pragma unroll
        for (int pp = 0; pp < NP; pp++) {
#pragma unroll
            for (int u = 0; u < WIN; u++) {
                const f2 a1 = unit_arg(cs_tag, cp, np, pp, i, u);
                if constexpr (KEEP) arg[(i * NP + pp) * WIN + u] = a1;
                const f2 f = f2{__builtin_amdgcn_exp2f(a1.x), __builtin_amdgcn_exp2f(a1.y)};
                wsum[pp] = pk_fma(unit_depth(dp, pp, u), f, wsum[pp]);
                if constexpr (VP) wgt[pp] = pk_fma(unit_depth(vp, pp, u), f, wgt[pp]);
                else wgt[pp] = wgt[pp] + f;             // f == 0 for an invalid tap
            }
        }
    };
    f2 c2[NP], num[NP], den[NP];

    auto pass2_row = [&](auto cs_tag, auto ds_tag, auto keep_tag, int i) {
        constexpr bool VP = decltype(cs_tag)::value || !BYCODE;   // validity pairs: where an invalid tap's weight is not 0 by itself
        constexpr bool DS = decltype(ds_tag)::value;
        constexpr bool KEEP = decltype(keep_tag)::value;
        f2 dp[SEGP], vp[VP ? SEGP : 1];
        u2 cp[SEGP];
        f2 np[SEGP];
        const int rb = (ty + i) * RP + sx;
#pragma unroll
        for (int m = 0; m < SEGP; m++) {
            dp[m] = ALIGNED ? *reinterpret_cast<const f2*>(&l_d(rb + 2 * m)) : f2{l_d(rb + 2 * m), l_d(rb + 2 * m + 1)};
            if constexpr (VP) vp[m] = pk_add_clamp(dp[m], dp[m]);
            if constexpr (!KEEP) {
                cp[m] = ALIGNED ? *reinterpret_cast<const u2*>(&l_c(rb + 2 * m)) : u2{l_c(rb + 2 * m), l_c(rb + 2 * m + 1)};
                np[m] = ALIGNED ? *reinterpret_cast<const f2*>(&l_n(rb + 2 * m)) : f2{l_n(rb + 2 * m), l_n(rb + 2 * m + 1)};
            }
        }
#pragma unroll
        for (int pp = 0; pp < NP; pp++) {
#pragma unroll
            for (int u = 0; u < WIN; u++) {
                f2 a1;
                if constexpr (KEEP) a1 = arg[(i * NP + pp) * WIN + u];
                else a1 = unit_arg(cs_tag, cp, np, pp, i, u);
                const f2 dq = unit_depth(dp, pp, u);
                const f2 t = (dq - c2[pp]) * bcast(a.sd);    // subtract first: see the scalar kernel
                f2 a2;
                if (DS) {
                    const f2 m = pk_mul_clamp(pk_fma(-t, t, T2), kBig);    // Q1: underflowed depth factor skipped
                    a2 = pk_fma(-(t * m), t, a1);
                } else {
                    a2 = pk_fma(-t, t, a1);                                  // the tile's depth range cannot reach the threshold
                }
                const f2 f = f2{__builtin_amdgcn_exp2f(a2.x), __builtin_amdgcn_exp2f(a2.y)};
                num[pp] = pk_fma(dq, f, num[pp]);
                if constexpr (VP) den[pp] = pk_fma(unit_depth(vp, pp, u), f, den[pp]);
                else den[pp] = den[pp] + f;
            }
        }
    };
    // both passes, specialised on which Q1 rules this tile needs
    auto run = [&](auto cs_tag, auto ds_tag) {
        // rows [0, CR): unrolled, arguments kept; rows [CR, WIN): the recomputing loop
#pragma unroll
        for (int i = 0; i < CR; i++) pass1_row(cs_tag, std::true_type{}, i);
#pragma unroll 1
        for (int i = CR; i < WIN; i++) pass1_row(cs_tag, std::false_type{}, i);
#pragma unroll
        for (int pp = 0; pp < NP; pp++) {
            // window averages (wgt == 0 handled at the store); v_rcp_f32 is 1 ulp, the same order as the
            // summation-order noise already present in wsum
            c2[pp] = wsum[pp] * f2{__builtin_amdgcn_rcpf(wgt[pp].x), __builtin_amdgcn_rcpf(wgt[pp].y)};
            num[pp] = den[pp] = bcast(0.0f);
        }
#pragma unroll
        for (int i = 0; i < CR; i++) pass2_row(cs_tag, ds_tag, std::true_type{}, i);
#pragma unroll 1
        for (int i = CR; i < WIN; i++) pass2_row(cs_tag, ds_tag, std::false_type{}, i);
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    // Four bodies for the small windows.  For the wide ones only {both rules, no rule}: a body with exactly one rule made
    // the window-19 instance 182-188 VGPRs instead of 131 (2 instead of 3 waves per SIMD), which costs more than the
    // partial elision gains.
    if constexpr (!ELIDE) {
        run(std::integral_constant<bool, CSKIP>{}, T_{});
    } else if constexpr (WIN >= 15) {
        if ((CSKIP && tile_c) || tile_d) run(std::integral_constant<bool, CSKIP>{}, T_{});
        else run(F_{}, F_{});
    } else {
        if (!CSKIP || !tile_c) {
            if (tile_d) run(F_{}, T_{});
            else run(F_{}, F_{});
        } else {
            if (tile_d) run(T_{}, T_{});
            else run(T_{}, F_{});
        }
    }

    float* __restrict__ op = a.out + frame + (size_t)y * a.width + xb;
#pragma unroll
    for (int pp = 0; pp < NP; pp++) {
        float r0 = 0.0f, r1 = 0.0f;
        if (wgt[pp].x > 0.0f) r0 = (den[pp].x == 0.0f) ? 0.0f : num[pp].x * __builtin_amdgcn_rcpf(den[pp].x);
        if (wgt[pp].y > 0.0f) r1 = (den[pp].y == 0.0f) ? 0.0f : num[pp].y * __builtin_amdgcn_rcpf(den[pp].y);
        if (xb + 2 * pp >= 0 && xb + 2 * pp < a.width) op[2 * pp] = r0;
        if (xb + 2 * pp + 1 < a.width) op[2 * pp + 1] = r1;
        KDE_STAGE(if (a.stage_avg) {
            float* sp = a.stage_avg + frame + (size_t)y * a.width + xb;
            if (xb + 2 * pp >= 0 && xb + 2 * pp < a.width) sp[2 * pp] = c2[pp].x;
            if (xb + 2 * pp + 1 < a.width) sp[2 * pp + 1] = c2[pp].y;
        })
    }
}

#undef l_d
#undef l_c
#undef l_n

template <int WIN, int NP, int BX, int BY, bool CACHE, bool VL, bool ELIDE_ON = true, int WTX = BX>
int launch_pk_variant(const JbfLaunch& l, const FastArgs& fa, bool cskip, hipStream_t s)
{
    FastArgs a = fa;
    a.tiles_x = ceil_div(l.width, BX * NP * 2);
    a.tiles_y = ceil_div(l.height, BY);
    const long long blocks = (long long)a.tiles_x * a.tiles_y * l.n;
    a.div_tiles = make_fastdiv24((uint32_t)(a.tiles_x * a.tiles_y), (uint64_t)blocks);
    a.div_tx = make_fastdiv24((uint32_t)a.tiles_x, (uint64_t)a.tiles_x * a.tiles_y);
    if (blocks > 0x7fffffffLL) return fail(KDE_ERR_INVALID, "jbf: batch too large for one launch");
    if (cskip)
        hipLaunchKernelGGL((jbf_pk_kernel<WIN, NP, BX, BY, CACHE, true, VL, ELIDE_ON, WTX>), dim3((unsigned)blocks), dim3(BX * BY), 0, s, a);
    else
        hipLaunchKernelGGL((jbf_pk_kernel<WIN, NP, BX, BY, CACHE, false, VL, ELIDE_ON, WTX>), dim3((unsigned)blocks), dim3(BX * BY), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

template <int WIN, int PX, int BX, int BY, bool CACHE>
int launch_variant(const JbfLaunch& l, const FastArgs& fa, bool cskip, hipStream_t s)
{
    FastArgs a = fa;
    a.tiles_x = ceil_div(l.width, BX * PX);
    a.tiles_y = ceil_div(l.height, BY);
    const long long blocks = (long long)a.tiles_x * a.tiles_y * l.n;
    a.div_tiles = make_fastdiv24((uint32_t)(a.tiles_x * a.tiles_y), (uint64_t)blocks);
    a.div_tx = make_fastdiv24((uint32_t)a.tiles_x, (uint64_t)a.tiles_x * a.tiles_y);
    if (blocks > 0x7fffffffLL) return fail(KDE_ERR_INVALID, "jbf: batch too large for one launch");
    if (cskip)
        hipLaunchKernelGGL((jbf_fast_kernel<WIN, PX, BX, BY, CACHE, true>), dim3((unsigned)blocks), dim3(BX * BY), 0, s, a);
    else
        hipLaunchKernelGGL((jbf_fast_kernel<WIN, PX, BX, BY, CACHE, false>), dim3((unsigned)blocks), dim3(BX * BY), 0, s, a);
    KDE_HIP_TRY(hipGetLastError());
    return KDE_OK;
}

struct Variant {
    const char* name;
    int window;
    bool packed;           // packed kernels read the table as (tap of p0, tap of p1) pairs per unit
    int (*launch)(const JbfLaunch&, const FastArgs&, bool, hipStream_t);
};

// name: w<window>-<pk|sc><pixels per thread>-<threads x>x<threads y>-<c = pass-1 arguments cached in registers | r = recomputed>
#define V(WIN, PX, BX, BY, CACHE) \
    {"w" #WIN "-sc" #PX "-" #BX "x" #BY "-" #CACHE, WIN, false, &launch_variant<WIN, PX, BX, BY, CACHE>}
#define K(WIN, NP, BX, BY, CACHE) \
    {"w" #WIN "-pk" #NP "-" #BX "x" #BY "-" #CACHE "-v4", WIN, true, &launch_pk_variant<WIN, NP, BX, BY, CACHE, true>}
#define KS(WIN, NP, BX, BY, CACHE) \
    {"w" #WIN "-pk" #NP "-" #BX "x" #BY "-" #CACHE "-v1", WIN, true, &launch_pk_variant<WIN, NP, BX, BY, CACHE, false>}
#define KN(WIN, NP, BX, BY, CACHE) \
    {"w" #WIN "-pk" #NP "-" #BX "x" #BY "-" #CACHE "-v4-noelide", WIN, true, &launch_pk_variant<WIN, NP, BX, BY, CACHE, true, false>}
// KQ: wavefronts of 8x8 threads inside the tile (WTX = 8) instead of BX x (64 / BX); KR ("-rows"): the plain mapping of a tile
// whose built-in kernel is a KQ one
#define KQ(WIN, NP, BX, BY, CACHE) \
    {"w" #WIN "-pk" #NP "-" #BX "x" #BY "-" #CACHE "-v4", WIN, true, &launch_pk_variant<WIN, NP, BX, BY, CACHE, true, true, 8>}
#define KR(WIN, NP, BX, BY, CACHE) \
    {"w" #WIN "-pk" #NP "-" #BX "x" #BY "-" #CACHE "-v4-rows", WIN, true, &launch_pk_variant<WIN, NP, BX, BY, CACHE, true>}
const Variant kVariants[] = {
    // the FIRST variant listed for a window is the built-in choice (interleaved A/B sweep on MI355X,
    // profiles/r03_sweep_k1_variants.log); the others stay selectable for the tile sweep of BASELINE config 3.
    // r03: the vector loader ("-v4": 16-byte depth + 12-byte colour loads, LDS rows shifted so that the pass loops keep
    // their 64-bit reads) is the default at every window: 10.11 vs 10.17 ms at window 19, 1.102 vs 1.101 at window 11
    K(5, 1, 16, 16, true),  K(5, 1, 32, 8, true),   KS(5, 1, 16, 16, true),  K(5, 2, 32, 8, true),  K(5, 1, 32, 8, false),
    V(5, 2, 32, 8, true),   V(5, 1, 64, 4, true),
    K(7, 1, 16, 16, true),  K(7, 1, 32, 8, true),   KS(7, 1, 32, 8, true),  K(7, 1, 32, 8, false),  V(7, 1, 64, 4, true),
    // tiles (pixels) of BASELINE config 3's sweep: 64x16 / 32x16 / 64x8 / 128x8 with 4 or 2 pixels per thread (packed pairs),
    // and the scalar kernels at 2 and 1 pixels per thread (32x16, 32x8)
    // window 11 (EXPERIMENTS.md Part I item 13): the 64x16-pixel tile with its wavefronts as 8x8-thread quarters, 32x8 pixels each --
    // the squarer footprint meets fewer of the content's edges than the 64x4 pixels of a row-major wavefront, so fewer wavefronts
    // run a rule body.  "-rows" is the same tile with the row-major mapping, w11-pk2-8x32 a 32x32-pixel tile whose row-major
    // wavefronts have the 32x8 footprint by themselves (measured equal to the built-in choice)
    KQ(11, 2, 16, 16, false), KR(11, 2, 16, 16, false), K(11, 2, 8, 32, false),
    KS(11, 2, 16, 16, false), KS(11, 1, 16, 16, false), K(11, 1, 16, 16, false), K(11, 1, 32, 8, false),
    KS(11, 1, 32, 8, false), KS(11, 2, 32, 8, false), V(11, 2, 16, 16, false), V(11, 1, 32, 8, false),
    KN(11, 2, 16, 16, false),      // the default without rule elision: the window's data-independent floor
    K(19, 1, 16, 16, false), KS(19, 1, 16, 16, false), KS(19, 2, 16, 16, false), K(19, 2, 16, 16, false), K(19, 1, 32, 8, false),
    KS(19, 1, 32, 8, false), KS(19, 2, 32, 8, false), V(19, 2, 16, 16, false), V(19, 1, 32, 8, false),
    KN(19, 1, 16, 16, false),
    // r04: the other windows the ABI accepts (kde_jbf_params.window_size is a run-time argument in the reference,
    // JointBilateralFilter.cu:10,18-19).  Up to window 21 the log2(S) table travels in the kernel-argument block; windows 23-31
    // (further down) read it from a device table.  Same kernel template, vector loader; the pass-1 arguments stay in registers at window 3 and are recomputed from window 9 on.
    // First listed = built-in choice (tools/sweep_jbf.py, profiles/r04_sweep_k1_windows.log)
    K(3, 1, 16, 16, true),   K(3, 2, 16, 16, true),
    K(9, 2, 16, 16, false),  K(9, 1, 16, 16, false),  KN(9, 2, 16, 16, false),
    K(13, 2, 16, 16, false), K(13, 1, 16, 16, false),
    K(15, 1, 16, 16, false), K(15, 2, 16, 16, false),
    K(17, 1, 16, 16, false), K(17, 2, 16, 16, false),
    K(21, 1, 16, 16, false), K(21, 2, 16, 16, false),
    // windows 23..31: the log2(S) table no longer fits the argument block and comes from a device copy (FastArgs::tab_dev)
    K(23, 1, 16, 16, false), K(25, 1, 16, 16, false), K(27, 1, 16, 16, false), K(29, 1, 16, 16, false), K(31, 1, 16, 16, false),
};
static_assert(sizeof(FastArgs) <= 4096, "FastArgs is passed by value as the kernel-argument block");
#undef V
#undef K
#undef KS
#undef KN
#undef KQ
#undef KR
constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

}  // namespace

int jbf_fast_variant_count() { return kNumVariants; }
const char* jbf_fast_variant_name(int v) { return (v >= 0 && v < kNumVariants) ? kVariants[v].name : "?"; }
int jbf_fast_variant_window(int v) { return (v >= 0 && v < kNumVariants) ? kVariants[v].window : 0; }

// first listed variant of a window that can serve the launch is the built-in choice
int jbf_fast_default_variant(const JbfLaunch& l)
{
    for (int v = 0; v < kNumVariants; v++)
        if (kVariants[v].window == l.window) return v;
    return -1;
}

bool jbf_fast_supported(const JbfLaunch& l)
{
    if (l.color_sigma == 0.0f || l.depth_sigma == 0.0f) return false;
    const double kc = 1.4426950408889634 / (double)l.color_den;
    if (!(kc > kMinKc) || !(kc < 1.0e30)) return false;   // the invalid-tap bias / marker must drive exp2 to 0 (kInvalidHBits)
    return jbf_fast_default_variant(l) >= 0;
}

// log2 of the spatial table at the 2^24 scale, in the layout a variant reads: scalar kernels tab[i*W + j]; packed kernels the
// pair (tap of p0, tap of p1) of unit u at tab[(i*W + u)*2 .. +1] (see jbf_pk_kernel).  out: W*W (scalar) / 2*W*W (packed) floats
void jbf_fast_fill_table(int W, const float* table_host, bool packed, float* out)
{
    auto lg = [&](int i, int j) {
        const float sv = table_host[i * W + j];
        return (float)(((sv == 0.0f) ? 0.0 : std::log2((double)sv)) + kScaleLog2);   // S == 0 -> factor skipped
    };
    if (!packed) {
        for (int i = 0; i < W; i++)
            for (int j = 0; j < W; j++) out[i * W + j] = lg(i, j);
        return;
    }
    for (int i = 0; i < W; i++)
        for (int u = 0; u < W; u++) {   // unit -> (tap of p0, tap of p1)
            out[(i * W + u) * 2] = lg(i, pair_unit_tap(W, u, 0));
            out[(i * W + u) * 2 + 1] = lg(i, pair_unit_tap(W, u, 1));
        }
}

bool jbf_fast_needs_device_table(int window) { return window > 21; }

int launch_jbf_fast(const JbfLaunch& l, int variant, const float* table_host, hipStream_t s)
{
    if (variant < 0 || variant >= kNumVariants || kVariants[variant].window != l.window)
        return fail(KDE_ERR_INVALID, "jbf: variant %d does not implement window %d", variant, l.window);
    FastArgs a;
    memset(&a, 0, sizeof(a));
    a.depth = l.depth;
    a.guide = l.guide;
    a.out = l.out;
    a.width = l.width;
    a.height = l.height;
    a.n = l.n;
    const double log2e = 1.4426950408889634;
    a.kc = (float)(log2e / (double)l.color_den);
    a.sd = (float)std::sqrt(log2e / (double)l.depth_den);
    a.t_skip = std::isinf(l.d2_skip) ? INFINITY : (float)(std::sqrt((double)l.d2_skip) * std::sqrt(log2e / (double)l.depth_den));
    a.t2_skip = std::isinf(a.t_skip) ? 3.0e38f : a.t_skip * a.t_skip;
    a.cd_skip = l.cd_skip;
    a.vec4 = (l.width % 4 == 0) && ((reinterpret_cast<uintptr_t>(l.depth) & 15u) == 0) &&
             ((reinterpret_cast<uintptr_t>(l.guide) & 3u) == 0);
    KDE_STAGE(a.stage_avg = g_stage.jbf_avg; a.stage_counters = g_stage.counters; a.stage_force = g_stage.force_full_rules;)
    if (jbf_fast_needs_device_table(l.window)) {
        if (!l.log2_pk_dev) return fail(KDE_ERR_INVALID, "jbf: window %d needs the handle's device copy of the log2 table", l.window);
        a.tab_dev = l.log2_pk_dev;
    } else {
        jbf_fast_fill_table(l.window, table_host, kVariants[variant].packed, a.tab);
    }
    const bool cskip = l.cd_skip <= 195075;
    return kVariants[variant].launch(l, a, cskip, s);
}

}  // namespace kde
