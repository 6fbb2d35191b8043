// kde_device_packed.h — the packed forms the tuned kernels share: a BGR pixel as one dword, float math on PAIRS of
// horizontally adjacent pixels (v_pk_*_f32), and the "unit" geometry that feeds the pairs from aligned LDS pairs.
// Users: jbf_fast.hip (K1), jbf_kernels.hip (K0, MRF), ers_kernels.hip (K10), spdsr_kernels.hip (MRF sweep),
// stream_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kde {

// packed BGR (3 bytes per pixel) -> one dword, B in byte 0, byte 3 = 0: the operand of v_dot4_u32_u8
__device__ __forceinline__ uint32_t load_bgrx(const uint8_t* __restrict__ img, size_t pix)
{
    const uint8_t* p = img + pix * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// ---- pair arithmetic ------------------------------------------------------------------------------------------------
// A wave64 f32 VALU instruction costs 4 cycles on a gfx950 SIMD whether it is scalar or v_pk_*_f32, so the tuned kernels
// give a thread a pair of pixels (p0 = even column, p1 = p0 + 1) and write every float add / mul / fma on 2-vectors.
typedef float f2 __attribute__((ext_vector_type(2)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 bcast(float v) { return f2{v, v}; }
// packed add / multiply with the VOP3P clamp bit: the result is clamped to [0, 1] (NaN -> 0, DX10_CLAMP is on).  It turns
// a comparison into a {0,1} mask without v_cmp / v_cndmask: clamp(2 d) is "tap valid", clamp(T - x) is "x < T" on integers
__device__ __forceinline__ f2 pk_add_clamp(f2 a, f2 b)
{
    f2 r;
    asm("v_pk_add_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ f2 pk_mul_clamp(f2 a, f2 b)
{
    f2 r;
    asm("v_pk_mul_f32 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// clamp(c - a*b)
__device__ __forceinline__ f2 pk_fnma_clamp(f2 a, f2 b, f2 c)
{
    f2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 neg_lo:[1,0,0] neg_hi:[1,0,0] clamp" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// ---- unit geometry --------------------------------------------------------------------------------------------------
// A thread's row segment arrives from LDS as aligned 64-bit pairs (col 2m, col 2m+1); tap j of p0 is segment column j,
// tap j of p1 column j + 1.  A "unit" = one tap for each pixel of the pair, chosen so that both sit in ONE aligned pair
// (win odd, HALF = (win - 1) / 2):
//    straight  u <= HALF:      p0 tap 2u         = lo(u),  p1 tap 2u          = hi(u)
//    swapped   HALF < u < win-1, m = u - HALF:
//                              p0 tap 2m + 1     = hi(m),  p1 tap 2m - 1      = lo(m)      (op_sel swap, no data movement)
//    leftover  u == win - 1:   p0 tap 1          = hi(0),  p1 tap win - 2     = lo(HALF)   (two halves of two pairs)
// pair_unit_tap is the tap of `pixel` (0 / 1) in unit u: the host fills per-unit tables with it (log2 of the spatial
// weight of both taps = one SGPR pair), the pickers below read the operands.  A table filled by one rule and read by
// another would be silently wrong output, hence one definition.
__host__ __device__ constexpr int pair_unit_tap(int win, int u, int pixel)
{
    const int half = (win - 1) / 2;
    if (u <= half) return 2 * u;
    if (u < win - 1) return 2 * (u - half) + (pixel ? -1 : 1);
    return pixel ? win - 2 : 1;
}

// the operand pair of unit u out of the segment's pairs: pair m straight or swapped, or two halves of two pairs.
// pp = which of the thread's pixel pairs (its window starts pp pairs into the segment).
template <class V>
__device__ __forceinline__ V pair_unit_pick(const V* seg, int win, int u, int pp = 0)
{
    const int half = (win - 1) / 2;
    if (u <= half) return seg[pp + u];
    if (u < win - 1) return __builtin_shufflevector(seg[pp + (u - half)], seg[pp + (u - half)], 1, 0);
    return V{seg[pp].y, seg[pp + half].x};
}
// the same operands as two scalars (integer operands of v_dot4 / address arithmetic): no swap to perform
template <class V, class T>
__device__ __forceinline__ void pair_unit_pick(const V* seg, int win, int u, int pp, T& v0, T& v1)
{
    const int half = (win - 1) / 2;
    if (u <= half) { v0 = seg[pp + u].x; v1 = seg[pp + u].y; }
    else if (u < win - 1) { v0 = seg[pp + (u - half)].y; v1 = seg[pp + (u - half)].x; }
    else { v0 = seg[pp].y; v1 = seg[pp + half].x; }
}

namespace detail {
// every odd window 3..31: the taps of p0 and of p1 are each a permutation of 0..win-1, and for u < win - 1 both taps of a
// unit lie in one aligned pair of the segment (p1's tap j is column j + 1)
constexpr bool pair_units_ok(int win)
{
    for (int pixel = 0; pixel < 2; pixel++) {
        unsigned seen = 0;
        for (int u = 0; u < win; u++) {
            const int j = pair_unit_tap(win, u, pixel);
            if (j < 0 || j >= win || (seen >> j & 1u)) return false;
            seen |= 1u << j;
        }
    }
    for (int u = 0; u < win - 1; u++)
        if (pair_unit_tap(win, u, 0) / 2 != (pair_unit_tap(win, u, 1) + 1) / 2) return false;
    return true;
}
constexpr bool pair_units_ok_all()
{
    for (int win = 3; win <= 31; win += 2)
        if (!pair_units_ok(win)) return false;
    return true;
}
}  // namespace detail
static_assert(detail::pair_units_ok_all(), "unit geometry: taps must be permutations and share one aligned pair");

}  // namespace kde
