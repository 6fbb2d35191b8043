// kde_host_math.h — the host-side arithmetic behind the reference's "a factor that underflowed to exactly 0 is not
// multiplied in" rule (Q1) and the spatial table.  Pure C++ (no HIP): kde_api.cpp includes it, and
// tests/sanitize/host_driver.cpp compiles it with -fsanitize=address,undefined next to the CPU oracle.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace kde {

// smallest float x with exp(-x) rounding to 0 in IEEE binary32 (round to nearest): x > 150 ln 2
inline float exp_zero_threshold()
{
    // exp(-x) rounds to 0 in binary32 iff exp(-x) < 2^-150 iff x > 150 ln 2
    const double t = 150.0 * 0.693147180559945309417232121458;
    float f = (float)t;
    while ((double)f <= t) f = std::nextafterf(f, INFINITY);
    while ((double)std::nextafterf(f, 0.0f) > t) f = std::nextafterf(f, 0.0f);
    return f;
}

// calcSpatialFilter: JointBilateralFilter.cpp:31-40 / EdgeRefinedSuperpixel.cpp:46-55 (powf(x, 2.0f) written x*x)
inline void spatial_table(int window, float sigma, float* table)
{
    for (int i = 0; i < window; i++)
        for (int j = 0; j < window; j++) {
            const float fx = (float)(j - window / 2), fy = (float)(i - window / 2);
            const float dis_x = fx * fx, dis_y = fy * fy;
            table[i * window + j] = expf(-(dis_x + dis_y) / (2.0f * (sigma * sigma)));
        }
}

// smallest non-negative float q with q / den >= thr (float division); +inf if none
inline float smallest_q_reaching(float den, float thr)
{
    if (!(den > 0.0f)) return 0.0f;
    uint32_t lo = 0, hi = 0x7f800000u;   // bit patterns of +0 .. +inf are ordered like the values
    auto val = [](uint32_t b) { float f; memcpy(&f, &b, 4); return f; };
    if (!(val(hi) / den >= thr)) return INFINITY;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (val(mid) / den >= thr) hi = mid;
        else lo = mid + 1;
    }
    return val(lo);
}

// smallest integer colour distance cd in [0, 3*255^2] with (float)cd / den >= thr; 195076 (= 3*255^2 + 1) if none
inline int smallest_cd_reaching(float den, float thr)
{
    int lo = 0, hi = 195076;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if ((float)mid / den >= thr) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ---- acos decided on its argument -----------------------------------------------------------
// acos(d) < c becomes d > t: t is the largest float in [-1, 1] whose double acos, rounded to float, is not below the float
// constant c.  c <= 0 or NaN: +inf (nothing passes); c above pi: the float just below -1 (every d in [-1, 1] passes, a d
// below -1 has a NaN acos and fails).  (float)acos((double)t) does not grow with t, so the boundary is found by bisection
// on the floats in value order.
inline float acos_threshold(float c)
{
    auto key = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    auto unkey = [](uint32_t k) { const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; memcpy(&f, &u, 4); return f; };
    auto reaches = [c](float t) { return (float)std::acos((double)t) >= c; };
    if (c != c) return INFINITY;
    if (!reaches(-1.0f)) return std::nextafterf(-1.0f, -INFINITY);
    if (reaches(1.0f)) return INFINITY;
    uint32_t lo = key(-1.0f), hi = key(1.0f);   // reaches at lo, not at hi
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (reaches(unkey(mid))) lo = mid;
        else hi = mid;
    }
    return unkey(lo);
}

// ---- NormalAdaptiveSuperpixel ------------------------------------------------------------
// NA3: acos(normal_diff) < 3.141592653f / 3.0f (NormalAdaptiveSuperpixel.cu:805) is decided on the argument,
// normal_diff > t
inline float nasp_acos_threshold() { return acos_threshold(3.141592653f / 3.0f); }

// ---- LabelEquivalenceSeg ------------------------------------------------------------------------
// compNormal's acos(d) > 0 && acos(d) < max_angle (LabelEquivalenceSeg.cu:39-40) is d < 1.0f && d > t
inline float les_acos_threshold(float max_angle) { return acos_threshold(max_angle); }

// NA4: expf(-num / (2 * powf(sigma, 2.0f))) (.cu:769, :772) is DEFINED as (float)exp((double)arg), arg the float quotient
inline float nasp_weight(float num, float sigma)
{
    const float arg = -num / (2.0f * (sigma * sigma));
    return (float)std::exp((double)arg);
}

// The weights of the integer numerators 0 .. cap-1, truncated at the first that is exactly 0 (the weight does not grow
// with the numerator, so every later one is 0 too).  Returns the number of entries written (every numerator from there on weighs 0 if
// *reached_zero, else the table covers all of 0 .. cap-1).
inline int nasp_weight_table(float sigma, long long cap, float* table, bool* reached_zero)
{
    *reached_zero = false;
    long long i = 0;
    for (; i < cap; i++) {
        const float w = nasp_weight((float)i, sigma);
        if (w == 0.0f) {
            *reached_zero = true;
            break;
        }
        table[i] = w;
    }
    return (int)i;
}

}  // namespace kde
