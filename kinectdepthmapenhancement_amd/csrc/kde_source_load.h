// kde_source_load.h -- how a kernel reads a kde_error3d_source (a packed float3 cloud, or a float / uint16 depth map that stands
// for the cloud projectiveToReal(float*) makes of it), eight consecutive pixels per lane.  One function for
// error3d_kernels.hip and cloud_kernels.hip, so that both see the same points whichever loads fetched them.
#pragma once
#include "kde_internal.h"
#include "kde_device_math.h"

namespace kde {

__device__ __forceinline__ size_t source_element_size(int format)
{
    return format == KDE_SRC_POINTS_F32 ? sizeof(kde_float3) : format == KDE_SRC_DEPTH_F32 ? sizeof(float) : sizeof(uint16_t);
}

// The points of the pixels 8 * oct .. 8 * oct + 7 of one frame, oct = oct0 + lane, as P[3k .. 3k+2] = (x, y, z) of pixel k;
// a pixel beyond the frame gets a NaN z, which no range admits.  Called by all 64 lanes of a wave together (oct0, frame,
// format and vec are wave-uniform): the 16-byte path of packed float3 is the wave's 6 KB loaded as 384 consecutive float4
// and transposed through LDS.  A depth map gives the cloud projectiveToReal(float*) makes of it: p2r_one, the function K2
// runs.
template <bool NT>
__device__ __forceinline__ void load_octet(const void* __restrict__ frame, int format, bool vec, unsigned oct0, unsigned lane,
                                           unsigned px, const Camera& c, float4* w, float (&P)[24])
{
    const unsigned oct = oct0 + lane;
    const unsigned full = px / 8;                   // octets that lie wholly inside the frame
    const bool whole = vec && oct < full;           // this lane's octet comes from 16-byte loads
    if (format == KDE_SRC_POINTS_F32) {
        if (vec) {
            const unsigned nvec = (oct0 < full ? (full - oct0 < 64u ? full - oct0 : 64u) : 0u) * 6u;
            const float4* p = reinterpret_cast<const float4*>(frame) + (size_t)oct0 * 6;
#pragma unroll
            for (unsigned j = 0; j < 6; j++) {
                const unsigned idx = j * 64u + lane;
                if (idx < nvec) w[idx] = ld4(p + idx, NT);
            }
            wave_exchange_fence();
            if (whole) {
#pragma unroll
                for (unsigned j = 0; j < 6; j++) {
                    const float4 v = w[lane * 6 + j];
                    P[4 * j] = v.x;
                    P[4 * j + 1] = v.y;
                    P[4 * j + 2] = v.z;
                    P[4 * j + 3] = v.w;
                }
            }
            wave_exchange_fence();
        }
        if (!whole) {
            const float* f = static_cast<const float*>(frame) + 24 * (size_t)oct;
#pragma unroll
            for (unsigned k = 0; k < 8; k++) {
                P[3 * k] = P[3 * k + 1] = 0.0f;
                P[3 * k + 2] = NAN;
                if (oct * 8 + k < px) {
                    P[3 * k] = f[3 * k];
                    P[3 * k + 1] = f[3 * k + 1];
                    P[3 * k + 2] = f[3 * k + 2];
                }
            }
        }
        return;
    }
    float z[8];
    if (format == KDE_SRC_DEPTH_F32) {
        if (whole) {
            const float4 a = ld4(reinterpret_cast<const float4*>(frame) + 2 * (size_t)oct, NT);
            const float4 b = ld4(reinterpret_cast<const float4*>(frame) + 2 * (size_t)oct + 1, NT);
            z[0] = a.x; z[1] = a.y; z[2] = a.z; z[3] = a.w;
            z[4] = b.x; z[5] = b.y; z[6] = b.z; z[7] = b.w;
        } else {
            const float* f = static_cast<const float*>(frame) + 8 * (size_t)oct;
#pragma unroll
            for (unsigned k = 0; k < 8; k++) z[k] = oct * 8 + k < px ? f[k] : NAN;
        }
    } else {
        if (whole) {
            const float4 v = ld4(reinterpret_cast<const float4*>(frame) + oct, NT);   // eight uint16: moved, not converted
            const unsigned q[4] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
#pragma unroll
            for (unsigned k = 0; k < 4; k++) {
                z[2 * k] = (float)(q[k] & 0xffffu);     // (float)u, exact: the widening a feed applies
                z[2 * k + 1] = (float)(q[k] >> 16);
            }
        } else {
            const uint16_t* u = static_cast<const uint16_t*>(frame) + 8 * (size_t)oct;
#pragma unroll
            for (unsigned k = 0; k < 8; k++) z[k] = oct * 8 + k < px ? (float)u[k] : NAN;
        }
    }
    const unsigned row = (unsigned)c.width;
    unsigned y = (oct * 8) / row, x = oct * 8 - y * row;
#pragma unroll
    for (unsigned k = 0; k < 8; k++) {
        p2r_one(c, 0, x, y, z[k], &P[3 * k]);
        if (++x == row) {
            x = 0;
            ++y;
        }
    }
}

}  // namespace kde
