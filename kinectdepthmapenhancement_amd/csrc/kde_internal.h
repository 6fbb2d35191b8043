// kde_internal.h — shared host-side plumbing of libkde_hip.so (not part of the public ABI).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/kde_hip.h"
#include "kde_device_math.h" // Camera and the device functions more than one kernel file runs
#include "kde_host_math.h"   // exp_zero_threshold, spatial_table, smallest_*_reaching (pure C++)

namespace kde {

// ---- error reporting -----------------------------------------------------------------------
int fail(int code, const char* fmt, ...);   // records the message for kde_last_error_string() and returns code

#define KDE_HIP_TRY(expr)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::kde::fail(KDE_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                               __FILE__, __LINE__);                                           \
    } while (0)

#define KDE_TRY(expr)                \
    do {                             \
        int rc_ = (expr);            \
        if (rc_ != KDE_OK) return rc_; \
    } while (0)

#define KDE_REQUIRE(cond, ...)                                   \
    do {                                                         \
        if (!(cond)) return ::kde::fail(KDE_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// ---- stage hooks -----------------------------------------------------------------------------
// Compiled ONLY into tools/hooks/libkde_hip_stage.so (-DKDE_STAGE_HOOKS, include/kde_test_hooks.h): the same
// sources as the product library plus per-pixel dumps of K1's / K10's intermediate stages, a switch that forces the
// full-rule bodies, and counters of the body each tile ran.  The product library contains none of it.
#ifdef KDE_STAGE_HOOKS
struct StageCtl {
    float* jbf_avg;          // [n][H][W]: first-pass average of K1 as pass 2 uses it (NaN where the sum of weights is 0)
    float* ers_avg;          // [H][W]: K10 pass-1 average (NaN where the sum of weights is 0)
    float* ers_dev;          // [H][W]: K10 pass-2 mean absolute deviation (undefined where ers_avg is NaN)
    unsigned* counters;      // [8]: K1 tiles per body (colour rule + 2 * depth rule), K10 tiles (small-a, not, no depth rule, depth rule)
    int force_full_rules;    // != 0: every tile runs the body with both Q1 rules / the per-pixel deviation pass
};
extern StageCtl g_stage;
#define KDE_STAGE(...) __VA_ARGS__
#else
#define KDE_STAGE(...)
#endif

constexpr size_t kCacheBytes = (size_t)256 << 20;   // Infinity Cache: calls that move more than this stream past it (ld4 / st4)
// The launch sites that pick the streaming twin of their kernel (non-temporal loads / stores) by the bytes a call moves; the
// order is that of kde_stage_streaming_launches (include/kde_test_hooks.h, tools/hooks/stage.py: SITES)
enum CacheSite {
    kSiteP2rDepth,         // stream_kernels.hip launch_p2r_any: p2r_depth_kernel<true> (depth and interp)
    kSitePointsMap,        // stream_kernels.hip launch_points_any: points_map_kernel<true> (p2r points and r2p)
    kSitePointsToDepthF32, // stream_kernels.hip launch_points_to_depth: points_to_depth_kernel<true, false>
    kSitePointsToDepthU16, //                                            points_to_depth_kernel<true, true>
    kSiteCloud,            // cloud_kernels.hip launch_cloud
    kSiteMesh,             // mesh_kernels.hip launch_mesh (its launch_cloud counts as kSiteCloud)
    kSiteError3d,          // error3d_kernels.hip launch_error3d
    kSiteUndistColor,      // undist_kernels.hip launch_undist_color
    kSiteUndistDepth,      // undist_kernels.hip launch_undist_depth
    kSiteReg,              // reg_kernels.hip launch_reg
    kSiteRegGather,        // reg_kernels.hip launch_reg_gather
    kSiteTemporal,         // kde_api_temporal.cpp kde_temporal_filter_batch: TemporalLaunch::nt_store
    kCacheSites
};
// Does a call that moves `bytes` stream past the cache?  The one statement of the decision for every site above: a site asks
// exactly when the answer `true` makes it launch its streaming form.  The stage build compares with a threshold a test can
// set (kde_stage_set_cache_bytes) and counts the answers `true` per site; the product library has the constant and no state.
#ifdef KDE_STAGE_HOOKS
extern size_t g_stage_cache_bytes;
extern uint64_t g_stage_streaming[kCacheSites];
inline bool past_cache(CacheSite site, size_t bytes)
{
    const bool yes = bytes > g_stage_cache_bytes;
    if (yes) g_stage_streaming[site]++;
    return yes;
}
#else
inline bool past_cache(CacheSite, size_t bytes) { return bytes > kCacheBytes; }
#endif
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// A depth frame is KDE_DEPTH_F32 or KDE_DEPTH_U16 (the sensor's millimetres, 0 = invalid): the one statement of the two formats for
// the host code and the launchers (kde_depth_stage.h holds the rest of what the depth-in / depth-out stages share)
inline bool depth_format_ok(int f) { return f == KDE_DEPTH_F32 || f == KDE_DEPTH_U16; }
__host__ __device__ inline size_t depth_element(int f) { return f == KDE_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float); }
// range[k] of a colour guide, k = |db| + |dg| + |dr| = 0 .. 765 (GuidedDepthUpsampling, DepthHoleFilling)
constexpr int kColourRange = 766;

// Device buffer with RAII; never throws.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    int alloc(size_t count)
    {
        release();
        if (count == 0) return KDE_OK;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            return fail(KDE_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        }
        n = count;
        return KDE_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// Pinned host buffer (the reference's cudaMallocHost'ed *_Host members), allocated lazily.
template <typename T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    int ensure(size_t count)
    {
        if (p && n >= count) return KDE_OK;
        release();
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(KDE_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
        }
        n = count;
        return KDE_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
    ~PinnedBuf() { release(); }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
};

// ---- launchers implemented in the .hip translation units ------------------------------------
struct JbfLaunch {
    int width, height, n;
    int window;
    const float* depth;        // [n][H][W]
    const uint8_t* guide;      // [n][H][W][3]
    float* out;                // [n][H][W]
    const float* s_eff;        // device, window^2 (zeros replaced by 1)
    const float* table_host;   // host, window^2 (calcSpatialFilter as computed)
    const float* log2_pk_dev;  // device, 2 * window^2: the packed kernels' log2(S) pairs, windows > 21 only (jbf_fast.hip)
    float spatial_sigma, color_sigma, depth_sigma;
    float color_den, depth_den;    // 2*sigma^2 as the reference forms it (float)
    int cd_skip;               // colour factor skipped (== underflow to 0) when cd >= cd_skip
    float d2_skip;             // depth factor skipped when (d_q - wavg)^2 >= d2_skip
    int variant;
};
int launch_jbf(const JbfLaunch& a, hipStream_t s);
int jbf_active_variant(const JbfLaunch& a);
// tuned variants (jbf_fast.hip); variant ids there are 0-based, the public id is +1 (0 = generic kernel)
int jbf_fast_variant_count();
const char* jbf_fast_variant_name(int v);
int jbf_fast_variant_window(int v);
int jbf_fast_default_variant(const JbfLaunch& l);
bool jbf_fast_supported(const JbfLaunch& l);
void jbf_fast_fill_table(int window, const float* table_host, bool packed, float* out);
bool jbf_fast_needs_device_table(int window);
int launch_jbf_fast(const JbfLaunch& l, int variant, const float* table_host, hipStream_t s);
int jbf_variant_count();
const char* jbf_variant_name(int v);

struct PresmoothLaunch {
    int width, height, n;
    int radius;                // ksz/2 after OpenCV's adjustment
    const uint8_t* src;        // [n][H][W][3]
    uint8_t* dst;
    const float* lut;          // device, (radius^2+1) x 766 weights
    long long grid_cap;        // persistent-grid size for the tuned kernels (presmooth_resident_blocks at handle creation)
};
int launch_presmooth(const PresmoothLaunch& a, hipStream_t s);
long long presmooth_resident_blocks(int radius);   // on the current device; 0 for radii served by the generic kernel

struct MrfLaunch {
    int width, height, n, window;
    const float* depth;
    const uint8_t* bgr;
    float* out;
    float color_sigma, smooth_sigma;
};
int launch_mrf(const MrfLaunch& a, hipStream_t s);

int launch_p2r_depth(const Camera& c, int n, const float* depth, kde_float3* out, hipStream_t s);
int launch_p2r_points(const Camera& c, int n, const kde_float3* in, kde_float3* out, hipStream_t s);
int launch_p2r_interp(const Camera& c, int n, const float* depth, kde_float3* out, hipStream_t s);
int launch_r2p(const Camera& c, int n, const kde_float3* in, kde_float3* out, hipStream_t s);

int launch_buf_init(kde_weighted_d* buf, size_t n, hipStream_t s);
int launch_buf_insert_depth(kde_weighted_d* buf, const float* d, size_t n, hipStream_t s);
int launch_buf_insert_float2(kde_weighted_d* buf, const float* xy, int width, int height, hipStream_t s);
int launch_buf_get(const kde_weighted_d* buf, float* out, size_t n, int which, hipStream_t s);
int launch_buf_update(kde_weighted_d* buf, const float* d, size_t n, int n_frames, hipStream_t s);
// host-fed JBF (kde_jbf_feed_process): n uint16 depth samples -> float, exact
int launch_widen_u16(const uint16_t* src, float* dst, size_t n, hipStream_t s);
// kde_points_to_depth: the z of n packed points as float (bits unchanged) or as uint16 (depth_to_u16, kde_device_math.h)
int launch_points_to_depth(const kde_float3* pts, void* out, size_t n, bool u16, hipStream_t s);

// MeanError3D (error3d_kernels.hip): the quality metric of main.cpp:220-308 for n frames x m candidates, two launches
constexpr int kError3dMaxCandidates = 8;
constexpr unsigned kError3dSegmentPixels = 2048;   // pixels one workgroup reduces to one partial: a constant of the build
struct Error3dPartial {                            // one segment of one frame for one candidate
    double sum;
    uint32_t count, pad_;
};
inline unsigned error3d_segments(size_t frame_px) { return (unsigned)((frame_px + kError3dSegmentPixels - 1) / kError3dSegmentPixels); }
struct Error3dLaunch {
    int n, m;
    const void* cand[kError3dMaxCandidates];       // [n][H][W] of the format's element
    int cand_format[kError3dMaxCandidates];        // KDE_SRC_*
    const void* truth;                             // [truth_frames][H][W]
    int truth_format;
    int truth_frames;                              // 1 or n
    Camera cam;                                    // width, height always; fx, fy, cx, cy where a source is a depth map
    float z_min, z_max;
    Error3dPartial* partials;                      // [n][m][error3d_segments(W * H)]
    kde_error3d_result* results;                   // [n][m]
};
int launch_error3d(const Error3dLaunch& a, hipStream_t s);

// PointCloudXYZRGB (cloud_kernels.hip): the coloured cloud of main.cpp:211-300 for n frames, compacted in raster order
constexpr unsigned kCloudSegmentPixels = 2048;     // pixels one workgroup counts and scatters: a constant of the build
constexpr unsigned kCloudScanThreads = 256;        // segment counts one pass of the per-frame scan (C2) takes
inline unsigned cloud_segments(size_t frame_px) { return (unsigned)((frame_px + kCloudSegmentPixels - 1) / kCloudSegmentPixels); }
struct CloudLaunch {
    int n;
    const void* src;                               // [n][H][W] of the format's element
    int format;                                    // KDE_SRC_*
    const uint8_t* bgr;                            // [bgr_frames][H][W][3]
    int bgr_frames;                                // 1 or n
    Camera cam;                                    // width, height always; fx, fy, cx, cy where the source is a depth map
    float z_min, z_max, divisor;
    int negate_z, organized;
    uint32_t* seg;                                 // [n][cloud_segments(W * H)]: counts after C1, offsets after C2 (dense mode)
    uint32_t* counts;                              // [n]
    kde_cloud_point* out;                          // [n][H][W] records, 16-byte aligned: frame f's slot starts at f * W * H
};
int launch_cloud(const CloudLaunch& a, hipStream_t s);
// C2 alone: seg [n][segs] counts become offsets in place, counts[f] the total of frame f
int launch_segment_scan(uint32_t* seg, unsigned segs, uint32_t* counts, int n, hipStream_t s);

// OrganizedMesh (mesh_kernels.hip): the triangles of the depth grid over the dense cloud of launch_cloud.  The tables are
// per frame and cover whole segments of kCloudSegmentPixels pixels: a pixel beyond the frame is an invalid pixel without a quad.
constexpr unsigned kMeshGroupPixels = 64;          // pixels one validity word and one rank prefix stand for
inline size_t mesh_table_pixels(size_t frame_px) { return (size_t)cloud_segments(frame_px) * kCloudSegmentPixels; }
struct MeshLaunch {
    CloudLaunch cloud;                             // the vertices: dense mode; seg holds the segments' vertex offsets after it ran
    float max_diff, rel_diff;
    int diagonal, flip_winding;
    uint8_t* mask;                                 // [n][table pixels / 8]: bit k of byte t = pixel 8 t + k is a vertex
    uint32_t* group_rank;                          // [n][table pixels / 64]: vertices of the segment before the group
    uint8_t* code;                                 // [n][table pixels]: the triangles the pixel's quad gives, a set of four forms
    uint32_t* tri_seg;                             // [n][segments]: triangle counts after M1, offsets after M2
    uint32_t* tri_counts;                          // [n]
    kde_mesh_triangle* triangles;                  // [n][2 (W-1) (H-1)] records, 4-byte aligned
};
int launch_mesh(const MeshLaunch& a, hipStream_t s);

// DepthRegistration (reg_kernels.hip): what Kinect.cpp:71-75 asks OpenNI for -- the depth map as the colour camera sees it
struct RegCalib {
    float fxd, fyd, cxd, cyd;                      // depth camera; cx, cy stay floats (not truncated as DimensionConvertor does)
    float fxc, fyc, cxc, cyc;                      // colour camera
    float r[9], t[3];                              // P_colour = R * P_depth + t, millimetres
};
constexpr int kRegMaxSplat = 16;
constexpr int kRegMaxSide = 1 << 24;               // W - 1 and H - 1 of either camera are exact floats
// keys per frame of the z-buffer: the frame's pixels rounded up to whole octets, so every frame starts on a 32-byte boundary
__host__ __device__ constexpr size_t reg_zstride(size_t color_px) { return (color_px + 7) & ~(size_t)7; }
struct RegLaunch {
    int n;
    const void* depth;                             // [n][hd][wd] float or uint16
    int depth_format;                              // KDE_DEPTH_*
    int wd, hd, wc, hc;
    RegCalib c;
    float z_min, z_max;
    int max_splat;                                 // 0: point mode
    uint32_t* zbuf;                                // [n][reg_zstride(wc * hc)] keys (register only)
    uint32_t* filled;                              // [n] (register only)
    void* out;                                     // [n][hc][wc] float or uint16 (register only)
    int out_format;                                // KDE_DEPTH_*
};
int launch_reg(const RegLaunch& a, hipStream_t s);
// the companion gather: out [n][hd][wd][3] from bgr [bgr_frames][hc][wc][3]
int launch_reg_gather(const RegLaunch& a, const uint8_t* bgr, int bgr_frames, uint8_t* out, hipStream_t s);

// LensUndistortion (undist_kernels.hip): distorted frames resampled into a pinhole view, a gather
struct UndistCalib {
    float fx, fy, cx, cy;                          // the source (distorted) camera; cx, cy stay floats
    float fxn, fyn, cxn, cyn;                      // the target (pinhole) camera
    float k1, k2, p1, p2, k3, k4, k5, k6;          // OpenCV's order (the rational model; k4..k6 = 0: Brown-Conrady)
};
struct UndistLaunch {
    int n;
    int sw, sh, ow, oh;                            // source and output frame
    UndistCalib c;
    float z_min, z_max;                            // depth only
    int depth_interp;                              // 0: nearest, 1: guarded bilinear
    float max_gap;
    const void* depth;                             // [n][sh][sw] float or uint16 (depth only)
    int depth_format;                              // KDE_DEPTH_*
    void* out;                                     // [n][oh][ow] float or uint16 (depth only)
    int out_format;                                // KDE_DEPTH_*
    uint32_t* filled;                              // [n] (depth only)
};
// out [n][oh][ow][3] from bgr [bgr_frames][sh][sw][3]
int launch_undist_color(const UndistLaunch& a, const uint8_t* bgr, int bgr_frames, uint8_t* out, hipStream_t s);
int launch_undist_depth(const UndistLaunch& a, hipStream_t s);          // 2 kernels: filled = 0, the remap
int launch_undist_map(const UndistLaunch& a, float2* map, hipStream_t s);   // map [oh][ow] of (us, vs)

// GuidedDepthUpsampling (upsample_kernels.hip): low-resolution depth to the size of its colour image, a gather
constexpr int kUpsampleMaxRadius = 4;
constexpr int kUpsampleTileW = 32, kUpsampleTileH = 8;     // output pixels of a tile
constexpr int kUpsampleTilesPerGroup = 4;          // consecutive tiles (raster order) of one workgroup
// the tap window of a tile the kernel's LDS arrays hold: the bound derived in upsample_kernels.hip (42 x 18) and two to spare
constexpr int kUpsampleWinW = kUpsampleTileW + 2 * kUpsampleMaxRadius + 4, kUpsampleWinH = kUpsampleTileH + 2 * kUpsampleMaxRadius + 4;
// x0 of output column i (y0 of row j with sy): one function for the kernel and for the window check of kde_upsample_create
__host__ __device__ inline int upsample_floor(int i, float scale) { return (int)floorf(((float)i + 0.5f) * scale - 0.5f); }
struct UpsampleLaunch {
    int n;
    int sw, sh, ow, oh;                            // source and output frame
    int radius;                                    // 1 .. kUpsampleMaxRadius
    float sx, sy;                                  // (float)sw / (float)ow, (float)sh / (float)oh
    float max_gap, z_min, z_max;                   // max_gap 0: no guard
    const void* depth;                             // [n][sh][sw] float or uint16
    int depth_format;                              // KDE_DEPTH_*
    const uint8_t* bgr;                            // [bgr_frames][oh][ow][3]
    int bgr_frames;                                // 1 or n
    void* out;                                     // [n][oh][ow] float or uint16
    int out_format;                                // KDE_DEPTH_*
    const int* gx_of;                              // [sw]: the output column that is source column qx
    const int* gy_of;                              // [sh]
    const float* range;                            // [kColourRange]
    uint32_t* partial;                             // [n][upsample_groups(ow, oh)]: the count of each workgroup
    uint32_t* filled;                              // [n]
};
unsigned upsample_groups(int ow, int oh);                     // workgroups per frame
int launch_upsample(const UpsampleLaunch& a, hipStream_t s);  // 2 kernels: the upsampling, filled = the sum of its counts

// DepthHoleFilling (holefill_kernels.hip): holes filled from their valid neighbours under a colour guide, pass by pass
constexpr int kHolefillMaxRadius = 3;
constexpr int kHolefillMaxIterations = 64;
constexpr int kHolefillMaxFuse = 4;                // passes one launch performs in LDS, at the most
constexpr int kHolefillTileW = 32, kHolefillTileH = 16;    // pixels of a workgroup's tile
struct HolefillLaunch {
    int n;
    int w, h;
    int radius;                                    // 1 .. kHolefillMaxRadius
    int iterations;                                // 1 .. kHolefillMaxIterations
    int fuse;                                      // 1 .. kHolefillMaxFuse passes per launch
    int min_taps, gap_rule;
    float max_gap, z_min, z_max;                   // max_gap 0: no guard
    const void* depth;                             // [n][h][w] float or uint16
    int depth_format;                              // KDE_DEPTH_*
    const uint8_t* bgr;                            // [bgr_frames][h][w][3]
    int bgr_frames;                                // 1 or n
    void* out;                                     // [n][h][w] float or uint16; overlaps neither depth nor state
    int out_format;                                // KDE_DEPTH_*
    float* state[2];                               // [n][h][w] each: the state between two launches
    uint8_t* pass;                                 // [n][h][w]: pass_of, in place between launches and the result
    const float* space;                            // [(2 radius + 1)^2]
    const float* range;                            // [kColourRange]
    uint32_t* partial;                             // [n][holefill_groups(w, h)][2]: the two counts of each workgroup
    uint32_t* filled;                              // [n]
    uint32_t* remaining;                           // [n]
    // one launch of the fill kernel (set by launch_holefill)
    const void* src;                               // the state it reads: depth, or what the launch before it wrote
    int src_format;
    void* dst;
    int dst_format;
    int p0, passes;                                // it performs passes p0 + 1 .. p0 + passes
    bool first, last;                              // first: src is the caller's depth and is sanitised; last: dst is out, counts
};
unsigned holefill_groups(int w, int h);                       // workgroups per frame
// ceil(iterations / fuse) launches of the fill kernel, then filled / remaining = the sums of the last one's counts
int launch_holefill(const HolefillLaunch& a, hipStream_t s);

// DepthSpeckleFilter (speckle_kernels.hip): connected components under a depth link, the small ones removed
constexpr int kSpeckleMaxSize = 1 << 24;           // min_size, at the most
constexpr int kSpeckleTileW = 32, kSpeckleTileH = 16;      // pixels of a workgroup's tile
struct SpeckleLaunch {
    int n;
    int w, h;
    int min_size, connectivity;                    // 1 .. kSpeckleMaxSize; 4 or 8
    float max_diff, rel_diff, z_min, z_max;
    const void* depth;                             // [n][h][w] float or uint16
    int depth_format;
    void* out;                                     // [n][h][w] float or uint16; may be depth itself in depth's format
    int out_format;
    int32_t* labels;                               // [n][h][w] or nullptr
    int32_t* parent;                               // [n][h][w]: the union-find table, raster indices within a frame, -1 invalid
    uint32_t* size;                                // [n][h][w]: pixels of a local component at its local root, of a component at its root
    uint32_t* partial;                             // [n][speckle_groups(w, h)][3]: removed, kept roots, caps of each workgroup
    uint32_t* removed;                             // [n]
    uint32_t* components;                          // [n]
    uint32_t* capped;                              // [n]
};
unsigned speckle_groups(int w, int h);                        // workgroups per frame
// 5 kernels (3 for a frame of one tile): tile labelling, seam unions, resolve, apply, the sums of the counts
int launch_speckle(const SpeckleLaunch& a, hipStream_t s);

// DepthTemporalFilter (temporal_kernels.hip): a per-pixel running value over consecutive frames, the state kept between calls
struct TemporalLaunch {
    int n;
    int w, h;
    int pixels, unroll;                            // the pixels a thread owns (1, 2, 4, 8), the frames it loads ahead (1, 2, 4)
    float alpha, max_diff, rel_diff, z_min, z_max;
    int persist_min, color_thresh;                 // 0 .. 8; 0 .. 765
    const void* depth;                             // [n][h][w] float or uint16
    int depth_format;
    const uint8_t* bgr;                            // [n][h][w][3] or nullptr
    void* out;                                     // [n][h][w] float or uint16; may be depth itself in depth's format
    int out_format;
    int nt_store;                                  // != 0: the output streams past the cache
    float* value;                                  // [h][w]: the state
    uint32_t* hist;                                // [h][w]
    uint32_t* partial;                             // [n][temporal_waves(w * h, pixels)][2]: smoothed | jumped << 16, held | changed << 16
    uint32_t* counts;                              // smoothed[max_batch], jumped[max_batch], held[max_batch], changed[max_batch]
    int max_batch;
};
unsigned temporal_waves(size_t px, int pixels);               // wavefronts of the filter launch
void temporal_shape(size_t px, int n, int* pixels, int* unroll);   // the library's choice
// 2 kernels: the filter, the sums of the counts
int launch_temporal(const TemporalLaunch& a, hipStream_t s);
// 1 kernel: both state words of px pixels to 0
int launch_temporal_reset(float* value, uint32_t* hist, size_t px, hipStream_t s);

// DepthDecimation (decimate_kernels.hip): frames made `factor` times smaller each way, a pixel from the valid samples of its block
struct DecimateLaunch {
    int n;
    int sw, sh, ow, oh;                            // source and output frame: ow = ceil(sw / factor), oh likewise
    int factor;                                    // 2 .. 8
    int mode, min_valid;                           // KDE_DECIMATE_MEDIAN | KDE_DECIMATE_MEAN; 1 .. factor^2
    float max_gap, z_min, z_max;                   // max_gap 0: no guard
    const void* depth;                             // [n][sh][sw] float or uint16
    int depth_format;
    void* out;                                     // [n][oh][ow] float or uint16
    int out_format;
    uint32_t* partial;                             // [n][decimate_groups(ow, oh, factor)][2]: filled, mixed of each workgroup
    uint32_t* filled;                              // [n]
    uint32_t* mixed;                               // [n]
    const uint8_t* bgr;                            // the colour call: [n][sh][sw][3]
    uint8_t* out_bgr;                              //                  [n][oh][ow][3]
};
unsigned decimate_groups(int ow, int oh, int factor);         // workgroups per frame
int launch_decimate(const DecimateLaunch& a, hipStream_t s);  // 2 kernels: the decimation, the sums of its counts
int launch_decimate_color(const DecimateLaunch& a, hipStream_t s);   // 1 kernel

struct DaspGeom {
    int width, height, rows, cols, wx, wy;
};
// n = frames of a batch (per-frame colour / cloud / cluster tables / outputs, back to back); the single-frame forms take n = 1
int launch_dasp_sample(const DaspGeom& g, int n, const uint8_t* bgr, const kde_float3* pts, kde_superpixel* mean,
                       kde_float3* centers, kde_superpixel* mean2, kde_float3* centers2, hipStream_t s);
int launch_dasp_init_ld(const DaspGeom& g, kde_label_distance* ld, hipStream_t s);   // init_LD alone: a call of no iteration
int launch_dasp_calc_ld(const DaspGeom& g, const uint8_t* bgr, const kde_float3* pts, kde_label_distance* ld,
                        const kde_superpixel* mean, const kde_float3* centers, int32_t* labels, float color_sigma,
                        float spatial_sigma, float depth_sigma, bool first, hipStream_t s);
int launch_dasp_calc_ld_dual(const DaspGeom& g, int n, const uint8_t* bgr, const kde_float3* pts, kde_label_distance* ld_a,
                             const kde_superpixel* mean_a, const kde_float3* centers_a, int32_t* labels_a,
                             const float sig_a[3], kde_label_distance* ld_b, const kde_superpixel* mean_b,
                             const kde_float3* centers_b, int32_t* labels_b, const float sig_b[3], bool first, bool write_ld,
                             hipStream_t s);
int launch_dasp_analyze(const DaspGeom& g, const uint8_t* bgr, const kde_float3* pts, const int32_t* labels,
                        kde_superpixel* mean, kde_float3* centers, const float* intr_dev, hipStream_t s);
int launch_dasp_analyze_dual(const DaspGeom& g, int n, const uint8_t* bgr, const kde_float3* pts, const int32_t* labels_a,
                             kde_superpixel* mean_a, kde_float3* centers_a, const int32_t* labels_b, kde_superpixel* mean_b,
                             kde_float3* centers_b, const float* intr_dev, hipStream_t s);

// NormalAdaptiveSuperpixel (nasp_kernels.hip): n frames back to back, per-frame colour / cloud / normals / tables / outputs
struct NaspLaunch {
    DaspGeom g;
    int n;
    const uint8_t* bgr;            // [n][H][W][3]
    const kde_float3* pts;         // [n][H][W] millimetres
    const kde_float3* nrm;         // [n][H][W]
    kde_label_distance* ld;        // [n][H][W]
    int32_t* labels;               // [n][H][W]
    kde_superpixel* mean;          // [n][rows*cols]
    kde_float3* centers;           // [n][rows*cols]
    kde_float3* spn;               // [n][rows*cols] superpixel normals
    float* variance;               // [n][rows*cols]
    const float* intr;             // 9 floats
    const float* ctab;             // NA4: colour weight by integer colour distance, ctab_n entries (0 beyond)
    const float* stab;             // NA4: spatial weight by integer squared pixel distance, stab_n entries (0 beyond)
    int ctab_n, stab_n;
    float kc, ks, kd, kn;          // (sigma / sum of sigmas)^2 as .cu:256-258 forms them
    float win2;                    // ((wx + wy) / 2)^2
    float acos_thr;                // NA3
    int reset_on;                  // depth_sigma != 0 || normal_sigma != 0 (.cu:349)
};
int launch_nasp_sample(const NaspLaunch& a, hipStream_t s);
int launch_nasp_init_ld(const NaspLaunch& a, hipStream_t s);    // initLD_NASP alone, for iteration = 0
int launch_nasp_calc_ld(const NaspLaunch& a, bool first, hipStream_t s);
int launch_nasp_clusters(const NaspLaunch& a, hipStream_t s);   // analyzeClusters_NASP + calculateWeightedAverage

// LabelEquivalenceSeg::labelImage (les_kernels.hip): n frames back to back; per-superpixel inputs and tables are strided by nc
constexpr int kLesMaxClusters = 2048;   // the graph step keeps its per-superpixel tables in LDS (56 KB at 2048)
struct LesLaunch {
    int width, height, n;
    int nc, wpr;                   // superpixels per frame (L1), adjacency words per row = ceil(nc / 32)
    const kde_float3* normals;     // [n][nc]
    const int32_t* labels;         // [n][H][W]
    const kde_float3* centers;     // [n][nc]
    int32_t* count;                // [n][nc] pixels per superpixel; all zero between calls, like adj
    uint32_t* adj;                 // [n][nc][wpr] bit B of row A: some pixel of A has an L2-neighbour in B
    int32_t* list;                 // [n][nc * wpr] indices of the adjacency words that kept a bit
    int32_t* mfin;                 // [n][nc] merged label per superpixel after the rounds and countKernel's test
    float4* mnd;                   // [n][nc] merged (n, d) by merged label
    int32_t* merged_label;         // [n][H][W]
    float4* merged_nd;             // [n][H][W]
    float* variance;               // [n][nc] by merged label
    int32_t* size;                 // [n][nc] by merged label
    int iterations;
    float thr, max_dist;           // L6 threshold of max_angle; max_plane_distance
};
int launch_les_label_image(const LesLaunch& a, hipStream_t s);   // 3 kernels

// Projection_GPU::PlaneProjection, five-argument overload (proj_kernels.hip): n frames back to back; the two tables are
// strided by nc, the rays and the spatial table belong to the camera / the handle
constexpr int kProjMaxWindow = 15;
struct ProjLaunch {
    int width, height, n;
    int nc;                        // entries per frame of variance / size (P1)
    const float4* nd;              // [n][H][W] merged (n, d) per pixel
    const int32_t* labels;         // [n][H][W] merged label
    const float* variance;         // [n][nc] by merged label
    const kde_float3* pts;         // [n][H][W] millimetres
    const int32_t* size;           // [n][nc] by merged label
    const float2* nxy;             // [H][W] x, y of the unit-depth ray (initTemp)
    const float* spatial;          // window^2 (calcSpatialFilter)
    kde_float3* plane_fitted;      // [n][H][W]
    float* z;                      // [n][H][W] z as variance_optimization leaves it
    kde_float3* optimized;         // [n][H][W]
    int window, min_size;
    float thr;                     // P3: the L6 threshold of max_angle
    float depth_den;               // 2 * depth_sigma^2 as .cu:231 forms it
};
int launch_proj_plane_projection(const ProjLaunch& a, hipStream_t s);   // 2 kernels

int launch_ers_edge_phase(int width, int height, int dir, int window, const int32_t* color_labels, const int32_t* l0,
                          const float* d0, int32_t* l1, float* d1, hipStream_t s);
int launch_ers_edge_refining(int width, int height, int n, int window, const int32_t* color_labels, const int32_t* l0,
                             const float* d0, int32_t* scratch_l, float* scratch_d, int32_t* l2, float* d2, bool two_launches,
                             hipStream_t s);
int launch_ers_enhance(int width, int height, int n, const float* rd, const uint8_t* bgr, const int32_t* labels,
                       const float* s_eff, const float* table_host, int window, float color_sigma, float depth_sigma,
                       float exp_zero, float* out, int variant, hipStream_t s);

// NormalMapGenerator (normal_kernels.hip): one fixed launch sequence per batch of n frames of millimetre points
struct NormalsLaunch {
    int width, height, n, method;   // KDE_NORMALS_CM or KDE_NORMALS_BILATERAL
    float factor, smoothing;        // max_depth_change_factor, normal_smoothing_size
    const kde_float3* pts;          // [n][H][W] millimetres
    kde_float3* out;                // [n][H][W] normals
    float* fs;                      // [n][H][W] final smoothing map (CM)
    uint8_t* dci;                   // [n][H][W] depth-change map (CM)
    int* cmax;                      // [n] ordered-int key of the largest DDSA (CM)
    float* dt_scratch;              // normals_dt_bands(H) * n * 2 * W floats (CM)
    uint32_t* cnt;                  // [chunk_frames][H][W] integral of z != 0 (CM)
    double* sums;                   // [9][chunk_frames][H][W] integrals of x, y, z and the products (CM)
    int chunk_frames;
};
int normals_dt_bands(int height);
int normals_chunk_frames(int width, int height, int max_batch);
int launch_normals(const NormalsLaunch& a, hipStream_t s);

int launch_spdsr_init_normalized(const Camera& c, float* nxy, hipStream_t s);
int launch_spdsr_cluster_planes(int width, int height, int n, int nclusters, int table_frames, const int32_t* labels,
                                const kde_float3* pts, double* sums, double* cov, float* nd, int* moments_dirty, hipStream_t s);
int launch_spdsr_plane_projection(int width, int height, int n, int nclusters, const float* nd, const int32_t* labels,
                                  const kde_float3* pts, const float* nxy, kde_float3* plane_fitted, kde_float3* opt_a,
                                  kde_float3* opt_b, int sweeps, kde_float3** result, hipStream_t s);

}  // namespace kde
