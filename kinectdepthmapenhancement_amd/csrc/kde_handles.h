// kde_handles.h — what the kde_api*.cpp files share (no .hip file includes this): the rules every handle follows
// (device ownership, create() bounds, host mirrors, device getters, superpixel geometry) and the handle structs that
// another handle reads.  A handle that nobody else looks into is defined in its own .cpp.
#pragma once

#include "kde_internal.h"

#include <algorithm>
#include <cfloat>
#include <climits>

namespace kde {

// ---- device ownership ---------------------------------------------------------------------------------
// A handle belongs to the device that was current when it was created (its buffers live there).  Calls made while
// another device is current are rejected instead of launching kernels on the wrong device's memory.
inline int current_device()
{
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return d;
}

inline int check_on_device(int device, const char* who)
{
    const int cur = current_device();
    if (cur != device)
        return fail(KDE_ERR_INVALID, "%s: the handle was created on device %d but device %d is current (kde_set_device)", who,
                    device, cur);
    return KDE_OK;
}
#define KDE_ON_DEVICE(h, who) KDE_TRY(check_on_device((h)->device, who))

// ---- create() -----------------------------------------------------------------------------------------
inline bool frame_ok(int width, int height) { return width >= 1 && height >= 1 && (long long)width * height <= (1ll << 30); }
inline bool batch_ok(int max_batch) { return max_batch >= 1 && max_batch <= 65535; }

// The frame / batch bounds of a create().  batch_who: the prefix of the max_batch message where it is not who.
inline int check_frame_batch(const char* who, int width, int height, int max_batch, const char* batch_who = nullptr)
{
    KDE_REQUIRE(frame_ok(width, height), "%s: bad size", who);
    KDE_REQUIRE(batch_ok(max_batch), "%s: max_batch must be in 1..65535", batch_who ? batch_who : who);
    return KDE_OK;
}

// A handle of the current device for max_batch frames of width x height; nullptr when the host is out of memory.
template <typename H>
H* new_handle(int width, int height, int max_batch)
{
    H* h = new (std::nothrow) H;
    if (!h) return nullptr;
    h->device = current_device();
    h->width = width;
    h->height = height;
    h->max_batch = max_batch;
    return h;
}

// ---- getters ------------------------------------------------------------------------------------------
// A *_Host member of the reference: `count` elements of the handle's own device buffer copied into pinned memory that
// holds `capacity` elements (allocated on first use, for the handle's max_batch), ready when the call returns.
template <typename T>
int host_mirror(const char* who, int device, const T* dev, size_t count, size_t capacity, PinnedBuf<T>& host, hipStream_t s,
                const T** out)
{
    KDE_TRY(check_on_device(device, who));
    KDE_TRY(host.ensure(capacity));
    KDE_HIP_TRY(hipMemcpyAsync(host.p, dev, count * sizeof(T), hipMemcpyDeviceToHost, s));
    KDE_HIP_TRY(hipStreamSynchronize(s));
    *out = host.p;
    return KDE_OK;
}

// extern "C" int fn(handle* h, type** out): a device pointer the handle owns
#define KDE_DEVICE_GETTER(fn, handle, type, expr)       \
    extern "C" int fn(handle* h, type** out)            \
    {                                                   \
        KDE_REQUIRE(h && out, #fn ": null argument");   \
        *out = (expr);                                  \
        return KDE_OK;                                  \
    }

// ---- SetParametor -------------------------------------------------------------------------------------
// rows x cols superpixels on a width x height frame (DepthAdaptiveSuperpixel.cpp:19-21); min_window is the side of the
// candidate grid a cluster's window must hold: 4 (DASP) or 8 (NASP)
inline int superpixel_geometry(int width, int height, int rows, int cols, int min_window, DaspGeom* g)
{
    KDE_REQUIRE(rows >= 1 && cols >= 1, "SetParametor: rows and cols must be >= 1");
    const int wx = width / cols, wy = height / rows;
    const int m = min_window;
    KDE_REQUIRE(wx >= m && wy >= m, "SetParametor: window %dx%d < %dx%d (the %dx%d candidate grid would leave the %s)", wx, wy, m,
                m, m, m, m == 4 ? "image" : "window");
    KDE_REQUIRE(width / wx == cols, "SetParametor: width/(width/cols) != cols (cluster table would be indexed out of bounds)");
    KDE_REQUIRE(height >= 6, "SetParametor: height must be >= 6");
    g->width = width; g->height = height; g->rows = rows; g->cols = cols; g->wx = wx; g->wy = wy;
    return KDE_OK;
}

}  // namespace kde

#include "kde_depth_stage.h"   // the depth-in / depth-out stages: what their four handles and entry points share

using namespace kde;

// =====================================================================================================
// handles that other handles read (the C ABI names them, so they are not in the namespace)
// =====================================================================================================
struct kde_jbf {                    // kde_api_jbf.cpp
    int device = -1;                // hipGetDevice() at creation
    int width = 0, height = 0, max_batch = 1;
    kde_jbf_params p{};
    std::vector<float> table;       // SpatialFilter_Host
    DevBuf<float> s_eff;            // SpatialFilter_Device (zeros replaced by 1: "skip the factor")
    DevBuf<float> log2_pk;          // windows 23..31: the packed kernels' log2(S) pairs (too large for the kernel-argument block)
    DevBuf<float> filtered;         // Filtered_Device
    DevBuf<uint8_t> smooth;         // smooth_Device
    DevBuf<float> pre_lut;          // K0 weight table
    PinnedBuf<float> filtered_host; // Filtered_Host
    int pre_radius = 0;
    long long pre_grid_cap = 0;     // persistent-grid size of K0 on the device this handle was created on
    float color_den = 0, depth_den = 0;
    int cd_skip = INT_MAX;
    float d2_skip = INFINITY;
    int variant = -1;
    int n_last = 0;                 // frames of the last call that wrote Filtered_Device (0: none yet)
};

struct kde_dimconv {                // kde_api_dimconv.cpp
    Camera cam{};
    bool set = false;
};

struct kde_dasp {                        // kde_api_dasp_ers.cpp
    int device = -1;
    int width, height;
    int max_batch = 1;                   // > 1 only for the private segmenters of a batched pipeline object
    bool set = false;
    DaspGeom g{};
    DevBuf<int32_t> labels;              // Labels_Device                [max_batch][H][W]
    DevBuf<kde_label_distance> ld;       // LD_Device                    [max_batch][H][W]
    DevBuf<kde_superpixel> mean;         // meanData_Device              [max_batch][rows*cols]
    DevBuf<kde_float3> centers;          // superpixelCenters_Device     [max_batch][rows*cols]
    DevBuf<float> intr;                  // intrinsicDevice
    PinnedBuf<int32_t> labels_host;      // Labels_Host
    PinnedBuf<kde_superpixel> mean_host; // meanData_Host
    // Set by the pipeline objects (RGBF / SPDSR) for their PRIVATE segmenters: the analyzeClusters that
    // follows the last calculateLD only refreshes mean/centres, which nothing reads before the next
    // Segmentation re-samples them (DepthAdaptiveSuperpixel.cu:576-586) and which the pipelines do not expose.
    bool skip_trailing_analyze = false;
};
namespace kde {
int dasp_create_impl(kde_dasp** out, int width, int height, int max_batch);
}

struct kde_ers {                          // kde_api_dasp_ers.cpp
    int device = -1;
    int width, height;
    int max_batch = 1;                    // > 1 only inside a batched pipeline object
    int n_last = 1;                       // frames of the last EdgeRefining
    static constexpr int WindowSize = 7;            // EdgeRefinedSuperpixel.cpp:4
    static constexpr float SpatialSigma = 30.0f;    // :5
    static constexpr float ColorSigma = 50.0f;      // :6
    static constexpr float DepthSigma = 70.0f;      // :7
    DevBuf<float> s_eff;                  // SpatialFilter_Device
    DevBuf<int32_t> labels_a, labels_b;   // refinedLabels_Device [max_batch] + one frame of phase scratch
    DevBuf<float> depth_a, depth_b;       // K9 result [max_batch] + one frame of phase scratch
    DevBuf<float> refined_depth;          // refinedDepth_Device [max_batch]
    PinnedBuf<int32_t> labels_host;
    PinnedBuf<float> depth_host;
    float exp_zero = 0;
    float table_host[49];                 // SpatialFilter_Host as calcSpatialFilter computed it
    int enhance_variant = 0;              // kde_ers_set_variant
};
namespace kde {
int ers_create_impl(kde_ers** out, int width, int height, int max_batch);
// n frames back to back in every argument (n = 1: the reference's call)
int ers_edge_refining_n(kde_ers* h, int n, const int32_t* color_labels_dev, const int32_t* depth_labels_dev,
                        const float* depth_dev, const uint8_t* bgr_dev, void* stream);

// RegionGrowingBilateralFilter / SPDepthSuperResolution: two private segmenters and the refiner (kde_api_pipeline.cpp)
struct Pipeline {
    int width = 0, height = 0, max_batch = 1;
    kde_dasp* SP = nullptr;     // colour segmentation
    kde_dasp* DASP = nullptr;   // depth-adaptive segmentation
    kde_ers* ERS = nullptr;
    ~Pipeline();
    int init(int w, int h, int batch);
    // n frames back to back in depth / pts / bgr.  Every kernel of the chain takes the whole batch in one launch
    // (blockIdx -> (frame, tile); per-frame cluster tables, label maps and outputs), so a batch costs the same four
    // launches as one frame and each frame's result is bit-identical to its single-frame call.
    int run(int n, const float* depth, const kde_float3* pts, const uint8_t* bgr, float c1, float s1, float d1, float c2,
            float s2, float d2, int iters, void* stream);
};
}  // namespace kde

struct kde_normals {                    // kde_api_normals.cpp
    int device = -1;
    int width = 0, height = 0, max_batch = 1;
    kde_normals_params p{};
    int chunk_frames = 1;               // frames per pass of the integral-image stage
    DevBuf<kde_float3> normals;         // normalMap (NormalMapGenerator.h:51)
    DevBuf<float> fs;                   // finalSmoothingMap (SmoothingAreaMapGenerator.h:41)
    DevBuf<uint8_t> dci;                // depthChangeIndicationMap (:38)
    DevBuf<int> cmax;                   // per frame: the largest DDSA, as an ordered int key
    DevBuf<float> dt_scratch;           // two rows per distance-transform workgroup
    DevBuf<uint32_t> cnt;               // IntegralCount (IntegralImageGenerator.h:50)
    DevBuf<double> sums;                // IntegralXYZ, IntegralXXXYXZ, IntegralYYYZZZ as 9 planes
    PinnedBuf<kde_float3> normals_host;
    int n_last = 0;                     // frames of the last call that wrote the object-owned normal map
    bool fs_valid = false;              // the last call ran CM
};

struct kde_nasp {                        // kde_api_nasp.cpp
    int device = -1;
    int width = 0, height = 0, max_batch = 1;
    bool set = false;
    DaspGeom g{};
    int n_last = 1;                      // frames of the last Segmentation
    DevBuf<int32_t> labels;              // Labels_Device                [max_batch][H][W]
    DevBuf<kde_label_distance> ld;       // LD_Device                    [max_batch][H][W]
    DevBuf<kde_superpixel> mean;         // meanData_Device              [max_batch][rows*cols]
    DevBuf<kde_float3> centers;          // superpixelCenters_Device     [max_batch][rows*cols]
    DevBuf<kde_float3> normals;          // superpixelNormals_Device     [max_batch][rows*cols]
    DevBuf<float> variance;              // NormalsVariance_Device       [max_batch][rows*cols]
    DevBuf<float> intr;                  // intrinsicDevice
    // NA4: the weights of the weighted pass by integer numerator, rebuilt on the host when a call's sigma differs from
    // the one the table holds
    static constexpr long long kColorCap = 3 * 255 * 255 + 1;
    static constexpr long long kSpatialCapMax = 1ll << 20;
    long long spatial_need = 0;          // 1 + the largest squared pixel distance of the scan window
    long long spatial_cap = 0;           // entries allocated: min(spatial_need, kSpatialCapMax)
    DevBuf<float> ctab, stab;
    PinnedBuf<float> ctab_host, stab_host;
    int ctab_n = 0, stab_n = 0;
    float ctab_sigma = 0.0f, stab_sigma = 0.0f;
    bool ctab_valid = false, stab_valid = false;
    hipEvent_t uploaded = nullptr;       // the last table upload: the pinned mirrors are rewritten only after it
    float acos_thr = 0.5f;               // NA3
    PinnedBuf<int32_t> labels_host;      // Labels_Host
    PinnedBuf<kde_superpixel> mean_host; // meanData_Host
    PinnedBuf<kde_float3> centers_host;  // superpixelCenters_Host
    PinnedBuf<kde_float3> normals_host;  // superpixelNormals_Host
    PinnedBuf<float> variance_host;      // NormalsVariance_Host
    ~kde_nasp()
    {
        if (uploaded) (void)hipEventDestroy(uploaded);
    }
};
namespace kde {
// NA4: make the device tables those of (color_sigma, spatial_sigma); see kde_api_nasp.cpp
int nasp_tables(kde_nasp* h, float color_sigma, float spatial_sigma, hipStream_t s);
}

struct kde_les {                         // kde_api_les.cpp
    int device = -1;
    int width = 0, height = 0, max_batch = 1;
    int cap = 0;                         // largest n_clusters the buffers hold: min(W*H, kLesMaxClusters)
    kde_les_params p{};
    float thr = 0.0f;                    // L6: the threshold of p.max_angle
    int n_last = 1, nc_last = 0;         // frames and n_clusters of the last labelImage (0: none yet)
    bool dirty = false;                  // a launch failed: counts / adjacency may not be zero
    DevBuf<int32_t> merged_label;        // MergedClusterLabel_Device     [max_batch][H][W]
    DevBuf<float4> merged_nd;            // MergedClusterND_Device        [max_batch][H][W]
    DevBuf<float> variance;              // MergedClusterVariance_Device  [max_batch][cap]
    DevBuf<int32_t> size;                // merged_cluster_size           [max_batch][cap]
    DevBuf<int32_t> scratch;             // counts [n][nc], adjacency [n][nc][wpr]: all zero between calls (any n, nc)
    DevBuf<int32_t> tables;              // word list [n][nc * wpr], merged label per superpixel [n][nc]
    DevBuf<float4> mnd;                  // merged (n, d) by merged label [max_batch][cap]
    PinnedBuf<int32_t> merged_label_host;   // MergedClusterLabel_Host
    PinnedBuf<float4> merged_nd_host;       // MergedClusterND_Host
};

struct kde_proj {                        // kde_api_proj.cpp
    int device = -1;
    int width = 0, height = 0, max_batch = 1;
    kde_proj_params p{};
    float thr = 0.0f;                    // P3: the L6 threshold of p.max_angle
    int n_last = 1;
    DevBuf<float> nxy;                   // Normalized3D_Device (x, y of the unit-depth ray)  [H][W]
    DevBuf<float> spatial;               // SpatialFilter_Device                             window^2
    DevBuf<kde_float3> plane_fitted;     // PlaneFitted3D_Device                             [max_batch][H][W]
    DevBuf<float> z;                     // z of Optimized3D_Device before the filter (P4)   [max_batch][H][W]
    DevBuf<kde_float3> optimized;        // Optimized3D_Device                               [max_batch][H][W]
    PinnedBuf<kde_float3> plane_fitted_host, optimized_host;
};

// KinectDepthEnhancement: the six stage objects in the order of KinectDepthEnhancement.cpp:56-81
struct kde_enh {                         // kde_api_proj.cpp; kde_api_enh_feed.cpp runs it and reads Projector
    int width = 0, height = 0, max_batch = 1;
    int nclusters = 0;                   // rows * cols of SetParametor (0: not called)
    kde_jbf* JBF = nullptr;
    kde_dimconv conv;                    // Convertor
    kde_normals* NormalGenerator = nullptr;
    kde_nasp* NASP = nullptr;
    kde_les* spMerging = nullptr;
    kde_proj* Projector = nullptr;       // created by SetParametor, as in the reference (.cpp:54)
    DevBuf<kde_float3> edge_points;      // EdgeEnhanced3DPoints_Device  [max_batch][H][W]
    ~kde_enh()
    {
        kde_jbf_destroy(JBF);
        kde_normals_destroy(NormalGenerator);
        kde_nasp_destroy(NASP);
        kde_les_destroy(spMerging);
        kde_proj_destroy(Projector);
    }
};
