// kde_api_pipeline.cpp — the pipeline objects: RegionGrowingBilateralFilter (kde_rgbf_*) and SPDepthSuperResolution
// (kde_spdsr_*), both a Pipeline (kde_handles.h) of two private segmenters and the refiner of kde_api_dasp_ers.cpp.
#include "kde_handles.h"

// =====================================================================================================
// Pipeline
// =====================================================================================================
Pipeline::~Pipeline()
{
    kde_dasp_destroy(SP);
    kde_dasp_destroy(DASP);
    kde_ers_destroy(ERS);
}

int Pipeline::init(int w, int h, int batch)
{
    width = w;
    height = h;
    max_batch = batch;
    KDE_TRY(dasp_create_impl(&DASP, w, h, batch));
    KDE_TRY(dasp_create_impl(&SP, w, h, batch));
    DASP->skip_trailing_analyze = SP->skip_trailing_analyze = true;
    KDE_TRY(ers_create_impl(&ERS, w, h, batch));
    return KDE_OK;
}

int Pipeline::run(int n, const float* depth, const kde_float3* pts, const uint8_t* bgr, float c1, float s1, float d1, float c2,
                  float s2, float d2, int iters, void* stream)
{
    KDE_REQUIRE(SP->set && DASP->set, "Process: SetParametor was not called");
    KDE_REQUIRE(bgr && pts && depth, "Process: null argument");
    KDE_ON_DEVICE(SP, "Process");
    KDE_REQUIRE(n >= 1 && n <= max_batch, "Process: n=%d outside 1..max_batch=%d", n, max_batch);
    // SP->Segmentation(...) and DASP->Segmentation(...) (RegionGrowingBilateralFilter.cpp:28-29) run on the same
    // colour + cloud with the same grid, so they share the work that does not depend on the sigmas:
    // sampleInitialClusters is computed once (its result is identical for both) and every assignment step
    // labels both maps in one pass.  Per-object results are exactly those of two separate Segmentation calls.
    hipStream_t s = as_stream(stream);
    const DaspGeom& g = SP->g;
    // The first assignment step reads the sampled clusters once for both segmenters and forms init_LD's
    // assignment in registers (calc_ld_kernel<.., FIRST>); DASP's own copy of the sampled clusters is only
    // needed as the starting point of its first analyzeClusters, i.e. when there is more than one iteration.
    // (the sampling kernel writes that copy itself: no device-to-device copies between the launches)
    KDE_TRY(launch_dasp_sample(g, n, bgr, pts, SP->mean.p, SP->centers.p, iters > 1 ? DASP->mean.p : nullptr,
                               iters > 1 ? DASP->centers.p : nullptr, s));
    const float sa[3] = {c1, s1, d1}, sb[3] = {c2, s2, d2};
    for (int i = 0; i < iters; i++) {
        // the (distance, label) records are only read by a LATER assignment step: the last step does not store them
        // (the private segmenters of a pipeline expose labels only)
        KDE_TRY(launch_dasp_calc_ld_dual(g, n, bgr, pts, SP->ld.p, SP->mean.p, SP->centers.p, SP->labels.p, sa, DASP->ld.p,
                                         DASP->mean.p, DASP->centers.p, DASP->labels.p, sb, i == 0, /*write_ld=*/i < iters - 1, s));
        if (i == iters - 1) break;   // the trailing analyzeClusters is dead for the private segmenters
        // both objects got the same intrinsics in SetParametor, so one launch updates both cluster sets
        KDE_TRY(launch_dasp_analyze_dual(g, n, bgr, pts, SP->labels.p, SP->mean.p, SP->centers.p, DASP->labels.p,
                                         DASP->mean.p, DASP->centers.p, SP->intr.p, s));
    }
    return ers_edge_refining_n(ERS, n, SP->labels.p, DASP->labels.p, depth, bgr, stream);
}

struct kde_rgbf {
    Pipeline p;
};

// max_batch frames per call (kde_rgbf_process_batch); the reference's constructor is max_batch = 1
extern "C" int kde_rgbf_create_batch(kde_rgbf** out, int width, int height, int max_batch)
{
    KDE_REQUIRE(out, "kde_rgbf_create: null out");
    *out = nullptr;
    kde_rgbf* h = new (std::nothrow) kde_rgbf;
    if (!h) return fail(KDE_ERR_NOMEM, "kde_rgbf_create: out of host memory");
    int rc = h->p.init(width, height, max_batch);
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_rgbf_create(kde_rgbf** out, int width, int height) { return kde_rgbf_create_batch(out, width, height, 1); }

extern "C" int kde_rgbf_destroy(kde_rgbf* h) { delete h; return KDE_OK; }

extern "C" int kde_rgbf_set_parameters(kde_rgbf* h, int rows, int cols, const double* K)
{
    KDE_REQUIRE(h, "kde_rgbf_set_parameters: null handle");
    KDE_TRY(kde_dasp_set_parameters(h->p.SP, rows, cols, K));      // RegionGrowingBilateralFilter.cpp:24
    return kde_dasp_set_parameters(h->p.DASP, rows, cols, K);      // :25
}

extern "C" int kde_rgbf_process_batch(kde_rgbf* h, int n, const float* depth_dev, const kde_float3* points_dev,
                                      const uint8_t* bgr_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev && points_dev && bgr_dev, "kde_rgbf_process: null argument");
    // RegionGrowingBilateralFilter.cpp:28-31, per frame
    return h->p.run(n, depth_dev, points_dev, bgr_dev, 200.0f, 40.0f, 0.0f, 100.0f, 20.0f, 200.0f, 1, stream);
}

extern "C" int kde_rgbf_process(kde_rgbf* h, const float* depth_dev, const kde_float3* points_dev, const uint8_t* bgr_dev, void* stream)
{
    return kde_rgbf_process_batch(h, 1, depth_dev, points_dev, bgr_dev, stream);
}

extern "C" int kde_rgbf_refined_depth_device(kde_rgbf* h, float** out)
{
    KDE_REQUIRE(h, "kde_rgbf_refined_depth_device: null handle");
    return kde_ers_refined_depth_device(h->p.ERS, out);
}

extern "C" int kde_rgbf_refined_depth_host(kde_rgbf* h, void* stream, const float** out)
{
    KDE_REQUIRE(h, "kde_rgbf_refined_depth_host: null handle");
    return kde_ers_refined_depth_host(h->p.ERS, stream, out);
}

extern "C" int kde_rgbf_refined_labels_device(kde_rgbf* h, int32_t** out)
{
    KDE_REQUIRE(h, "kde_rgbf_refined_labels_device: null handle");
    return kde_ers_refined_labels_device(h->p.ERS, out);
}

extern "C" int kde_rgbf_sp_labels_device(kde_rgbf* h, int32_t** out)
{
    KDE_REQUIRE(h, "kde_rgbf_sp_labels_device: null handle");
    return kde_dasp_labels_device(h->p.SP, out);
}

extern "C" int kde_rgbf_dasp_labels_device(kde_rgbf* h, int32_t** out)
{
    KDE_REQUIRE(h, "kde_rgbf_dasp_labels_device: null handle");
    return kde_dasp_labels_device(h->p.DASP, out);
}

struct kde_spdsr {
    Pipeline p;
    kde_dimconv conv;
    int nclusters = 0;
    DevBuf<kde_float3> edge_points;   // EdgeEnhanced3DPoints_Device            [max_batch][H][W]
    DevBuf<float> cluster_nd;         // ClusterND_Device (float4 per cluster)   [max_batch][rows*cols]
    DevBuf<double> sums, cov;         // per-cluster moments (replace the host cv::Mat / cv::PCA round trip)
    int moments_dirty = 0;            // raised while sums / cov hold accumulated moments nobody has consumed (spdsr_kernels.hip)
    DevBuf<float> nxy;                // Projection_GPU::Normalized3D_Device (x, y of the unit-depth ray; the camera's)
    DevBuf<kde_float3> plane_fitted;  // Projection_GPU::PlaneFitted3D_Device    [max_batch][H][W]
    DevBuf<kde_float3> opt_a, opt_b;  // Projection_GPU::Optimized3D_Device, double-buffered (D5)
    kde_float3* optimized = nullptr;
    int n_last = 1;
    PinnedBuf<kde_float3> optimized_host;
};

extern "C" int kde_spdsr_create_batch(kde_spdsr** out, int width, int height, int max_batch)
{
    KDE_REQUIRE(out, "kde_spdsr_create: null out");
    *out = nullptr;
    kde_spdsr* h = new (std::nothrow) kde_spdsr;
    if (!h) return fail(KDE_ERR_NOMEM, "kde_spdsr_create: out of host memory");
    int rc = h->p.init(width, height, max_batch);
    const size_t px = (size_t)width * height;
    if (rc == KDE_OK) rc = h->edge_points.alloc(px * max_batch);   // SPDepthSuperResolution.cpp:19
    if (rc == KDE_OK) rc = h->nxy.alloc(px * 2);                    // Projection_GPU::initMemory (Projection_GPU.cpp:45-51)
    if (rc == KDE_OK) rc = h->plane_fitted.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->opt_a.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->opt_b.alloc(px * max_batch);
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_spdsr_create(kde_spdsr** out, int width, int height) { return kde_spdsr_create_batch(out, width, height, 1); }

extern "C" int kde_spdsr_destroy(kde_spdsr* h) { delete h; return KDE_OK; }

extern "C" int kde_spdsr_set_parameters(kde_spdsr* h, int rows, int cols, const double* K)
{
    KDE_REQUIRE(h, "kde_spdsr_set_parameters: null handle");
    KDE_TRY(kde_dasp_set_parameters(h->p.SP, rows, cols, K));       // SPDepthSuperResolution.cpp:46
    KDE_TRY(kde_dasp_set_parameters(h->p.DASP, rows, cols, K));     // :47
    KDE_TRY(kde_dimconv_set_camera(&h->conv, K, h->p.width, h->p.height));   // :48
    // Projector = new Projection_GPU(Width, Height, intrinsic) (:49): same truncated intrinsics, initNormalized3D
    h->nclusters = rows * cols;
    const size_t kb = (size_t)h->nclusters * h->p.max_batch;
    KDE_TRY(h->cluster_nd.alloc(kb * 4));          // :52-53
    KDE_TRY(h->sums.alloc(kb * 4));
    KDE_TRY(h->cov.alloc(kb * 6));
    // the moment tables are zero between calls: cluster_planes_kernel clears what it has consumed (no memsets per frame)
    KDE_HIP_TRY(hipMemset(h->sums.p, 0, kb * 4 * sizeof(double)));
    KDE_HIP_TRY(hipMemset(h->cov.p, 0, kb * 6 * sizeof(double)));
    KDE_HIP_TRY(hipMemset(h->cluster_nd.p, 0, kb * 4 * sizeof(float)));
    h->moments_dirty = 0;
    KDE_TRY(launch_spdsr_init_normalized(h->conv.cam, h->nxy.p, nullptr));
    KDE_HIP_TRY(hipStreamSynchronize(nullptr));
    return KDE_OK;
}

extern "C" int kde_spdsr_process_batch(kde_spdsr* h, int n, const float* depth_dev, const kde_float3* points_dev,
                                       const uint8_t* bgr_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev && points_dev && bgr_dev, "kde_spdsr_process: null argument");
    // SPDepthSuperResolution.cpp:59-64, per frame
    KDE_REQUIRE(h->nclusters > 0, "kde_spdsr_process: SetParametor was not called");
    KDE_TRY(h->p.run(n, depth_dev, points_dev, bgr_dev, 200.0f, 10.0f, 0.0f, 0.0f, 10.0f, 200.0f, 5, stream));
    KDE_TRY(kde_dimconv_projective_to_real_depth(&h->conv, n, h->p.ERS->refined_depth.p, h->edge_points.p, stream));
    // :65-170 on the device: per-cluster plane of the labelled cloud (no D2H / host PCA / H2D)
    hipStream_t s = as_stream(stream);
    KDE_TRY(launch_spdsr_cluster_planes(h->p.width, h->p.height, n, h->nclusters, h->p.max_batch, h->p.ERS->labels_a.p, h->edge_points.p,
                                        h->sums.p, h->cov.p, h->cluster_nd.p, &h->moments_dirty, s));
    // Projector->PlaneProjection(ClusterND_Device, refined labels, EdgeEnhanced3DPoints_Device) (:190)
    h->n_last = n;
    return launch_spdsr_plane_projection(h->p.width, h->p.height, n, h->nclusters, h->cluster_nd.p, h->p.ERS->labels_a.p,
                                         h->edge_points.p, h->nxy.p, h->plane_fitted.p, h->opt_a.p, h->opt_b.p, 20,
                                         &h->optimized, s);
}

extern "C" int kde_spdsr_process(kde_spdsr* h, const float* depth_dev, const kde_float3* points_dev, const uint8_t* bgr_dev, void* stream)
{
    return kde_spdsr_process_batch(h, 1, depth_dev, points_dev, bgr_dev, stream);
}

#ifdef KDE_STAGE_HOOKS
// include/kde_test_hooks.h: exists only in tools/hooks/libkde_hip_stage.so.  What kde_spdsr_process_batch runs after the
// back-projection, on the caller's labels and cloud (and, if given, the caller's planes instead of the fit).
extern "C" int kde_stage_spdsr_tail(kde_spdsr* h, int n, const int32_t* labels_dev, const kde_float3* points_dev,
                                    const float* nd_dev_or_null, int sweeps, void* stream)
{
    KDE_REQUIRE(h && labels_dev && points_dev, "kde_stage_spdsr_tail: null argument");
    KDE_REQUIRE(h->nclusters > 0, "kde_stage_spdsr_tail: SetParametor was not called");
    KDE_ON_DEVICE(h->p.SP, "kde_stage_spdsr_tail");
    KDE_REQUIRE(n >= 1 && n <= h->p.max_batch, "kde_stage_spdsr_tail: n=%d outside 1..max_batch=%d", n, h->p.max_batch);
    KDE_REQUIRE(sweeps >= 0, "kde_stage_spdsr_tail: sweeps=%d is negative", sweeps);
    hipStream_t s = as_stream(stream);
    if (nd_dev_or_null)
        KDE_HIP_TRY(hipMemcpyAsync(h->cluster_nd.p, nd_dev_or_null, (size_t)n * h->nclusters * 4 * sizeof(float),
                                   hipMemcpyDeviceToDevice, s));
    else
        KDE_TRY(launch_spdsr_cluster_planes(h->p.width, h->p.height, n, h->nclusters, h->p.max_batch, labels_dev, points_dev,
                                            h->sums.p, h->cov.p, h->cluster_nd.p, &h->moments_dirty, s));
    h->n_last = n;
    return launch_spdsr_plane_projection(h->p.width, h->p.height, n, h->nclusters, h->cluster_nd.p, labels_dev, points_dev,
                                         h->nxy.p, h->plane_fitted.p, h->opt_a.p, h->opt_b.p, sweeps, &h->optimized, s);
}
#endif

extern "C" int kde_spdsr_refined_depth_device(kde_spdsr* h, float** out)
{
    KDE_REQUIRE(h, "kde_spdsr_refined_depth_device: null handle");
    return kde_ers_refined_depth_device(h->p.ERS, out);
}

extern "C" int kde_spdsr_refined_depth_host(kde_spdsr* h, void* stream, const float** out)
{
    KDE_REQUIRE(h, "kde_spdsr_refined_depth_host: null handle");
    return kde_ers_refined_depth_host(h->p.ERS, stream, out);
}

extern "C" int kde_spdsr_refined_labels_device(kde_spdsr* h, int32_t** out)
{
    KDE_REQUIRE(h, "kde_spdsr_refined_labels_device: null handle");
    return kde_ers_refined_labels_device(h->p.ERS, out);
}

KDE_DEVICE_GETTER(kde_spdsr_edge_enhanced_points_device, kde_spdsr, kde_float3, h->edge_points.p)
KDE_DEVICE_GETTER(kde_spdsr_plane_fitted_points_device, kde_spdsr, kde_float3, h->plane_fitted.p)
KDE_DEVICE_GETTER(kde_spdsr_cluster_nd_device, kde_spdsr, float, h->cluster_nd.p)

extern "C" int kde_spdsr_optimized_points_device(kde_spdsr* h, kde_float3** out)
{
    KDE_REQUIRE(h && out, "kde_spdsr_optimized_points_device: null argument");
    KDE_REQUIRE(h->optimized, "getOptimizedPoints: Process has not run yet");
    *out = h->optimized;
    return KDE_OK;
}

extern "C" int kde_spdsr_optimized_points_host(kde_spdsr* h, void* stream, const kde_float3** out)
{
    KDE_REQUIRE(h && out, "kde_spdsr_optimized_points_host: null argument");
    KDE_REQUIRE(h->optimized, "getOptimizedPoints: Process has not run yet");
    const size_t px = (size_t)h->p.width * h->p.height;
    return host_mirror("kde_spdsr_optimized_points_host", h->p.SP->device, h->optimized, px * h->n_last, px * h->p.max_batch,
                       h->optimized_host, as_stream(stream), out);
}
