// kde_api_dasp_ers.cpp — DepthAdaptiveSuperpixel (kde_dasp_*) and EdgeRefinedSuperpixel (kde_ers_*).  Both structs are in
// kde_handles.h: the pipeline objects of kde_api_pipeline.cpp own two segmenters and a refiner and drive them batched.
#include "kde_handles.h"

// =====================================================================================================
// DepthAdaptiveSuperpixel
// =====================================================================================================
int kde::dasp_create_impl(kde_dasp** out, int width, int height, int max_batch)
{
    KDE_REQUIRE(out, "kde_dasp_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_dasp_create", width, height, max_batch, "create"));
    kde_dasp* h = new_handle<kde_dasp>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_dasp_create: out of host memory");
    const size_t px = (size_t)width * height * max_batch;
    int rc = h->labels.alloc(px);                 // SuperpixelSegmentation.cpp (ctor)
    if (rc == KDE_OK) rc = h->ld.alloc(px);
    if (rc == KDE_OK) rc = h->intr.alloc(9);      // DepthAdaptiveSuperpixel.cpp:6
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_dasp_create(kde_dasp** out, int width, int height) { return dasp_create_impl(out, width, height, 1); }

extern "C" int kde_dasp_destroy(kde_dasp* h) { delete h; return KDE_OK; }

extern "C" int kde_dasp_set_parameters(kde_dasp* h, int rows, int cols, const double* K)
{
    KDE_REQUIRE(h && K, "kde_dasp_set_parameters: null argument");
    KDE_ON_DEVICE(h, "kde_dasp_set_parameters");
    DaspGeom g;
    KDE_TRY(superpixel_geometry(h->width, h->height, rows, cols, 4, &g));
    const size_t k = (size_t)rows * cols * h->max_batch;
    KDE_TRY(h->mean.alloc(k));       // initMemory, DepthAdaptiveSuperpixel.cpp:40-50
    KDE_TRY(h->centers.alloc(k));
    KDE_HIP_TRY(hipMemset(h->mean.p, 0, k * sizeof(kde_superpixel)));
    KDE_HIP_TRY(hipMemset(h->centers.p, 0, k * sizeof(kde_float3)));
    // what a call of no iteration leaves where the reference's buffers are uninitialised: labels 0 (and LD 0 until a call)
    const size_t px = (size_t)h->width * h->height * h->max_batch;
    KDE_HIP_TRY(hipMemset(h->ld.p, 0, px * sizeof(kde_label_distance)));
    KDE_HIP_TRY(hipMemset(h->labels.p, 0, px * sizeof(int32_t)));
    float intr[9];
    for (int i = 0; i < 9; i++) intr[i] = (float)K[i];   // DepthAdaptiveSuperpixel.cpp:33-37
    KDE_HIP_TRY(hipMemcpy(h->intr.p, intr, sizeof(intr), hipMemcpyHostToDevice));
    h->g = g;
    h->set = true;
    return KDE_OK;
}

extern "C" int kde_dasp_segmentation(kde_dasp* h, const uint8_t* bgr_dev, const kde_float3* points_dev,
                                     float color_sigma, float spatial_sigma, float depth_sigma, int iteration, void* stream)
{
    KDE_REQUIRE(h && bgr_dev && points_dev, "kde_dasp_segmentation: null argument");
    KDE_ON_DEVICE(h, "kde_dasp_segmentation");
    KDE_REQUIRE(h->set, "kde_dasp_segmentation: SetParametor was not called");
    KDE_REQUIRE(iteration >= 0, "kde_dasp_segmentation: negative iteration count");
    // the weights are (sigma / sum of sigmas)^2 (.cu:209-217): a zero sum is 0/0 in the reference
    KDE_REQUIRE(spatial_sigma + color_sigma + depth_sigma != 0.0f, "kde_dasp_segmentation: the sigmas must not sum to zero");
    hipStream_t s = as_stream(stream);
    // DepthAdaptiveSuperpixel.cu:570-586
    // init_LD (K5) is folded into the first calculateLD: its output is only ever read there
    KDE_TRY(launch_dasp_sample(h->g, 1, bgr_dev, points_dev, h->mean.p, h->centers.p, nullptr, nullptr, s));
    if (iteration == 0) KDE_TRY(launch_dasp_init_ld(h->g, h->ld.p, s));      // no first calculateLD to form the initial LD in
    for (int i = 0; i < iteration; i++) {
        KDE_TRY(launch_dasp_calc_ld(h->g, bgr_dev, points_dev, h->ld.p, h->mean.p, h->centers.p, h->labels.p,
                                    color_sigma, spatial_sigma, depth_sigma, i == 0, s));
        if (h->skip_trailing_analyze && i == iteration - 1) break;
        KDE_TRY(launch_dasp_analyze(h->g, bgr_dev, points_dev, h->labels.p, h->mean.p, h->centers.p, h->intr.p, s));
    }
    return KDE_OK;
}

KDE_DEVICE_GETTER(kde_dasp_labels_device, kde_dasp, int32_t, h->labels.p)
KDE_DEVICE_GETTER(kde_dasp_mean_device, kde_dasp, kde_superpixel, h->mean.p)
KDE_DEVICE_GETTER(kde_dasp_centers_device, kde_dasp, kde_float3, h->centers.p)
KDE_DEVICE_GETTER(kde_dasp_ld_device, kde_dasp, kde_label_distance, h->ld.p)

// the *_Host getters of a kde_dasp mirror one frame: only the private segmenters of a pipeline hold more
extern "C" int kde_dasp_labels_host(kde_dasp* h, void* stream, const int32_t** out)
{
    KDE_REQUIRE(h && out, "kde_dasp_labels_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    return host_mirror("kde_dasp_labels_host", h->device, h->labels.p, px, px, h->labels_host, as_stream(stream), out);
}

extern "C" int kde_dasp_mean_host(kde_dasp* h, void* stream, const kde_superpixel** out, int* count)
{
    KDE_REQUIRE(h && out && count, "kde_dasp_mean_host: null argument");
    KDE_REQUIRE(h->set, "kde_dasp_mean_host: SetParametor has not been called");
    const size_t nc = (size_t)h->g.rows * h->g.cols;
    KDE_TRY(host_mirror("kde_dasp_mean_host", h->device, h->mean.p, nc, nc, h->mean_host, as_stream(stream), out));
    *count = (int)nc;
    return KDE_OK;
}

// =====================================================================================================
// EdgeRefinedSuperpixel
// =====================================================================================================
int kde::ers_create_impl(kde_ers** out, int width, int height, int max_batch)
{
    KDE_REQUIRE(out, "kde_ers_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_ers_create", width, height, max_batch, "create"));
    kde_ers* h = new_handle<kde_ers>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_ers_create: out of host memory");
    h->exp_zero = exp_zero_threshold();
    const size_t px = (size_t)width * height;
    float table[49];
    spatial_table(kde_ers::WindowSize, kde_ers::SpatialSigma, table);
    memcpy(h->table_host, table, sizeof(table));
    for (float& v : table)
        if (v == 0.0f) v = 1.0f;
    int rc = h->s_eff.alloc(49);
    if (rc == KDE_OK) rc = h->labels_a.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->labels_b.alloc(px);
    if (rc == KDE_OK) rc = h->depth_a.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->depth_b.alloc(px);
    if (rc == KDE_OK) rc = h->refined_depth.alloc(px * max_batch);
    if (rc == KDE_OK && hipMemcpy(h->s_eff.p, table, sizeof(table), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(KDE_ERR_HIP, "kde_ers_create: table upload failed");
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_ers_create(kde_ers** out, int width, int height) { return ers_create_impl(out, width, height, 1); }

extern "C" int kde_ers_destroy(kde_ers* h) { delete h; return KDE_OK; }

int kde::ers_edge_refining_n(kde_ers* h, int n, const int32_t* color_labels_dev, const int32_t* depth_labels_dev,
                             const float* depth_dev, const uint8_t* bgr_dev, void* stream)
{
    KDE_REQUIRE(h && color_labels_dev && depth_labels_dev && depth_dev && bgr_dev, "kde_ers_edge_refining: null argument");
    KDE_ON_DEVICE(h, "kde_ers_edge_refining");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "EdgeRefining: n=%d outside 1..max_batch=%d", n, h->max_batch);
    hipStream_t s = as_stream(stream);
    const int W = h->width, H = h->height;
    // EdgeRefinedSuperpixel.cu:210-211 copies labels/depth, then edge_refining works in place; here the
    // horizontal phase reads the caller's buffers and the vertical phase reads the horizontal result (kept in
    // LDS by the fused kernel), so the two D2D copies disappear.
    KDE_TRY(launch_ers_edge_refining(W, H, n, kde_ers::WindowSize, color_labels_dev, depth_labels_dev, depth_dev,
                                     h->labels_b.p, h->depth_b.p, h->labels_a.p, h->depth_a.p,
                                     /*two_launches=*/h->enhance_variant == 3, s));
    // depthmap_enhancement (.cu:220-221)
    KDE_TRY(launch_ers_enhance(W, H, n, h->depth_a.p, bgr_dev, h->labels_a.p, h->s_eff.p, h->table_host,
                               kde_ers::WindowSize, kde_ers::ColorSigma, kde_ers::DepthSigma, h->exp_zero,
                               h->refined_depth.p, h->enhance_variant, s));
    h->n_last = n;
    return KDE_OK;
}

extern "C" int kde_ers_edge_refining(kde_ers* h, const int32_t* color_labels_dev, const int32_t* depth_labels_dev,
                                     const float* depth_dev, const uint8_t* bgr_dev, void* stream)
{
    return ers_edge_refining_n(h, 1, color_labels_dev, depth_labels_dev, depth_dev, bgr_dev, stream);
}

extern "C" int kde_ers_set_variant(kde_ers* h, int variant)
{
    KDE_REQUIRE(h, "kde_ers_set_variant: null handle");
    KDE_REQUIRE(variant >= 0 && variant <= 3, "kde_ers_set_variant: variant %d out of range (0..3)", variant);
    h->enhance_variant = variant;
    return KDE_OK;
}

KDE_DEVICE_GETTER(kde_ers_stage_edge_depth_device, kde_ers, float, h->depth_a.p)
KDE_DEVICE_GETTER(kde_ers_refined_labels_device, kde_ers, int32_t, h->labels_a.p)
KDE_DEVICE_GETTER(kde_ers_refined_depth_device, kde_ers, float, h->refined_depth.p)

// the *_Host getters mirror the frames the last call produced (one for the reference's single-frame calls)
extern "C" int kde_ers_refined_labels_host(kde_ers* h, void* stream, const int32_t** out)
{
    KDE_REQUIRE(h && out, "kde_ers_refined_labels_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    return host_mirror("kde_ers_refined_labels_host", h->device, h->labels_a.p, px * h->n_last, px * h->max_batch, h->labels_host,
                       as_stream(stream), out);
}

extern "C" int kde_ers_refined_depth_host(kde_ers* h, void* stream, const float** out)
{
    KDE_REQUIRE(h && out, "kde_ers_refined_depth_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    return host_mirror("kde_ers_refined_depth_host", h->device, h->refined_depth.p, px * h->n_last, px * h->max_batch,
                       h->depth_host, as_stream(stream), out);
}
