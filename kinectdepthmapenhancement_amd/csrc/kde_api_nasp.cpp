// kde_api_nasp.cpp — NormalAdaptiveSuperpixel (kde_nasp_*, nasp_kernels.hip).  struct kde_nasp is in kde_handles.h: the
// KinectDepthEnhancement pipeline reads its tables and builds its weight tables ahead of Process (nasp_tables).
#include "kde_handles.h"

extern "C" int kde_nasp_create(kde_nasp** out, int width, int height, int max_batch)
{
    KDE_REQUIRE(out, "kde_nasp_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_nasp_create", width, height, max_batch));
    kde_nasp* h = new_handle<kde_nasp>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_nasp_create: out of host memory");
    h->acos_thr = nasp_acos_threshold();
    const size_t px = (size_t)width * height * max_batch;
    int rc = h->labels.alloc(px);                 // SuperpixelSegmentation.cpp (ctor)
    if (rc == KDE_OK) rc = h->ld.alloc(px);
    if (rc == KDE_OK) rc = h->intr.alloc(9);      // DepthAdaptiveSuperpixel.cpp:6
    if (rc == KDE_OK) rc = h->ctab.alloc((size_t)kde_nasp::kColorCap);
    if (rc == KDE_OK) rc = h->ctab_host.ensure((size_t)kde_nasp::kColorCap);
    if (rc == KDE_OK && hipEventCreateWithFlags(&h->uploaded, hipEventDisableTiming) != hipSuccess)
        rc = fail(KDE_ERR_HIP, "kde_nasp_create: hipEventCreate failed");
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_nasp_destroy(kde_nasp* h) { delete h; return KDE_OK; }

extern "C" int kde_nasp_set_parameters(kde_nasp* h, int rows, int cols, const double* K)
{
    KDE_REQUIRE(h && K, "kde_nasp_set_parameters: null argument");
    KDE_ON_DEVICE(h, "kde_nasp_set_parameters");
    DaspGeom g;
    KDE_TRY(superpixel_geometry(h->width, h->height, rows, cols, 8, &g));
    const size_t k = (size_t)rows * cols * h->max_batch;
    const size_t px = (size_t)h->width * h->height * h->max_batch;
    KDE_TRY(h->mean.alloc(k));       // initMemory, NormalAdaptiveSuperpixel.cpp:19-37
    KDE_TRY(h->centers.alloc(k));
    KDE_TRY(h->normals.alloc(k));
    KDE_TRY(h->variance.alloc(k));
    // NA5: the reference leaves these as cudaMalloc returned them
    KDE_HIP_TRY(hipMemset(h->mean.p, 0, k * sizeof(kde_superpixel)));
    KDE_HIP_TRY(hipMemset(h->centers.p, 0, k * sizeof(kde_float3)));
    KDE_HIP_TRY(hipMemset(h->normals.p, 0, k * sizeof(kde_float3)));
    KDE_HIP_TRY(hipMemset(h->variance.p, 0, k * sizeof(float)));
    KDE_HIP_TRY(hipMemset(h->ld.p, 0, px * sizeof(kde_label_distance)));
    KDE_HIP_TRY(hipMemset(h->labels.p, 0, px * sizeof(int32_t)));
    // a thread of the two cluster kernels scans offsets (t - 8) * rp ... (t - 8) * rp + rp - 1, t = 0..15, per axis
    const long long rpx = g.wx * 2 / 16 + 1, rpy = g.wy * 2 / 16 + 1;
    h->spatial_need = 64 * (rpx * rpx + rpy * rpy) + 1;
    h->spatial_cap = std::min(h->spatial_need, kde_nasp::kSpatialCapMax);
    KDE_TRY(h->stab.alloc((size_t)h->spatial_cap));
    KDE_TRY(h->stab_host.ensure((size_t)h->spatial_cap));
    h->stab_valid = false;
    float intr[9];
    for (int i = 0; i < 9; i++) intr[i] = (float)K[i];   // DepthAdaptiveSuperpixel.cpp:33-37
    KDE_HIP_TRY(hipMemcpy(h->intr.p, intr, sizeof(intr), hipMemcpyHostToDevice));
    h->g = g;
    h->set = true;
    return KDE_OK;
}

// NA4: make the device tables those of (color_sigma, spatial_sigma).  A call with the sigmas of the previous one does
// nothing; otherwise the tables are rebuilt on the host and uploaded on the caller's stream from pinned memory the
// handle owns.  That upload cannot be part of a captured graph (a replay would re-read whatever the pinned mirror
// holds by then), so a capturing stream is refused: run one call with the same sigmas before capturing.
int kde::nasp_tables(kde_nasp* h, float color_sigma, float spatial_sigma, hipStream_t s)
{
    auto same = [](float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; };
    const bool need_c = !(h->ctab_valid && same(h->ctab_sigma, color_sigma));
    const bool need_s = !(h->stab_valid && same(h->stab_sigma, spatial_sigma));
    if (!need_c && !need_s) return KDE_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    KDE_HIP_TRY(hipStreamIsCapturing(s, &cap));
    if (cap != hipStreamCaptureStatusNone)
        return fail(KDE_ERR_UNSUPPORTED, "kde_nasp_segmentation: the first call with new color / spatial sigmas rebuilds the "
                                         "weight tables and cannot be captured; call once with these sigmas before capturing");
    KDE_HIP_TRY(hipEventSynchronize(h->uploaded));     // an earlier upload may still be reading the pinned mirrors
    if (need_s) {
        bool zero = false;
        const int n = nasp_weight_table(spatial_sigma, h->spatial_cap, h->stab_host.p, &zero);
        if (!zero && h->spatial_cap < h->spatial_need)
            return fail(KDE_ERR_UNSUPPORTED, "kde_nasp_segmentation: spatial_sigma %g is too large for a %dx%d window (its weight "
                                             "table would need %lld entries)", (double)spatial_sigma, h->g.wx, h->g.wy, h->spatial_need);
        h->stab_valid = false;
        if (n > 0) KDE_HIP_TRY(hipMemcpyAsync(h->stab.p, h->stab_host.p, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        h->stab_n = n;
        h->stab_sigma = spatial_sigma;
        h->stab_valid = true;
    }
    if (need_c) {
        bool zero = false;
        const int n = nasp_weight_table(color_sigma, kde_nasp::kColorCap, h->ctab_host.p, &zero);
        h->ctab_valid = false;
        if (n > 0) KDE_HIP_TRY(hipMemcpyAsync(h->ctab.p, h->ctab_host.p, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
        h->ctab_n = n;
        h->ctab_sigma = color_sigma;
        h->ctab_valid = true;
    }
    KDE_HIP_TRY(hipEventRecord(h->uploaded, s));
    return KDE_OK;
}

extern "C" int kde_nasp_segmentation_batch(kde_nasp* h, int n, const uint8_t* bgr_dev, const kde_float3* points_dev,
                                           const kde_float3* normals_dev, float color_sigma, float spatial_sigma,
                                           float depth_sigma, float normal_sigma, int iteration, void* stream)
{
    KDE_REQUIRE(h && bgr_dev && points_dev && normals_dev, "kde_nasp_segmentation: null argument");
    KDE_ON_DEVICE(h, "kde_nasp_segmentation");
    KDE_REQUIRE(h->set, "kde_nasp_segmentation: SetParametor was not called");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "kde_nasp_segmentation: bad n %d (max_batch %d)", n, h->max_batch);
    KDE_REQUIRE(iteration >= 0, "kde_nasp_segmentation: negative iteration count");
    // the weights are (sigma / sum of sigmas)^2 (.cu:256-258): a zero sum is 0/0 in the reference
    const float sum_sigma = spatial_sigma + color_sigma + normal_sigma + depth_sigma;
    KDE_REQUIRE(sum_sigma != 0.0f, "kde_nasp_segmentation: the sigmas must not sum to zero");
    hipStream_t s = as_stream(stream);
    KDE_TRY(nasp_tables(h, color_sigma, spatial_sigma, s));
    NaspLaunch a{};
    a.g = h->g;
    a.n = n;
    a.bgr = bgr_dev; a.pts = points_dev; a.nrm = normals_dev;
    a.ld = h->ld.p; a.labels = h->labels.p; a.mean = h->mean.p; a.centers = h->centers.p; a.spn = h->normals.p;
    a.variance = h->variance.p;
    a.intr = h->intr.p;
    a.ctab = h->ctab.p; a.ctab_n = h->ctab_n; a.stab = h->stab.p; a.stab_n = h->stab_n;
    const float rc = color_sigma / sum_sigma, rs = spatial_sigma / sum_sigma, rd = depth_sigma / sum_sigma,
                rn = normal_sigma / sum_sigma;
    a.kc = rc * rc; a.ks = rs * rs; a.kd = rd * rd; a.kn = rn * rn;
    const float half = (float)(h->g.wx + h->g.wy) / 2.0f;
    a.win2 = half * half;
    a.acos_thr = h->acos_thr;
    a.reset_on = (depth_sigma != 0.0f || normal_sigma != 0.0f) ? 1 : 0;
    // NormalAdaptiveSuperpixel.cu:1070-1096; initLD_NASP is folded into the first calculateLD_NASP, NA5 into the sampling
    KDE_TRY(launch_nasp_sample(a, s));
    if (iteration == 0) KDE_TRY(launch_nasp_init_ld(a, s));      // no first calculateLD_NASP to form the initial LD in
    for (int i = 0; i < iteration; i++) {
        KDE_TRY(launch_nasp_calc_ld(a, i == 0, s));
        KDE_TRY(launch_nasp_clusters(a, s));
    }
    h->n_last = n;
    return KDE_OK;
}

extern "C" int kde_nasp_segmentation(kde_nasp* h, const uint8_t* bgr_dev, const kde_float3* points_dev,
                                     const kde_float3* normals_dev, float color_sigma, float spatial_sigma, float depth_sigma,
                                     float normal_sigma, int iteration, void* stream)
{
    return kde_nasp_segmentation_batch(h, 1, bgr_dev, points_dev, normals_dev, color_sigma, spatial_sigma, depth_sigma,
                                       normal_sigma, iteration, stream);
}

KDE_DEVICE_GETTER(kde_nasp_labels_device, kde_nasp, int32_t, h->labels.p)                 // getLabelDevice (SuperpixelSegmentation.cpp)
KDE_DEVICE_GETTER(kde_nasp_mean_device, kde_nasp, kde_superpixel, h->mean.p)              // getMeanDataDevice
KDE_DEVICE_GETTER(kde_nasp_centers_device, kde_nasp, kde_float3, h->centers.p)            // getCentersDevice (NormalAdaptiveSuperpixel.h:23)
KDE_DEVICE_GETTER(kde_nasp_normals_device, kde_nasp, kde_float3, h->normals.p)            // getNormalsDevice (:25)
KDE_DEVICE_GETTER(kde_nasp_normals_variance_device, kde_nasp, float, h->variance.p)       // getNormalsVarianceDevice (:27)
KDE_DEVICE_GETTER(kde_nasp_ld_device, kde_nasp, kde_label_distance, h->ld.p)              // LD_Device

// the *_Host getters mirror the n_last frames the last Segmentation produced
extern "C" int kde_nasp_labels_host(kde_nasp* h, void* stream, const int32_t** out)
{
    KDE_REQUIRE(h && out, "kde_nasp_labels_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    return host_mirror("kde_nasp_labels_host", h->device, h->labels.p, px * h->n_last, px * h->max_batch, h->labels_host,
                       as_stream(stream), out);
}

// one per-cluster table: *count = the entries of the n_last frames
template <typename T>
static int nasp_table_host(kde_nasp* h, const char* who, void* stream, const DevBuf<T>& dev, PinnedBuf<T>& host, const T** out, int* count)
{
    KDE_REQUIRE(h && out && count, "%s: null argument", who);
    KDE_REQUIRE(h->set, "%s: SetParametor has not been called", who);
    const size_t nc = (size_t)h->g.rows * h->g.cols;
    KDE_TRY(host_mirror(who, h->device, dev.p, nc * h->n_last, nc * h->max_batch, host, as_stream(stream), out));
    *count = (int)(nc * h->n_last);
    return KDE_OK;
}

extern "C" int kde_nasp_mean_host(kde_nasp* h, void* stream, const kde_superpixel** out, int* count)
{
    KDE_REQUIRE(h, "kde_nasp_mean_host: null argument");
    return nasp_table_host(h, "kde_nasp_mean_host", stream, h->mean, h->mean_host, out, count);
}
extern "C" int kde_nasp_centers_host(kde_nasp* h, void* stream, const kde_float3** out, int* count)
{
    KDE_REQUIRE(h, "kde_nasp_centers_host: null argument");
    return nasp_table_host(h, "kde_nasp_centers_host", stream, h->centers, h->centers_host, out, count);
}
extern "C" int kde_nasp_normals_host(kde_nasp* h, void* stream, const kde_float3** out, int* count)
{
    KDE_REQUIRE(h, "kde_nasp_normals_host: null argument");
    return nasp_table_host(h, "kde_nasp_normals_host", stream, h->normals, h->normals_host, out, count);
}
extern "C" int kde_nasp_normals_variance_host(kde_nasp* h, void* stream, const float** out, int* count)
{
    KDE_REQUIRE(h, "kde_nasp_normals_variance_host: null argument");
    return nasp_table_host(h, "kde_nasp_normals_variance_host", stream, h->variance, h->variance_host, out, count);
}
