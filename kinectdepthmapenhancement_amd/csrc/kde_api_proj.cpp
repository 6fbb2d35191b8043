// kde_api_proj.cpp — Projection_GPU's five-argument PlaneProjection (kde_proj_*, proj_kernels.hip) and
// KinectDepthEnhancement (kde_enh_*), which owns one object of each stage and reads their buffers (kde_handles.h, where
// struct kde_enh is too: the host-fed form in kde_api_enh_feed.cpp runs it).
#include "kde_handles.h"

// =====================================================================================================
// Projection_GPU, five-argument PlaneProjection
// =====================================================================================================
extern "C" int kde_proj_default_params(kde_proj_params* p)
{
    KDE_REQUIRE(p, "kde_proj_default_params: null argument");
    p->window_size = 7;                          // Projection_GPU.cpp:4
    p->spatial_sigma = 20.0f;                    // :3
    p->depth_sigma = 100.0f;                     // :5
    p->max_angle = 3.141592653f / 8.0f;          // Projection_GPU.cu:38, :203
    p->min_size = 1300;                          // :203
    return KDE_OK;
}

extern "C" int kde_proj_create(kde_proj** out, int width, int height, int max_batch, const double* K, const kde_proj_params* params)
{
    KDE_REQUIRE(out, "kde_proj_create: null out");
    *out = nullptr;
    KDE_REQUIRE(K, "kde_proj_create: null intrinsic matrix");
    KDE_TRY(check_frame_batch("kde_proj_create", width, height, max_batch));
    kde_proj_params p;
    kde_proj_default_params(&p);
    if (params) p = *params;
    KDE_REQUIRE(p.window_size >= 1 && p.window_size <= kProjMaxWindow && (p.window_size & 1),
                "kde_proj_create: window_size must be odd in 1..%d", kProjMaxWindow);
    KDE_REQUIRE(p.spatial_sigma == p.spatial_sigma && p.spatial_sigma != 0.0f, "kde_proj_create: spatial_sigma must not be 0 or NaN");
    KDE_REQUIRE(p.depth_sigma > 0.0f, "kde_proj_create: depth_sigma must be > 0");
    KDE_REQUIRE(p.max_angle == p.max_angle, "kde_proj_create: max_angle must not be NaN");
    kde_proj* h = new_handle<kde_proj>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_proj_create: out of host memory");
    h->p = p;
    h->thr = acos_threshold(p.max_angle);
    const size_t px = (size_t)width * height;
    const int w2 = p.window_size * p.window_size;
    int rc = h->nxy.alloc(px * 2);               // initMemory, Projection_GPU.cpp:45-51
    if (rc == KDE_OK) rc = h->spatial.alloc((size_t)w2);
    if (rc == KDE_OK) rc = h->plane_fitted.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->z.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->optimized.alloc(px * max_batch);
    if (rc == KDE_OK) {
        float table[kProjMaxWindow * kProjMaxWindow];            // calcSpatialFilter, .cpp:35-44
        for (int i = 0; i < p.window_size; i++)
            for (int j = 0; j < p.window_size; j++) {
                const float dis_x = powf((float)(j - p.window_size / 2), 2.0f);
                const float dis_y = powf((float)(i - p.window_size / 2), 2.0f);
                table[i * p.window_size + j] = expf(-(dis_x + dis_y) / (2.0f * powf(p.spatial_sigma, 2.0f)));
            }
        if (hipMemcpy(h->spatial.p, table, (size_t)w2 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(KDE_ERR_HIP, "kde_proj_create: hipMemcpy failed");
    }
    if (rc == KDE_OK) {                          // initNormalized3D, .cu:124-128 (the constructor's intrinsics, .cpp:11-15)
        const Camera cam{(float)K[0], (float)K[4], (int)K[2], (int)K[5], width, height};
        rc = launch_spdsr_init_normalized(cam, h->nxy.p, nullptr);
        if (rc == KDE_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(KDE_ERR_HIP, "kde_proj_create: hipStreamSynchronize failed");
    }
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_proj_destroy(kde_proj* h) { delete h; return KDE_OK; }

extern "C" int kde_proj_plane_projection_batch(kde_proj* h, int n, const kde_float4* nd_dev, const int32_t* labels_dev,
                                               const float* variance_dev, const kde_float3* points_dev, const int32_t* size_dev,
                                               int n_clusters, void* stream)
{
    KDE_REQUIRE(h && nd_dev && labels_dev && variance_dev && points_dev && size_dev, "kde_proj_plane_projection: null argument");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "kde_proj_plane_projection: bad n %d (max_batch %d)", n, h->max_batch);
    KDE_REQUIRE(n_clusters >= 1, "kde_proj_plane_projection: n_clusters %d must be >= 1", n_clusters);
    KDE_ON_DEVICE(h, "kde_proj_plane_projection");
    ProjLaunch a{};
    a.width = h->width; a.height = h->height; a.n = n;
    a.nc = n_clusters;
    a.nd = reinterpret_cast<const float4*>(nd_dev); a.labels = labels_dev; a.variance = variance_dev;
    a.pts = points_dev; a.size = size_dev;
    a.nxy = reinterpret_cast<const float2*>(h->nxy.p);
    a.spatial = h->spatial.p;
    a.plane_fitted = h->plane_fitted.p; a.z = h->z.p; a.optimized = h->optimized.p;
    a.window = h->p.window_size; a.min_size = h->p.min_size;
    a.thr = h->thr;
    a.depth_den = 2.0f * (h->p.depth_sigma * h->p.depth_sigma);
    KDE_TRY(launch_proj_plane_projection(a, as_stream(stream)));
    h->n_last = n;
    return KDE_OK;
}

extern "C" int kde_proj_plane_projection(kde_proj* h, const kde_float4* nd_dev, const int32_t* labels_dev, const float* variance_dev,
                                         const kde_float3* points_dev, const int32_t* size_dev, int n_clusters, void* stream)
{
    return kde_proj_plane_projection_batch(h, 1, nd_dev, labels_dev, variance_dev, points_dev, size_dev, n_clusters, stream);
}

KDE_DEVICE_GETTER(kde_proj_optimized_points_device, kde_proj, kde_float3, h->optimized.p)
KDE_DEVICE_GETTER(kde_proj_plane_fitted_points_device, kde_proj, kde_float3, h->plane_fitted.p)

// the *_Host getters mirror the n_last frames the last PlaneProjection produced
extern "C" int kde_proj_optimized_points_host(kde_proj* h, void* stream, const kde_float3** out)
{
    KDE_REQUIRE(h && out, "kde_proj_optimized_points_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    return host_mirror("kde_proj_optimized_points_host", h->device, h->optimized.p, px * h->n_last, px * h->max_batch,
                       h->optimized_host, as_stream(stream), out);
}

extern "C" int kde_proj_plane_fitted_points_host(kde_proj* h, void* stream, const kde_float3** out)
{
    KDE_REQUIRE(h && out, "kde_proj_plane_fitted_points_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    return host_mirror("kde_proj_plane_fitted_points_host", h->device, h->plane_fitted.p, px * h->n_last, px * h->max_batch,
                       h->plane_fitted_host, as_stream(stream), out);
}

// =====================================================================================================
// KinectDepthEnhancement: the six stage objects in the order of KinectDepthEnhancement.cpp:56-81
// =====================================================================================================
extern "C" int kde_enh_create(kde_enh** out, int width, int height, int max_batch)
{
    KDE_REQUIRE(out, "kde_enh_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_enh_create", width, height, max_batch));
    kde_enh* h = new (std::nothrow) kde_enh;
    if (!h) return fail(KDE_ERR_NOMEM, "kde_enh_create: out of host memory");
    h->width = width;
    h->height = height;
    h->max_batch = max_batch;
    kde_normals_params np;
    kde_normals_default_params(&np);
    np.method = KDE_NORMALS_CM;                                                  // .cpp:53
    int rc = kde_jbf_create(&h->JBF, width, height, max_batch, nullptr);        // .cpp:17
    if (rc == KDE_OK) rc = kde_normals_create(&h->NormalGenerator, width, height, max_batch, &np);   // :20
    if (rc == KDE_OK) rc = kde_nasp_create(&h->NASP, width, height, max_batch);                      // :16
    if (rc == KDE_OK) rc = kde_les_create(&h->spMerging, width, height, max_batch, nullptr);         // :21
    if (rc == KDE_OK) rc = h->edge_points.alloc((size_t)width * height * max_batch);                 // :22
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_enh_destroy(kde_enh* h) { delete h; return KDE_OK; }

extern "C" int kde_enh_set_parameters(kde_enh* h, int rows, int cols, const double* K)
{
    KDE_REQUIRE(h && K, "kde_enh_set_parameters: null argument");
    KDE_ON_DEVICE(h->NASP, "kde_enh_set_parameters");
    KDE_REQUIRE(rows >= 1 && cols >= 1 && (long long)rows * cols <= h->spMerging->cap,
                "kde_enh_set_parameters: rows*cols must be in 1..%d (the kde_les_label_image bound)", h->spMerging->cap);
    h->nclusters = 0;
    KDE_TRY(kde_nasp_set_parameters(h->NASP, rows, cols, K));                    // .cpp:51
    KDE_TRY(kde_dimconv_set_camera(&h->conv, K, h->width, h->height));           // :52
    KDE_TRY(kde_normals_set_method(h->NormalGenerator, KDE_NORMALS_CM));         // :53
    kde_proj_destroy(h->Projector);
    h->Projector = nullptr;
    KDE_TRY(kde_proj_create(&h->Projector, h->width, h->height, h->max_batch, K, nullptr));   // :54
    // the weight tables of Process's Segmentation call (:67), built here so that Process never uploads
    KDE_TRY(nasp_tables(h->NASP, 10.0f, 50.0f, nullptr));
    KDE_HIP_TRY(hipStreamSynchronize(nullptr));
    h->nclusters = rows * cols;
    return KDE_OK;
}

extern "C" int kde_enh_process_batch(kde_enh* h, int n, const float* depth_dev, const uint8_t* bgr_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev && bgr_dev, "kde_enh_process: null argument");
    KDE_REQUIRE(h->nclusters > 0, "kde_enh_process: SetParametor was not called");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "kde_enh_process: bad n %d (max_batch %d)", n, h->max_batch);
    KDE_TRY(kde_jbf_process_batch(h->JBF, n, depth_dev, bgr_dev, nullptr, stream));                                  // .cpp:58
    KDE_TRY(kde_dimconv_projective_to_real_depth(&h->conv, n, h->JBF->filtered.p, h->edge_points.p, stream));        // :60
    KDE_TRY(kde_normals_generate_batch(h->NormalGenerator, n, h->edge_points.p, nullptr, stream));                   // :65
    KDE_TRY(kde_nasp_segmentation_batch(h->NASP, n, bgr_dev, h->edge_points.p, h->NormalGenerator->normals.p, 10.0f, 50.0f, 50.0f,
                                        150.0f, 1, stream));                                                         // :67
    KDE_TRY(kde_les_label_image_batch(h->spMerging, n, h->NASP->normals.p, h->NASP->labels.p, h->NASP->centers.p,
                                      h->NASP->variance.p, h->nclusters, stream));                                   // :76
    return kde_proj_plane_projection_batch(h->Projector, n, reinterpret_cast<const kde_float4*>(h->spMerging->merged_nd.p),
                                           h->spMerging->merged_label.p, h->spMerging->variance.p, h->edge_points.p,
                                           h->spMerging->size.p, h->nclusters, stream);                              // :79-80
}

extern "C" int kde_enh_optimized_points_device(kde_enh* h, kde_float3** out)
{
    KDE_REQUIRE(h && out, "kde_enh_optimized_points_device: null argument");
    KDE_REQUIRE(h->Projector, "getOptimizedPoints: SetParametor was not called");
    return kde_proj_optimized_points_device(h->Projector, out);
}

extern "C" int kde_enh_optimized_points_host(kde_enh* h, void* stream, const kde_float3** out)
{
    KDE_REQUIRE(h && out, "kde_enh_optimized_points_host: null argument");
    KDE_REQUIRE(h->Projector, "getOptimizedPoints: SetParametor was not called");
    return kde_proj_optimized_points_host(h->Projector, stream, out);
}

extern "C" int kde_enh_nasp_labels_device(kde_enh* h, int32_t** out)
{
    KDE_REQUIRE(h && out, "kde_enh_nasp_labels_device: null argument");
    return kde_nasp_labels_device(h->NASP, out);
}

extern "C" int kde_enh_merged_labels_device(kde_enh* h, int32_t** out)
{
    KDE_REQUIRE(h && out, "kde_enh_merged_labels_device: null argument");
    return kde_les_merged_label_device(h->spMerging, out);
}

KDE_DEVICE_GETTER(kde_enh_edge_enhanced_points_device, kde_enh, kde_float3, h->edge_points.p)
