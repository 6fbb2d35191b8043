// kde_api_les.cpp — LabelEquivalenceSeg (kde_les_*, les_kernels.hip).  struct kde_les is in kde_handles.h: the
// KinectDepthEnhancement pipeline reads its merged tables.
#include "kde_handles.h"

extern "C" int kde_les_default_params(kde_les_params* p)
{
    KDE_REQUIRE(p, "kde_les_default_params: null argument");
    p->iterations = 10;                          // LabelEquivalenceSeg.cu:235
    p->max_angle = 3.141592653f / 8.0f;          // :40
    p->max_plane_distance = 150.0f;              // :42
    return KDE_OK;
}

extern "C" int kde_les_create(kde_les** out, int width, int height, int max_batch, const kde_les_params* params)
{
    KDE_REQUIRE(out, "kde_les_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_les_create", width, height, max_batch));
    kde_les_params p;
    kde_les_default_params(&p);
    if (params) p = *params;
    KDE_REQUIRE(p.iterations >= 0, "kde_les_create: negative iteration count");
    KDE_REQUIRE(p.max_angle == p.max_angle && p.max_plane_distance == p.max_plane_distance, "kde_les_create: NaN parameter");
    kde_les* h = new_handle<kde_les>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_les_create: out of host memory");
    h->p = p;
    h->thr = les_acos_threshold(p.max_angle);
    h->cap = (int)std::min<long long>((long long)width * height, kLesMaxClusters);
    const size_t px = (size_t)width * height * max_batch, k = (size_t)h->cap * max_batch;
    const size_t wpr = (size_t)ceil_div(h->cap, 32);
    int rc = h->merged_label.alloc(px);
    if (rc == KDE_OK) rc = h->merged_nd.alloc(px);
    if (rc == KDE_OK) rc = h->variance.alloc(k);
    if (rc == KDE_OK) rc = h->size.alloc(k);
    if (rc == KDE_OK) rc = h->mnd.alloc(k);
    if (rc == KDE_OK) rc = h->scratch.alloc(k * (1 + wpr));
    if (rc == KDE_OK) rc = h->tables.alloc(k * (1 + wpr));
    // counts and adjacency must be zero on entry to every call; the kernels leave them so
    if (rc == KDE_OK && hipMemset(h->scratch.p, 0, k * (1 + wpr) * sizeof(int32_t)) != hipSuccess)
        rc = fail(KDE_ERR_HIP, "kde_les_create: hipMemset failed");
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_les_destroy(kde_les* h) { delete h; return KDE_OK; }

extern "C" int kde_les_label_image_batch(kde_les* h, int n, const kde_float3* normals_dev, const int32_t* labels_dev,
                                         const kde_float3* centers_dev, const float* variance_dev, int n_clusters, void* stream)
{
    KDE_REQUIRE(h && normals_dev && labels_dev && centers_dev, "kde_les_label_image: null argument");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "kde_les_label_image: bad n %d (max_batch %d)", n, h->max_batch);
    KDE_REQUIRE(n_clusters >= 1 && n_clusters <= h->cap, "kde_les_label_image: n_clusters %d is outside 1..%d (min(W*H, %d))",
                n_clusters, h->cap, kLesMaxClusters);
    KDE_ON_DEVICE(h, "kde_les_label_image");
    (void)variance_dev;                          // dead in the reference (.cu:82)
    LesLaunch a{};
    a.width = h->width; a.height = h->height; a.n = n;
    a.nc = n_clusters; a.wpr = ceil_div(n_clusters, 32);
    a.normals = normals_dev; a.labels = labels_dev; a.centers = centers_dev;
    const size_t k = (size_t)n * n_clusters, words = k * a.wpr;
    a.count = h->scratch.p;
    a.adj = reinterpret_cast<uint32_t*>(a.count + k);
    a.list = h->tables.p;
    a.mfin = a.list + words;
    a.mnd = h->mnd.p;
    a.merged_label = h->merged_label.p; a.merged_nd = h->merged_nd.p;
    a.variance = h->variance.p; a.size = h->size.p;
    a.iterations = h->p.iterations;
    a.thr = h->thr; a.max_dist = h->p.max_plane_distance;
    if (h->dirty) {                              // an earlier call failed between its launches: start from zero again
        KDE_HIP_TRY(hipMemsetAsync(h->scratch.p, 0, h->scratch.n * sizeof(int32_t), as_stream(stream)));
        h->dirty = false;
    }
    const int rc = launch_les_label_image(a, as_stream(stream));
    if (rc != KDE_OK) {
        h->dirty = true;
        return rc;
    }
    h->n_last = n;
    h->nc_last = n_clusters;
    return KDE_OK;
}

extern "C" int kde_les_label_image(kde_les* h, const kde_float3* normals_dev, const int32_t* labels_dev,
                                   const kde_float3* centers_dev, const float* variance_dev, int n_clusters, void* stream)
{
    return kde_les_label_image_batch(h, 1, normals_dev, labels_dev, centers_dev, variance_dev, n_clusters, stream);
}

KDE_DEVICE_GETTER(kde_les_merged_label_device, kde_les, int32_t, h->merged_label.p)                           // getMergedClusterLabel_Device
KDE_DEVICE_GETTER(kde_les_merged_nd_device, kde_les, kde_float4, reinterpret_cast<kde_float4*>(h->merged_nd.p))  // getMergedClusterND_Device
KDE_DEVICE_GETTER(kde_les_merged_variance_device, kde_les, float, h->variance.p)                                 // getMergedClusterVariance_Device
KDE_DEVICE_GETTER(kde_les_merged_size_device, kde_les, int32_t, h->size.p)                                       // getMergedClusterSize_Device

// the *_Host getters mirror the n_last frames the last labelImage produced
extern "C" int kde_les_merged_label_host(kde_les* h, void* stream, const int32_t** out)
{
    KDE_REQUIRE(h && out, "kde_les_merged_label_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    return host_mirror("kde_les_merged_label_host", h->device, h->merged_label.p, px * h->n_last, px * h->max_batch,
                       h->merged_label_host, as_stream(stream), out);
}

extern "C" int kde_les_merged_nd_host(kde_les* h, void* stream, const kde_float4** out)
{
    KDE_REQUIRE(h && out, "kde_les_merged_nd_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    const float4* nd = nullptr;
    KDE_TRY(host_mirror("kde_les_merged_nd_host", h->device, h->merged_nd.p, px * h->n_last, px * h->max_batch, h->merged_nd_host,
                        as_stream(stream), &nd));
    *out = reinterpret_cast<const kde_float4*>(nd);
    return KDE_OK;
}
