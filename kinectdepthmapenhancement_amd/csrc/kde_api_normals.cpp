// kde_api_normals.cpp — NormalMapGenerator (kde_normals_*, normal_kernels.hip).  struct kde_normals is in kde_handles.h:
// the KinectDepthEnhancement pipeline reads its normal map.
#include "kde_handles.h"

static int normals_check_method(int method, const char* who)
{
    if (method == KDE_NORMALS_SDC)
        return fail(KDE_ERR_UNSUPPORTED, "%s: SDC is not built (its flip test reads the previous call's output, "
                                         "NormalMapGenerator.cu:108)", who);
    KDE_REQUIRE(method == KDE_NORMALS_CM || method == KDE_NORMALS_BILATERAL, "%s: unknown method %d", who, method);
    return KDE_OK;
}

extern "C" int kde_normals_default_params(kde_normals_params* p)
{
    KDE_REQUIRE(p, "kde_normals_default_params: null argument");
    p->method = KDE_NORMALS_BILATERAL;     // NormalMapGenerator.cpp:15
    p->max_depth_change_factor = 0.05f;    // SmoothingAreaMapGenerator.cpp:15
    p->normal_smoothing_size = 20.0f;      // :16
    return KDE_OK;
}

extern "C" int kde_normals_create(kde_normals** out, int width, int height, int max_batch, const kde_normals_params* params)
{
    KDE_REQUIRE(out, "kde_normals_create: null out");
    *out = nullptr;
    KDE_REQUIRE(frame_ok(width, height) && batch_ok(max_batch), "kde_normals_create: bad size %dx%d x %d", width, height, max_batch);
    kde_normals_params p;
    if (params) p = *params;
    else kde_normals_default_params(&p);
    KDE_TRY(normals_check_method(p.method, "kde_normals_create"));
    KDE_REQUIRE(std::isfinite(p.max_depth_change_factor), "kde_normals_create: max_depth_change_factor must be finite");
    KDE_REQUIRE(std::isfinite(p.normal_smoothing_size) && std::fabs(p.normal_smoothing_size) <= 1e6f,
                "kde_normals_create: normal_smoothing_size must be finite, within +-1e6");
    kde_normals* h = new_handle<kde_normals>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_normals_create: out of host memory");
    h->p = p;
    h->chunk_frames = normals_chunk_frames(width, height, max_batch);
    const size_t px = (size_t)width * height;
    int rc = h->normals.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->fs.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->dci.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->cmax.alloc((size_t)max_batch);
    if (rc == KDE_OK) rc = h->dt_scratch.alloc((size_t)normals_dt_bands(height) * max_batch * 2 * width);
    if (rc == KDE_OK) rc = h->cnt.alloc(px * h->chunk_frames);
    if (rc == KDE_OK) rc = h->sums.alloc(px * h->chunk_frames * 9);
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_normals_destroy(kde_normals* h) { delete h; return KDE_OK; }

extern "C" int kde_normals_set_method(kde_normals* h, int method)
{
    KDE_REQUIRE(h, "kde_normals_set_method: null argument");
    KDE_TRY(normals_check_method(method, "kde_normals_set_method"));
    h->p.method = method;
    return KDE_OK;
}

extern "C" int kde_normals_generate_batch(kde_normals* h, int n, const kde_float3* points_dev, kde_float3* normals_dev, void* stream)
{
    KDE_REQUIRE(h && points_dev, "kde_normals_generate_batch: null argument");
    KDE_ON_DEVICE(h, "kde_normals_generate_batch");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "kde_normals_generate_batch: bad n %d (max_batch %d)", n, h->max_batch);
    NormalsLaunch a{h->width, h->height, n, h->p.method, h->p.max_depth_change_factor, h->p.normal_smoothing_size,
                    points_dev, normals_dev ? normals_dev : h->normals.p, h->fs.p, h->dci.p, h->cmax.p, h->dt_scratch.p,
                    h->cnt.p, h->sums.p, h->chunk_frames};
    KDE_TRY(launch_normals(a, as_stream(stream)));
    if (!normals_dev) h->n_last = n;
    h->fs_valid = h->p.method == KDE_NORMALS_CM;
    return KDE_OK;
}

KDE_DEVICE_GETTER(kde_normals_normal_map_device, kde_normals, kde_float3, h->normals.p)

extern "C" int kde_normals_normal_map_host(kde_normals* h, void* stream, const kde_float3** out)
{
    KDE_REQUIRE(h && out, "kde_normals_normal_map_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    const int frames = h->n_last > 0 ? h->n_last : 1;
    return host_mirror("kde_normals_normal_map_host", h->device, h->normals.p, px * frames, px * h->max_batch, h->normals_host,
                       as_stream(stream), out);
}

extern "C" int kde_normals_smoothing_map_device(kde_normals* h, float** out)
{
    KDE_REQUIRE(h && out, "kde_normals_smoothing_map_device: null argument");
    KDE_REQUIRE(h->fs_valid, "kde_normals_smoothing_map_device: the last call did not run CM");
    *out = h->fs.p;
    return KDE_OK;
}
