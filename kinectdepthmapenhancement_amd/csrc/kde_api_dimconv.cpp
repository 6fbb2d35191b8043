// kde_api_dimconv.cpp — DimensionConvertor (kde_dimconv_*) and Buffer2D (kde_buffer2d_*).  struct kde_dimconv is in
// kde_handles.h: kde_spdsr and kde_enh hold one by value.
#include "kde_handles.h"

// =====================================================================================================
// DimensionConvertor
// =====================================================================================================
extern "C" int kde_dimconv_create(kde_dimconv** out)
{
    KDE_REQUIRE(out, "kde_dimconv_create: null out");
    *out = new (std::nothrow) kde_dimconv;
    return *out ? KDE_OK : fail(KDE_ERR_NOMEM, "kde_dimconv_create: out of host memory");
}

extern "C" int kde_dimconv_destroy(kde_dimconv* h) { delete h; return KDE_OK; }

extern "C" int kde_dimconv_set_camera(kde_dimconv* h, const double* K, int width, int height)
{
    KDE_REQUIRE(h && K, "kde_dimconv_set_camera: null argument");
    KDE_REQUIRE(frame_ok(width, height), "kde_dimconv_set_camera: bad size");
    // DimensionConvertor.cpp:3-13
    h->cam.fx = (float)K[0];
    h->cam.fy = (float)K[4];
    h->cam.cx = (int)K[2];
    h->cam.cy = (int)K[5];
    h->cam.width = width;
    h->cam.height = height;
    h->set = true;
    return KDE_OK;
}

static int dimconv_check(kde_dimconv* h, int n, const void* in, const void* out, const char* who)
{
    KDE_REQUIRE(h && in && out, "%s: null argument", who);
    KDE_REQUIRE(h->set, "%s: setCameraParameters was not called", who);
    KDE_REQUIRE(n >= 1 && n <= 65535, "%s: bad frame count %d", who, n);
    // any float* / float3* is accepted, as by the reference: pointers that are not 16-byte aligned (or batched frames
    // whose size is not a multiple of 4) take the scalar kernels of stream_kernels.hip
    return KDE_OK;
}

extern "C" int kde_dimconv_projective_to_real_depth(kde_dimconv* h, int n, const float* depth_dev, kde_float3* out_dev, void* stream)
{
    KDE_TRY(dimconv_check(h, n, depth_dev, out_dev, "kde_dimconv_projective_to_real_depth"));
    return launch_p2r_depth(h->cam, n, depth_dev, out_dev, as_stream(stream));
}

extern "C" int kde_dimconv_projective_to_real_points(kde_dimconv* h, int n, const kde_float3* in_dev, kde_float3* out_dev, void* stream)
{
    KDE_TRY(dimconv_check(h, n, in_dev, out_dev, "kde_dimconv_projective_to_real_points"));
    return launch_p2r_points(h->cam, n, in_dev, out_dev, as_stream(stream));
}

extern "C" int kde_dimconv_projective_to_real_interp(kde_dimconv* h, int n, const float* depth_dev, kde_float3* out_dev, void* stream)
{
    KDE_TRY(dimconv_check(h, n, depth_dev, out_dev, "kde_dimconv_projective_to_real_interp"));
    return launch_p2r_interp(h->cam, n, depth_dev, out_dev, as_stream(stream));
}

extern "C" int kde_dimconv_real_to_projective(kde_dimconv* h, int n, const kde_float3* in_dev, kde_float3* out_dev, void* stream)
{
    KDE_TRY(dimconv_check(h, n, in_dev, out_dev, "kde_dimconv_real_to_projective"));
    return launch_r2p(h->cam, n, in_dev, out_dev, as_stream(stream));
}

// =====================================================================================================
// Buffer2D
// =====================================================================================================
struct kde_buffer2d {
    int device = -1;
    int width, height;
    DevBuf<kde_weighted_d> buf;   // devPtr
};

extern "C" int kde_buffer2d_create(kde_buffer2d** out, int width, int height)
{
    KDE_REQUIRE(out, "kde_buffer2d_create: null out");
    *out = nullptr;
    KDE_REQUIRE(frame_ok(width, height), "kde_buffer2d_create: bad size");
    kde_buffer2d* h = new (std::nothrow) kde_buffer2d;
    if (!h) return fail(KDE_ERR_NOMEM, "kde_buffer2d_create: out of host memory");
    h->device = current_device();
    h->width = width;
    h->height = height;
    int rc = h->buf.alloc((size_t)width * height);
    if (rc == KDE_OK) rc = launch_buf_init(h->buf.p, h->buf.n, nullptr);   // initDeviceMemoryElements
    if (rc == KDE_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(KDE_ERR_HIP, "kde_buffer2d_create: init failed");
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_buffer2d_destroy(kde_buffer2d* h) { delete h; return KDE_OK; }

extern "C" int kde_buffer2d_insert_depth(kde_buffer2d* h, const float* depth_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev, "kde_buffer2d_insert_depth: null argument");
    KDE_ON_DEVICE(h, "kde_buffer2d_insert_depth");
    return launch_buf_insert_depth(h->buf.p, depth_dev, h->buf.n, as_stream(stream));
}

extern "C" int kde_buffer2d_insert_float2(kde_buffer2d* h, const float* xy_dev, void* stream)
{
    KDE_REQUIRE(h && xy_dev, "kde_buffer2d_insert_float2: null argument");
    KDE_ON_DEVICE(h, "kde_buffer2d_insert_float2");
    return launch_buf_insert_float2(h->buf.p, xy_dev, h->width, h->height, as_stream(stream));
}

extern "C" int kde_buffer2d_insert_weighted(kde_buffer2d* h, const kde_weighted_d* data_dev, void* stream)
{
    KDE_REQUIRE(h && data_dev, "kde_buffer2d_insert_weighted: null argument");
    KDE_ON_DEVICE(h, "kde_buffer2d_insert_weighted");
    KDE_HIP_TRY(hipMemcpyAsync(h->buf.p, data_dev, h->buf.n * sizeof(kde_weighted_d), hipMemcpyDeviceToDevice, as_stream(stream)));
    return KDE_OK;
}

extern "C" int kde_buffer2d_get_depth_map(kde_buffer2d* h, float* out_dev, void* stream)
{
    KDE_REQUIRE(h && out_dev, "kde_buffer2d_get_depth_map: null argument");
    KDE_ON_DEVICE(h, "kde_buffer2d_get_depth_map");
    return launch_buf_get(h->buf.p, out_dev, h->buf.n, 0, as_stream(stream));
}

extern "C" int kde_buffer2d_get_weight_map(kde_buffer2d* h, float* out_dev, void* stream)
{
    KDE_REQUIRE(h && out_dev, "kde_buffer2d_get_weight_map: null argument");
    KDE_ON_DEVICE(h, "kde_buffer2d_get_weight_map");
    return launch_buf_get(h->buf.p, out_dev, h->buf.n, 1, as_stream(stream));
}

extern "C" int kde_buffer2d_update_sequence(kde_buffer2d* h, int n_frames, const float* depth_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev, "kde_buffer2d_update: null argument");
    KDE_ON_DEVICE(h, "kde_buffer2d_update");
    KDE_REQUIRE(n_frames >= 1, "kde_buffer2d_update: n_frames must be >= 1");
    return launch_buf_update(h->buf.p, depth_dev, h->buf.n, n_frames, as_stream(stream));
}

extern "C" int kde_buffer2d_update(kde_buffer2d* h, const float* depth_dev, void* stream)
{
    return kde_buffer2d_update_sequence(h, 1, depth_dev, stream);
}

KDE_DEVICE_GETTER(kde_buffer2d_raw_pointer, kde_buffer2d, kde_weighted_d, h->buf.p)
