// kde_api_reg.cpp — DepthRegistration (kde_reg_*): the registration Kinect::InitAllData (Kinect.cpp:71-75) asks OpenNI for,
// for a batch of frames on the device (reg_kernels.hip): depth warped into the colour camera's view through a z-buffer.
#include "kde_handles.h"

struct kde_reg {
    int device = -1;                        // -1: created on a host without a device (no buffers; the launches refuse)
    int width = 0, height = 0, max_batch = 1;   // the depth camera's frame
    int color_w = 0, color_h = 0;
    kde_reg_params p{};
    RegCalib c{};
    bool calibrated = false;
    DepthStage stage;                       // the last register_batch; depth [max_batch][color_h][color_w]
    DevBuf<uint32_t> zbuf;                  // [max_batch][reg_zstride(color_w * color_h)]
    DevBuf<uint32_t> filled;                // [max_batch]
    PinnedBuf<uint32_t> filled_host;
};

static const kde_reg_params kRegDefaults = {0.0f, FLT_MAX, 0};

// Kinect.cpp:71-75 takes no parameter: every finite positive depth is registered, one target pixel per source pixel
extern "C" int kde_reg_default_params(kde_reg_params* p)
{
    KDE_REQUIRE(p, "kde_reg_default_params: null argument");
    *p = kRegDefaults;
    return KDE_OK;
}

// Kinect.cpp:71-75: the two generators whose views are aligned
extern "C" int kde_reg_create(kde_reg** out, int depth_w, int depth_h, int color_w, int color_h, int max_batch, const kde_reg_params* p)
{
    const char* who = "kde_reg_create";
    KDE_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    KDE_TRY(check_frame_batch(who, depth_w, depth_h, max_batch));
    KDE_REQUIRE(frame_ok(color_w, color_h), "%s: bad size", who);
    KDE_REQUIRE(depth_w <= kRegMaxSide && depth_h <= kRegMaxSide && color_w <= kRegMaxSide && color_h <= kRegMaxSide,
                "%s: a side above %d is not an exact float", who, kRegMaxSide);
    const kde_reg_params q = p ? *p : kRegDefaults;
    KDE_TRY(check_z_range(who, q.z_min, q.z_max, " (the key order needs positive z)"));
    KDE_REQUIRE(q.max_splat >= 0 && q.max_splat <= kRegMaxSplat, "%s: max_splat=%d outside 0..%d", who, q.max_splat, kRegMaxSplat);
    kde_reg* h = new_handle<kde_reg>(depth_w, depth_h, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    h->color_w = color_w;
    h->color_h = color_h;
    h->p = q;
    if (h->device >= 0) {
        const size_t px = (size_t)color_w * color_h;
        int rc = h->zbuf.alloc((size_t)max_batch * reg_zstride(px));
        if (rc == KDE_OK) rc = h->filled.alloc((size_t)max_batch);
        if (rc == KDE_OK) rc = h->stage.depth.alloc((size_t)max_batch * px);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

// Kinect.cpp:71-75 keeps its generators for the life of the Kinect object
extern "C" int kde_reg_destroy(kde_reg* h)
{
    delete h;
    return KDE_OK;
}

// Kinect.cpp:71-75: SetViewPoint(*Image_Generator) uses the factory calibration of the device; here it is the caller's
extern "C" int kde_reg_set_calibration(kde_reg* h, const double* Kd9, const double* Kc9, const double* R9, const double* t3)
{
    const char* who = "kde_reg_set_calibration";
    KDE_REQUIRE(h && Kd9 && Kc9 && R9 && t3, "%s: null argument", who);
    RegCalib c{};
    c.fxd = (float)Kd9[0]; c.fyd = (float)Kd9[4]; c.cxd = (float)Kd9[2]; c.cyd = (float)Kd9[5];
    c.fxc = (float)Kc9[0]; c.fyc = (float)Kc9[4]; c.cxc = (float)Kc9[2]; c.cyc = (float)Kc9[5];
    for (int i = 0; i < 9; i++) {
        KDE_REQUIRE(std::isfinite(Kd9[i]) && std::isfinite(Kc9[i]) && std::isfinite(R9[i]), "%s: a non-finite calibration value", who);
        c.r[i] = (float)R9[i];
        KDE_REQUIRE(std::isfinite(c.r[i]), "%s: a non-finite calibration value", who);
    }
    for (int i = 0; i < 3; i++) {
        c.t[i] = (float)t3[i];
        KDE_REQUIRE(std::isfinite(t3[i]) && std::isfinite(c.t[i]), "%s: a non-finite calibration value", who);
    }
    KDE_REQUIRE(std::isfinite(c.fxd) && std::isfinite(c.fyd) && std::isfinite(c.cxd) && std::isfinite(c.cyd) && std::isfinite(c.fxc) &&
                    std::isfinite(c.fyc) && std::isfinite(c.cxc) && std::isfinite(c.cyc),
                "%s: a non-finite calibration value", who);
    KDE_REQUIRE(c.fxd > 0.0f && c.fyd > 0.0f && c.fxc > 0.0f && c.fyc > 0.0f, "%s: fx and fy must be > 0", who);
    h->c = c;
    h->calibrated = true;
    return KDE_OK;
}

// what register_batch and color_to_depth_batch ask of the object, n and the depth map alike
static int check_depth(const kde_reg* h, const char* who, int n, const void* depth_dev, int depth_format)
{
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_depth_in(who, depth_dev, depth_format));
    KDE_REQUIRE(h->calibrated, "%s: kde_reg_set_calibration was not called", who);
    return KDE_OK;
}

static RegLaunch launch_of(const kde_reg* h, int n, const void* depth_dev, int depth_format)
{
    RegLaunch a{};
    a.n = n;
    a.depth = depth_dev;
    a.depth_format = depth_format;
    a.wd = h->width;
    a.hd = h->height;
    a.wc = h->color_w;
    a.hc = h->color_h;
    a.c = h->c;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    a.max_splat = h->p.max_splat;
    return a;
}

// Kinect.cpp:71-75: the depth frames as the image generator's viewpoint sees them, n at once
extern "C" int kde_reg_register_batch(kde_reg* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev,
                                      void* stream)
{
    const char* who = "kde_reg_register_batch";
    KDE_REQUIRE(h && depth_dev, "%s: null argument", who);
    KDE_TRY(check_depth(h, who, n, depth_dev, depth_format));
    KDE_TRY(check_depth_out(who, out_dev, out_format));
    KDE_TRY(check_has_device(who, h->device));
    RegLaunch a = launch_of(h, n, depth_dev, depth_format);
    a.zbuf = h->zbuf.p;
    a.filled = h->filled.p;
    a.out = h->stage.written(out_dev);
    a.out_format = out_format;
    KDE_TRY(launch_reg(a, as_stream(stream)));
    h->stage.finished(n, out_format, a.out);
    return KDE_OK;
}

// Kinect.cpp:71-75 the other way round: the colour image as the depth camera sees it
extern "C" int kde_reg_color_to_depth_batch(kde_reg* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev,
                                            int bgr_frames, uint8_t* out_bgr_dev, void* stream)
{
    const char* who = "kde_reg_color_to_depth_batch";
    KDE_REQUIRE(h && depth_dev && bgr_dev && out_bgr_dev, "%s: null argument", who);
    KDE_TRY(check_depth(h, who, n, depth_dev, depth_format));
    KDE_TRY(check_bgr_frames(who, bgr_frames, n));
    KDE_TRY(check_has_device(who, h->device));
    return launch_reg_gather(launch_of(h, n, depth_dev, depth_format), bgr_dev, bgr_frames, out_bgr_dev, as_stream(stream));
}

// Kinect.cpp:71-75: the registered frames of the last call (out_dev of that call, or the object-owned buffer) on the device,
// and, as Kinect.cpp hands its frames to the host, the same in pinned memory, ready when the call returns
KDE_STAGE_DEPTH_GETTERS(kde_reg_depth_device, kde_reg_depth_host, kde_reg, "kde_reg_register_batch", (size_t)h->color_w * h->color_h)

// Kinect.cpp:71-75: how many pixels of the image viewpoint got a depth, per frame, on the device and in pinned memory
KDE_STAGE_COUNT_GETTERS(kde_reg_filled_device, kde_reg_filled_host, kde_reg, "kde_reg_register_batch", h->filled.p, h->filled_host)
