// kde_api_undist.cpp — LensUndistortion (kde_undist_*): frames of a camera with lens distortion resampled into the pinhole view
// every other class assumes, for a batch of frames on the device (undist_kernels.hip).  No reference counterpart: the
// reference's frames come through OpenNI from a Kinect v1 and are used as they are.
#include "kde_handles.h"

struct kde_undist {
    int device = -1;                        // -1: created on a host without a device (no buffers; the launches refuse)
    int width = 0, height = 0, max_batch = 1;   // the source (distorted) frame
    int out_w = 0, out_h = 0;
    kde_undist_params p{};
    UndistCalib c{};
    bool calibrated = false;
    bool map_valid = false;                 // map holds the map of c
    DepthStage stage;                       // the last depth_batch; depth [max_batch][out_h][out_w]
    DevBuf<uint32_t> filled;                // [max_batch]
    DevBuf<float2> map;                     // [out_h][out_w] of (us, vs)
    PinnedBuf<uint32_t> filled_host;
};

static const kde_undist_params kUndistDefaults = {0.0f, FLT_MAX, 0, 0.0f};

// every finite positive depth, the nearest sample: nothing is blended unless the caller names a max_gap
extern "C" int kde_undist_default_params(kde_undist_params* p)
{
    KDE_REQUIRE(p, "kde_undist_default_params: null argument");
    *p = kUndistDefaults;
    return KDE_OK;
}

extern "C" int kde_undist_create(kde_undist** out, int src_w, int src_h, int out_w, int out_h, int max_batch, const kde_undist_params* p)
{
    const char* who = "kde_undist_create";
    KDE_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    KDE_TRY(check_frame_batch(who, src_w, src_h, max_batch));
    KDE_REQUIRE(frame_ok(out_w, out_h), "%s: bad size", who);
    KDE_REQUIRE(src_w <= kRegMaxSide && src_h <= kRegMaxSide && out_w <= kRegMaxSide && out_h <= kRegMaxSide,
                "%s: a side above %d is not an exact float", who, kRegMaxSide);
    const kde_undist_params q = p ? *p : kUndistDefaults;
    KDE_TRY(check_z_range(who, q.z_min, q.z_max));
    KDE_REQUIRE(q.depth_interp == 0 || q.depth_interp == 1, "%s: depth_interp=%d is neither 0 (nearest) nor 1 (guarded bilinear)", who,
                q.depth_interp);
    KDE_REQUIRE(q.depth_interp == 0 || (std::isfinite(q.max_gap) && q.max_gap > 0.0f),
                "%s: depth_interp=1 needs a finite max_gap > 0 (millimetres), got %g", who, (double)q.max_gap);
    kde_undist* h = new_handle<kde_undist>(src_w, src_h, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    h->out_w = out_w;
    h->out_h = out_h;
    h->p = q;
    if (h->device >= 0) {
        const size_t px = (size_t)out_w * out_h;
        int rc = h->filled.alloc((size_t)max_batch);
        if (rc == KDE_OK) rc = h->stage.depth.alloc((size_t)max_batch * px);
        if (rc == KDE_OK) rc = h->map.alloc(px);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_undist_destroy(kde_undist* h)
{
    delete h;
    return KDE_OK;
}

extern "C" int kde_undist_set_calibration(kde_undist* h, const double* K9, const double* dist8, const double* Knew9)
{
    const char* who = "kde_undist_set_calibration";
    KDE_REQUIRE(h && K9 && dist8, "%s: null argument", who);
    const double* Kn = Knew9 ? Knew9 : K9;
    UndistCalib c{};
    c.fx = (float)K9[0]; c.fy = (float)K9[4]; c.cx = (float)K9[2]; c.cy = (float)K9[5];
    c.fxn = (float)Kn[0]; c.fyn = (float)Kn[4]; c.cxn = (float)Kn[2]; c.cyn = (float)Kn[5];
    float k[8];
    for (int i = 0; i < 9; i++) KDE_REQUIRE(std::isfinite(K9[i]) && std::isfinite(Kn[i]), "%s: a non-finite calibration value", who);
    for (int i = 0; i < 8; i++) {
        k[i] = (float)dist8[i];
        KDE_REQUIRE(std::isfinite(dist8[i]) && std::isfinite(k[i]), "%s: a non-finite distortion coefficient", who);
    }
    KDE_REQUIRE(std::isfinite(c.fx) && std::isfinite(c.fy) && std::isfinite(c.cx) && std::isfinite(c.cy) && std::isfinite(c.fxn) &&
                    std::isfinite(c.fyn) && std::isfinite(c.cxn) && std::isfinite(c.cyn),
                "%s: a non-finite calibration value", who);
    KDE_REQUIRE(c.fx > 0.0f && c.fy > 0.0f && c.fxn > 0.0f && c.fyn > 0.0f, "%s: fx and fy must be > 0", who);
    c.k1 = k[0]; c.k2 = k[1]; c.p1 = k[2]; c.p2 = k[3]; c.k3 = k[4]; c.k4 = k[5]; c.k5 = k[6]; c.k6 = k[7];
    h->c = c;
    h->calibrated = true;
    h->map_valid = false;
    return KDE_OK;
}

static UndistLaunch launch_of(const kde_undist* h, int n)
{
    UndistLaunch a{};
    a.n = n;
    a.sw = h->width;
    a.sh = h->height;
    a.ow = h->out_w;
    a.oh = h->out_h;
    a.c = h->c;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    a.depth_interp = h->p.depth_interp;
    a.max_gap = h->p.max_gap;
    return a;
}

extern "C" int kde_undist_color_batch(kde_undist* h, int n, const uint8_t* bgr_dev, int bgr_frames, uint8_t* out_bgr_dev, void* stream)
{
    const char* who = "kde_undist_color_batch";
    KDE_REQUIRE(h && bgr_dev && out_bgr_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_bgr_frames(who, bgr_frames, n));
    KDE_REQUIRE(h->calibrated, "%s: kde_undist_set_calibration was not called", who);
    KDE_TRY(check_has_device(who, h->device));
    return launch_undist_color(launch_of(h, n), bgr_dev, bgr_frames, out_bgr_dev, as_stream(stream));
}

extern "C" int kde_undist_depth_batch(kde_undist* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev,
                                      void* stream)
{
    const char* who = "kde_undist_depth_batch";
    KDE_REQUIRE(h && depth_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_depth_in(who, depth_dev, depth_format));
    KDE_TRY(check_depth_out(who, out_dev, out_format));
    KDE_REQUIRE(h->calibrated, "%s: kde_undist_set_calibration was not called", who);
    KDE_TRY(check_has_device(who, h->device));
    UndistLaunch a = launch_of(h, n);
    a.depth = depth_dev;
    a.depth_format = depth_format;
    a.out = h->stage.written(out_dev);
    a.out_format = out_format;
    a.filled = h->filled.p;
    KDE_TRY(launch_undist_depth(a, as_stream(stream)));
    h->stage.finished(n, out_format, a.out);
    return KDE_OK;
}

KDE_STAGE_DEPTH_GETTERS(kde_undist_depth_device, kde_undist_depth_host, kde_undist, "kde_undist_depth_batch", (size_t)h->out_w * h->out_h)
KDE_STAGE_COUNT_GETTERS(kde_undist_filled_device, kde_undist_filled_host, kde_undist, "kde_undist_depth_batch", h->filled.p, h->filled_host)

// the map of the calibration in force: computed by U3 on `stream` at the first request after kde_undist_set_calibration
extern "C" int kde_undist_map_device(kde_undist* h, void* stream, const float** out)
{
    const char* who = "kde_undist_map_device";
    KDE_REQUIRE(h && out, "%s: null argument", who);
    KDE_REQUIRE(h->calibrated, "%s: kde_undist_set_calibration was not called", who);
    KDE_TRY(check_has_device(who, h->device));
    if (!h->map_valid) {
        KDE_TRY(launch_undist_map(launch_of(h, 1), h->map.p, as_stream(stream)));
        h->map_valid = true;
    }
    *out = reinterpret_cast<const float*>(h->map.p);
    return KDE_OK;
}
