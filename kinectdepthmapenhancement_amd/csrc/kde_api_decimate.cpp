// kde_api_decimate.cpp — DepthDecimation (kde_decimate_*): depth frames and their colour guides made `factor` times smaller each
// way, hole-aware and edge-aware, for a batch of frames on the device (decimate_kernels.hip).  The one depth stage whose output
// is smaller than its input.  No reference counterpart: every class of the reference runs at the size of the frame it is given.
#include "kde_handles.h"

struct kde_decimate {
    int device = -1;                        // -1: created on a host without a device (no buffers; the launch refuses)
    int width = 0, height = 0, max_batch = 1;   // the source frame
    int out_w = 0, out_h = 0;
    kde_decimate_params p{};
    unsigned groups = 0;                    // workgroups per frame
    DepthStage stage;                       // the last depth_batch; depth [max_batch][out_h][out_w]
    DevBuf<uint32_t> partial;               // [max_batch][groups][2]
    DevBuf<uint32_t> counts;                // filled[max_batch], mixed[max_batch]
    PinnedBuf<uint32_t> filled_host, mixed_host;
};

static const kde_decimate_params kDecimateDefaults = {2, KDE_DECIMATE_MEDIAN, 1, 0.0f, 0.0f, FLT_MAX};
static const char* const kBatch = "kde_decimate_depth_batch";
constexpr int kDecimateMinFactor = 2, kDecimateMaxFactor = 8;

// half the size each way, the lower median of at least one valid sample, no guard, every finite positive depth
extern "C" int kde_decimate_default_params(kde_decimate_params* p)
{
    KDE_REQUIRE(p, "kde_decimate_default_params: null argument");
    *p = kDecimateDefaults;
    return KDE_OK;
}

extern "C" int kde_decimate_create(kde_decimate** out, int src_w, int src_h, int max_batch, const kde_decimate_params* p)
{
    const char* who = "kde_decimate_create";
    KDE_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    KDE_TRY(check_frame_batch(who, src_w, src_h, max_batch));
    KDE_REQUIRE(src_w <= kRegMaxSide && src_h <= kRegMaxSide, "%s: a side above %d is refused (the depth stages' bound)", who, kRegMaxSide);
    const kde_decimate_params q = p ? *p : kDecimateDefaults;
    KDE_REQUIRE(q.factor >= kDecimateMinFactor && q.factor <= kDecimateMaxFactor, "%s: factor=%d outside %d..%d", who, q.factor, kDecimateMinFactor,
                kDecimateMaxFactor);
    KDE_REQUIRE(q.mode == KDE_DECIMATE_MEDIAN || q.mode == KDE_DECIMATE_MEAN, "%s: mode=%d is neither KDE_DECIMATE_MEDIAN (0) nor KDE_DECIMATE_MEAN (1)",
                who, q.mode);
    KDE_REQUIRE(q.min_valid >= 1 && q.min_valid <= q.factor * q.factor, "%s: min_valid=%d outside 1..factor^2=%d", who, q.min_valid,
                q.factor * q.factor);
    KDE_TRY(check_max_gap(who, q.max_gap));
    KDE_TRY(check_z_range(who, q.z_min, q.z_max));
    kde_decimate* h = new_handle<kde_decimate>(src_w, src_h, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    h->p = q;
    h->out_w = (src_w + q.factor - 1) / q.factor;
    h->out_h = (src_h + q.factor - 1) / q.factor;
    h->groups = decimate_groups(h->out_w, h->out_h, q.factor);
    if (h->device >= 0) {
        int rc = h->counts.alloc((size_t)max_batch * 2);
        if (rc == KDE_OK) rc = h->partial.alloc((size_t)max_batch * h->groups * 2);
        if (rc == KDE_OK) rc = h->stage.depth.alloc((size_t)max_batch * h->out_w * h->out_h);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_decimate_destroy(kde_decimate* h)
{
    delete h;
    return KDE_OK;
}

extern "C" int kde_decimate_out_size(kde_decimate* h, int* out_w, int* out_h)
{
    KDE_REQUIRE(h && out_w && out_h, "kde_decimate_out_size: null argument");
    *out_w = h->out_w;
    *out_h = h->out_h;
    return KDE_OK;
}

// the pixel-centre rule: source pixel x shows at (x + 0.5) / k - 0.5 of the small image
extern "C" int kde_decimate_intrinsics(kde_decimate* h, const double* K_in, double* K_out)
{
    KDE_REQUIRE(h && K_in && K_out, "kde_decimate_intrinsics: null argument");
    const double k = (double)h->p.factor;
    double r[9];
    for (int i = 0; i < 9; i++) r[i] = K_in[i];
    r[0] = K_in[0] / k;
    r[1] = K_in[1] / k;
    r[2] = (K_in[2] + 0.5) / k - 0.5;
    r[3] = K_in[3] / k;
    r[4] = K_in[4] / k;
    r[5] = (K_in[5] + 0.5) / k - 0.5;
    for (int i = 0; i < 9; i++) K_out[i] = r[i];            // K_out may be K_in
    return KDE_OK;
}

static DecimateLaunch launch_of(const kde_decimate* h, int n)
{
    DecimateLaunch a{};
    a.n = n;
    a.sw = h->width;
    a.sh = h->height;
    a.ow = h->out_w;
    a.oh = h->out_h;
    a.factor = h->p.factor;
    a.mode = h->p.mode;
    a.min_valid = h->p.min_valid;
    a.max_gap = h->p.max_gap;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    return a;
}

extern "C" int kde_decimate_depth_batch(kde_decimate* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev, void* stream)
{
    const char* who = kBatch;
    KDE_REQUIRE(h && depth_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_depth_in(who, depth_dev, depth_format));
    KDE_TRY(check_depth_out(who, out_dev, out_format));
    // a workgroup reads a tile of the source while others write their pixels: any overlap lets one write what another has yet to read
    KDE_TRY(h->stage.check_not_in_place(who, depth_dev, depth_format, out_dev, out_format, (size_t)n * h->width * h->height,
                                        (size_t)n * h->out_w * h->out_h));
    KDE_TRY(check_has_device(who, h->device));
    DecimateLaunch a = launch_of(h, n);
    a.depth = depth_dev;
    a.depth_format = depth_format;
    a.out = h->stage.written(out_dev);
    a.out_format = out_format;
    a.partial = h->partial.p;
    a.filled = h->counts.p;
    a.mixed = h->counts.p + h->max_batch;
    KDE_TRY(launch_decimate(a, as_stream(stream)));
    h->stage.finished(n, out_format, a.out);
    return KDE_OK;
}

extern "C" int kde_decimate_color_batch(kde_decimate* h, int n, const uint8_t* bgr_dev, uint8_t* out_bgr_dev, void* stream)
{
    const char* who = "kde_decimate_color_batch";
    KDE_REQUIRE(h && bgr_dev && out_bgr_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(bgr_dev), b1 = b0 + (size_t)n * h->width * h->height * 3;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out_bgr_dev), o1 = o0 + (size_t)n * h->out_w * h->out_h * 3;
    KDE_REQUIRE(o1 <= b0 || b1 <= o0, "%s: out_bgr_dev overlaps bgr_dev (in place is not supported)", who);
    KDE_TRY(check_has_device(who, h->device));
    DecimateLaunch a = launch_of(h, n);
    a.bgr = bgr_dev;
    a.out_bgr = out_bgr_dev;
    return launch_decimate_color(a, as_stream(stream));
}

KDE_STAGE_DEPTH_GETTERS(kde_decimate_depth_device, kde_decimate_depth_host, kde_decimate, kBatch, (size_t)h->out_w * h->out_h)
KDE_STAGE_COUNT_GETTERS(kde_decimate_filled_device, kde_decimate_filled_host, kde_decimate, kBatch, h->counts.p, h->filled_host)
KDE_STAGE_COUNT_GETTERS(kde_decimate_mixed_device, kde_decimate_mixed_host, kde_decimate, kBatch, h->counts.p + h->max_batch, h->mixed_host)
