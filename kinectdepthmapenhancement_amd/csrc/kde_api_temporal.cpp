// kde_api_temporal.cpp — DepthTemporalFilter (kde_temporal_*): a per-pixel running depth over the consecutive frames of a
// sequence, for a batch of frames on the device (temporal_kernels.hip).  The one depth stage whose object carries state from a
// call to the next.  No reference counterpart: kde_buffer2d_update_sequence folds n frames into one plain average.
#include "kde_handles.h"

struct kde_temporal {
    int device = -1;                        // -1: created on a host without a device (no buffers; the launch refuses)
    int width = 0, height = 0, max_batch = 1;
    kde_temporal_params p{};
    int pixels = 0, unroll = 0;             // kde_temporal_set_shape (0, 0: temporal_shape chooses)
    DepthStage stage;                       // the last filter_batch; depth [max_batch][H][W]
    DevBuf<float> value;                    // [H][W]: the state
    DevBuf<uint32_t> hist;                  // [H][W]
    DevBuf<uint32_t> partial;               // [max_batch][temporal_waves(W * H, 1)][2]: room for every shape
    DevBuf<uint32_t> counts;                // smoothed[max_batch], jumped[max_batch], held[max_batch], changed[max_batch]
    PinnedBuf<uint32_t> smoothed_host, jumped_host, held_host, changed_host;
};

static const kde_temporal_params kTemporalDefaults = {0.4f, 10.0f, 0.02f, 3, 48, 0.0f, FLT_MAX};
static const char* const kBatch = "kde_temporal_filter_batch";

// 0.4 of a linked sample; a link holds within 10 mm + 2 % of the nearer depth (DepthSpeckleFilter's); a hole is held behind 3
// valid frames of the last 8; a colour step above 48 forgets; every finite positive depth
extern "C" int kde_temporal_default_params(kde_temporal_params* p)
{
    KDE_REQUIRE(p, "kde_temporal_default_params: null argument");
    *p = kTemporalDefaults;
    return KDE_OK;
}

static int check_diff(const char* who, const char* name, float v)
{
    KDE_REQUIRE(std::isfinite(v) && v >= 0.0f, "%s: %s=%g must be finite and >= 0", who, name, (double)v);
    return KDE_OK;
}

extern "C" int kde_temporal_create(kde_temporal** out, int width, int height, int max_batch, const kde_temporal_params* p)
{
    const char* who = "kde_temporal_create";
    KDE_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    KDE_TRY(check_frame_batch(who, width, height, max_batch));
    const kde_temporal_params q = p ? *p : kTemporalDefaults;
    KDE_REQUIRE(q.alpha > 0.0f && q.alpha <= 1.0f, "%s: alpha=%g outside (0, 1]", who, (double)q.alpha);   // a NaN fails
    KDE_TRY(check_diff(who, "max_diff", q.max_diff));
    KDE_TRY(check_diff(who, "rel_diff", q.rel_diff));
    KDE_REQUIRE(q.persist_min >= 0 && q.persist_min <= 8, "%s: persist_min=%d outside 0..8", who, q.persist_min);
    KDE_REQUIRE(q.color_thresh >= 0 && q.color_thresh <= kColourRange - 1, "%s: color_thresh=%d outside 0..%d", who, q.color_thresh, kColourRange - 1);
    KDE_TRY(check_z_range(who, q.z_min, q.z_max));
    kde_temporal* h = new_handle<kde_temporal>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    h->p = q;
    if (h->device >= 0) {
        const size_t px = (size_t)width * height;
        int rc = h->counts.alloc((size_t)max_batch * 4);
        if (rc == KDE_OK) rc = h->partial.alloc((size_t)max_batch * temporal_waves(px, 1) * 2);
        if (rc == KDE_OK) rc = h->stage.depth.alloc((size_t)max_batch * px);
        if (rc == KDE_OK) rc = h->value.alloc(px);
        if (rc == KDE_OK) rc = h->hist.alloc(px);
        // the state is empty before the first call on any stream
        if (rc == KDE_OK) rc = launch_temporal_reset(h->value.p, h->hist.p, px, nullptr);
        if (rc == KDE_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(KDE_ERR_HIP, "%s: the state could not be zeroed", who);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_temporal_destroy(kde_temporal* h)
{
    delete h;
    return KDE_OK;
}

static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return !(a0 + a_bytes <= b0 || b0 + b_bytes <= a0);
}

extern "C" int kde_temporal_filter_batch(kde_temporal* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev, int out_format,
                                         void* out_dev, void* stream)
{
    const char* who = kBatch;
    KDE_REQUIRE(h && depth_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_depth_in(who, depth_dev, depth_format));
    KDE_TRY(check_depth_out(who, out_dev, out_format));
    // A thread reads its own pixels of a frame before it writes them, and nobody else's: exactly in place is safe.  Any other
    // overlap lets one thread write what another has yet to read.
    const size_t px = (size_t)h->width * h->height, all = (size_t)n * px;
    const size_t in_bytes = all * depth_element(depth_format), out_bytes = all * depth_element(out_format);
    void* const w = h->stage.written(out_dev);
    const char* const which = out_dev ? "out_dev" : "the object-owned output buffer, which out_dev == NULL selects,";
    if (w && !(out_dev == depth_dev && out_format == depth_format))
        KDE_REQUIRE(!overlap(w, out_bytes, depth_dev, in_bytes),
                    "%s: %s overlaps depth_dev (in place is supported only with out_dev == depth_dev and out_format == depth_format)", who, which);
    if (w && bgr_dev) KDE_REQUIRE(!overlap(w, out_bytes, bgr_dev, all * 3), "%s: %s overlaps bgr_dev", who, which);
    KDE_TRY(check_has_device(who, h->device));
    TemporalLaunch a{};
    a.n = n;
    a.w = h->width;
    a.h = h->height;
    if (h->pixels) {
        a.pixels = h->pixels;
        a.unroll = h->unroll;
    } else {
        temporal_shape(px, n, &a.pixels, &a.unroll);
    }
    a.alpha = h->p.alpha;
    a.max_diff = h->p.max_diff;
    a.rel_diff = h->p.rel_diff;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    a.persist_min = h->p.persist_min;
    a.color_thresh = h->p.color_thresh;
    a.depth = depth_dev;
    a.depth_format = depth_format;
    a.bgr = bgr_dev;
    a.out = w;
    a.out_format = out_format;
    a.nt_store = past_cache(kSiteTemporal, in_bytes + out_bytes + (bgr_dev ? all * 3 : 0));
    a.value = h->value.p;
    a.hist = h->hist.p;
    a.partial = h->partial.p;
    a.counts = h->counts.p;
    a.max_batch = h->max_batch;
    KDE_TRY(launch_temporal(a, as_stream(stream)));
    h->stage.finished(n, out_format, a.out);
    return KDE_OK;
}

extern "C" int kde_temporal_reset(kde_temporal* h, void* stream)
{
    const char* who = "kde_temporal_reset";
    KDE_REQUIRE(h, "%s: null argument", who);
    KDE_TRY(check_has_device(who, h->device));
    KDE_TRY(launch_temporal_reset(h->value.p, h->hist.p, (size_t)h->width * h->height, as_stream(stream)));
    h->stage.finished(0, KDE_DEPTH_F32, nullptr);           // the getters ask for a call again
    return KDE_OK;
}

extern "C" int kde_temporal_state_device(kde_temporal* h, float** value, uint32_t** hist)
{
    KDE_REQUIRE(h && value && hist, "kde_temporal_state_device: null argument");
    *value = h->value.p;
    *hist = h->hist.p;
    return KDE_OK;
}

extern "C" int kde_temporal_set_shape(kde_temporal* h, int pixels_per_thread, int unroll)
{
    const char* who = "kde_temporal_set_shape";
    KDE_REQUIRE(h, "%s: null argument", who);
    const int P = pixels_per_thread, U = unroll;
    KDE_REQUIRE((P == 0 && U == 0) || ((P == 1 || P == 2 || P == 4 || P == 8) && (U == 1 || U == 2 || U == 4)),
                "%s: pixels_per_thread=%d, unroll=%d is neither 0, 0 nor one of 1, 2, 4, 8 with one of 1, 2, 4", who, P, U);
    h->pixels = P;
    h->unroll = U;
    return KDE_OK;
}

extern "C" int kde_temporal_shape(kde_temporal* h, int n, int* pixels_per_thread, int* unroll)
{
    const char* who = "kde_temporal_shape";
    KDE_REQUIRE(h && pixels_per_thread && unroll, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    if (h->pixels) {
        *pixels_per_thread = h->pixels;
        *unroll = h->unroll;
    } else {
        temporal_shape((size_t)h->width * h->height, n, pixels_per_thread, unroll);
    }
    return KDE_OK;
}

KDE_STAGE_DEPTH_GETTERS(kde_temporal_depth_device, kde_temporal_depth_host, kde_temporal, kBatch, (size_t)h->width * h->height)
KDE_STAGE_COUNT_GETTERS(kde_temporal_smoothed_device, kde_temporal_smoothed_host, kde_temporal, kBatch, h->counts.p, h->smoothed_host)
KDE_STAGE_COUNT_GETTERS(kde_temporal_jumped_device, kde_temporal_jumped_host, kde_temporal, kBatch, h->counts.p + h->max_batch, h->jumped_host)
KDE_STAGE_COUNT_GETTERS(kde_temporal_held_device, kde_temporal_held_host, kde_temporal, kBatch, h->counts.p + 2 * (size_t)h->max_batch, h->held_host)
KDE_STAGE_COUNT_GETTERS(kde_temporal_changed_device, kde_temporal_changed_host, kde_temporal, kBatch, h->counts.p + 3 * (size_t)h->max_batch,
                        h->changed_host)
