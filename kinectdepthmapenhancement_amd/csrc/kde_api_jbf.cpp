// kde_api_jbf.cpp — JointBilateralFilter (kde_jbf_*), its host-fed streaming form (kde_jbf_feed_*) and
// MarkovRandomField (kde_mrf_*).  struct kde_jbf is in kde_handles.h: the KinectDepthEnhancement pipeline reads it.
#include "kde_feed_ring.h"

// =====================================================================================================
// JointBilateralFilter
// =====================================================================================================
extern "C" int kde_jbf_default_params(kde_jbf_params* p)
{
    KDE_REQUIRE(p, "kde_jbf_default_params: null argument");
    p->window_size = 5;              // JointBilateralFilter.cpp:3
    p->spatial_sigma = 70.0f;        // :4
    p->color_sigma = 50.0f;          // :5
    p->depth_sigma = 20.0f;          // :6
    p->presmooth = 1;                // JointBilateralFilter.cu:285
    p->presmooth_kernel_size = 5;
    p->presmooth_sigma_color = 30.0f;
    p->presmooth_sigma_spatial = 30.0f;
    return KDE_OK;
}

static int jbf_create_impl(kde_jbf** out, int width, int height, int max_batch, const kde_jbf_params* params);

extern "C" int kde_jbf_create(kde_jbf** out, int width, int height, int max_batch, const kde_jbf_params* params)
{
    // the only entry point that builds std::vectors: nothing may cross the C boundary (kde_hip.h: "never aborts")
    try {
        return jbf_create_impl(out, width, height, max_batch, params);
    } catch (const std::bad_alloc&) {
        if (out) *out = nullptr;
        return fail(KDE_ERR_NOMEM, "kde_jbf_create: out of host memory");
    } catch (...) {
        if (out) *out = nullptr;
        return fail(KDE_ERR_INVALID, "kde_jbf_create: unexpected exception");
    }
}

static int jbf_create_impl(kde_jbf** out, int width, int height, int max_batch, const kde_jbf_params* params)
{
    KDE_REQUIRE(out, "kde_jbf_create: null out");
    *out = nullptr;
    KDE_REQUIRE(frame_ok(width, height), "kde_jbf_create: bad size %dx%d", width, height);
    KDE_REQUIRE(batch_ok(max_batch), "kde_jbf_create: max_batch must be in 1..65535");
    kde_jbf_params p;
    kde_jbf_default_params(&p);
    if (params) p = *params;
    KDE_REQUIRE(p.window_size >= 1 && p.window_size <= 31 && (p.window_size & 1), "kde_jbf_create: window_size must be odd in 1..31");
    KDE_REQUIRE(p.spatial_sigma == p.spatial_sigma && p.color_sigma >= 0.0f && p.depth_sigma >= 0.0f && p.spatial_sigma != 0.0f,
                "kde_jbf_create: sigmas must be >= 0 (spatial != 0)");
    struct Guard {                      // frees the half-built handle on every early return and on an exception
        kde_jbf* h;
        ~Guard() { delete h; }
    } guard{new_handle<kde_jbf>(width, height, max_batch)};
    kde_jbf* h = guard.h;
    if (!h) return fail(KDE_ERR_NOMEM, "kde_jbf_create: out of host memory");
    h->p = p;
    const int w = p.window_size;
    h->table.resize((size_t)w * w);
    spatial_table(w, p.spatial_sigma, h->table.data());
    std::vector<float> eff(h->table);
    for (float& v : eff)
        if (v == 0.0f) v = 1.0f;   // "if(spatial != 0) filter *= spatial" (JointBilateralFilter.cu:30-31)
    const size_t px = (size_t)width * height;
    int rc = h->s_eff.alloc(eff.size());
    if (rc == KDE_OK) rc = h->filtered.alloc(px * max_batch);
    if (rc == KDE_OK) rc = h->smooth.alloc(px * 3 * max_batch);
    if (rc == KDE_OK && hipMemcpy(h->s_eff.p, eff.data(), eff.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(KDE_ERR_HIP, "kde_jbf_create: table upload failed");
    if (rc == KDE_OK && jbf_fast_needs_device_table(w)) {
        std::vector<float> pk((size_t)2 * w * w);
        jbf_fast_fill_table(w, h->table.data(), /*packed=*/true, pk.data());
        rc = h->log2_pk.alloc(pk.size());
        if (rc == KDE_OK && hipMemcpy(h->log2_pk.p, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(KDE_ERR_HIP, "kde_jbf_create: log2 table upload failed");
    }
    // thresholds of the "factor == 0 -> skipped" rule (JointBilateralFilter.cu:32-33, 65-68)
    const float xz = exp_zero_threshold();
    h->color_den = 2 * (p.color_sigma * p.color_sigma);
    h->depth_den = 2.0f * (p.depth_sigma * p.depth_sigma);
    h->cd_skip = INT_MAX;
    if (p.color_sigma != 0.0f) h->cd_skip = smallest_cd_reaching(h->color_den, xz);   // 195076 = never reached
    h->d2_skip = p.depth_sigma != 0.0f ? smallest_q_reaching(h->depth_den, xz) : INFINITY;
    // K0 table: weight(space2, n1) = expf(space2*ss + n1^2*sc), the expression of OpenCV's kernel
    if (rc == KDE_OK && p.presmooth) {
        float sc_ = p.presmooth_sigma_color, ss_ = p.presmooth_sigma_spatial;
        sc_ = (sc_ <= 0) ? 1 : sc_;
        ss_ = (ss_ <= 0) ? 1 : ss_;
        int radius = (p.presmooth_kernel_size <= 0) ? (int)rint((double)ss_ * 1.5) : p.presmooth_kernel_size / 2;
        radius = radius > 1 ? radius : 1;
        // radii 1..4 have tuned kernels (LDS-resident weight table); larger ones (the OpenCV function takes any kernel
        // size) run the generic kernel with the table in global memory.  64 bounds the table at 12.5 MB.
        if (radius > 64) return fail(KDE_ERR_UNSUPPORTED, "kde_jbf_create: pre-smoothing radius %d > 64", radius);
        h->pre_radius = radius;
        h->pre_grid_cap = presmooth_resident_blocks(radius);
        const float ss = -0.5f / (ss_ * ss_), sc = -0.5f / (sc_ * sc_);
        std::vector<float> lut((size_t)(radius * radius + 1) * 766);
        for (int s2 = 0; s2 <= radius * radius; s2++)
            for (int n1 = 0; n1 < 766; n1++) {
                const float fn = (float)n1;
                lut[(size_t)s2 * 766 + n1] = expf((float)s2 * ss + (fn * fn) * sc);
            }
        rc = h->pre_lut.alloc(lut.size());
        if (rc == KDE_OK && hipMemcpy(h->pre_lut.p, lut.data(), lut.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(KDE_ERR_HIP, "kde_jbf_create: lut upload failed");
    }
    if (rc != KDE_OK) return rc;
    guard.h = nullptr;
    *out = h;
    return KDE_OK;
}

extern "C" int kde_jbf_destroy(kde_jbf* h)
{
    delete h;
    return KDE_OK;
}

static void jbf_fill_launch(const kde_jbf* h, JbfLaunch& a);

static int jbf_filter(kde_jbf* h, int n, const float* depth, const uint8_t* guide, float* out, hipStream_t s)
{
    JbfLaunch a;
    jbf_fill_launch(h, a);
    a.n = n;
    a.depth = depth;
    a.guide = guide;
    a.out = out;
    return launch_jbf(a, s);
}

static void jbf_fill_launch(const kde_jbf* h, JbfLaunch& a)
{
    a.width = h->width;
    a.height = h->height;
    a.n = 0;
    a.window = h->p.window_size;
    a.depth = nullptr;
    a.guide = nullptr;
    a.out = nullptr;
    a.s_eff = h->s_eff.p;
    a.table_host = h->table.data();
    a.log2_pk_dev = h->log2_pk.p;
    a.spatial_sigma = h->p.spatial_sigma;
    a.color_sigma = h->p.color_sigma;
    a.depth_sigma = h->p.depth_sigma;
    a.color_den = h->color_den;
    a.depth_den = h->depth_den;
    a.cd_skip = h->cd_skip;
    a.d2_skip = h->d2_skip;
    a.variant = h->variant;
}

static int jbf_presmooth(kde_jbf* h, int n, const uint8_t* bgr, uint8_t* dst, hipStream_t s)
{
    PresmoothLaunch a;
    a.width = h->width;
    a.height = h->height;
    a.n = n;
    a.radius = h->pre_radius;
    a.src = bgr;
    a.dst = dst;
    a.lut = h->pre_lut.p;
    a.grid_cap = h->pre_grid_cap;
    return launch_presmooth(a, s);
}

extern "C" int kde_jbf_process_batch(kde_jbf* h, int n, const float* depth_dev, const uint8_t* bgr_dev,
                                     float* filtered_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev && bgr_dev, "kde_jbf_process_batch: null argument");
    KDE_ON_DEVICE(h, "kde_jbf_process_batch");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "kde_jbf_process_batch: n=%d outside 1..max_batch=%d", n, h->max_batch);
    hipStream_t s = as_stream(stream);
    float* out = filtered_dev ? filtered_dev : h->filtered.p;
    const uint8_t* guide = bgr_dev;
    if (h->p.presmooth) {
        KDE_TRY(jbf_presmooth(h, n, bgr_dev, h->smooth.p, s));
        guide = h->smooth.p;
    }
    KDE_TRY(jbf_filter(h, n, depth_dev, guide, out, s));
    if (!filtered_dev) h->n_last = n;       // results in a caller's buffer are the caller's: the host getter never reads them
    return KDE_OK;
}

extern "C" int kde_jbf_process(kde_jbf* h, const float* depth_dev, const uint8_t* bgr_dev, size_t bgr_step, void* stream)
{
    KDE_REQUIRE(h, "kde_jbf_process: null handle");
    KDE_REQUIRE(bgr_step == (size_t)h->width * 3, "kde_jbf_process: colour image must be continuous (step %zu != 3*width)", bgr_step);
    return kde_jbf_process_batch(h, 1, depth_dev, bgr_dev, nullptr, stream);
}

extern "C" int kde_jbf_presmooth_batch(kde_jbf* h, int n, const uint8_t* bgr_dev, uint8_t* smooth_dev, void* stream)
{
    KDE_REQUIRE(h && bgr_dev, "kde_jbf_presmooth_batch: null argument");
    KDE_ON_DEVICE(h, "kde_jbf_presmooth_batch");
    KDE_REQUIRE(h->p.presmooth, "kde_jbf_presmooth_batch: handle was created with presmooth = 0");
    KDE_REQUIRE(n >= 1 && (smooth_dev || n <= h->max_batch), "kde_jbf_presmooth_batch: bad n");
    return jbf_presmooth(h, n, bgr_dev, smooth_dev ? smooth_dev : h->smooth.p, as_stream(stream));
}

extern "C" int kde_jbf_filter_batch(kde_jbf* h, int n, const float* depth_dev, const uint8_t* guide_bgr_dev,
                                    float* filtered_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev && guide_bgr_dev, "kde_jbf_filter_batch: null argument");
    KDE_ON_DEVICE(h, "kde_jbf_filter_batch");
    KDE_REQUIRE(n >= 1 && n <= 65535 && (filtered_dev || n <= h->max_batch), "kde_jbf_filter_batch: bad n");
    float* out = filtered_dev ? filtered_dev : h->filtered.p;
    KDE_TRY(jbf_filter(h, n, depth_dev, guide_bgr_dev, out, as_stream(stream)));
    if (!filtered_dev) h->n_last = n;
    return KDE_OK;
}

KDE_DEVICE_GETTER(kde_jbf_filtered_device, kde_jbf, float, h->filtered.p)
KDE_DEVICE_GETTER(kde_jbf_smooth_device, kde_jbf, uint8_t, h->smooth.p)

extern "C" int kde_jbf_filtered_host(kde_jbf* h, void* stream, const float** out)
{
    KDE_REQUIRE(h && out, "kde_jbf_filtered_host: null argument");
    // Filtered_Host mirrors the object's own Filtered_Device (JointBilateralFilter.cpp:45-49): n_last <= max_batch
    // frames of it, never a caller-owned output buffer (which may be larger than the pinned buffer, or freed)
    const size_t px = (size_t)h->width * h->height;
    const int frames = h->n_last > 0 ? std::min(h->n_last, h->max_batch) : 1;
    return host_mirror("kde_jbf_filtered_host", h->device, h->filtered.p, px * frames, px * h->max_batch, h->filtered_host,
                       as_stream(stream), out);
}

extern "C" int kde_jbf_spatial_table(kde_jbf* h, float* table_host, int capacity)
{
    KDE_REQUIRE(h && table_host, "kde_jbf_spatial_table: null argument");
    KDE_REQUIRE(capacity >= (int)h->table.size(), "kde_jbf_spatial_table: capacity %d < %zu", capacity, h->table.size());
    memcpy(table_host, h->table.data(), h->table.size() * sizeof(float));
    return KDE_OK;
}

extern "C" int kde_jbf_set_variant(kde_jbf* h, int variant)
{
    KDE_REQUIRE(h, "kde_jbf_set_variant: null handle");
    KDE_REQUIRE(variant >= -1 && variant < jbf_variant_count(), "kde_jbf_set_variant: variant %d out of range", variant);
    h->variant = variant;
    return KDE_OK;
}

extern "C" int kde_jbf_active_variant(kde_jbf* h, int* variant)
{
    KDE_REQUIRE(h && variant, "kde_jbf_active_variant: null argument");
    JbfLaunch a;
    jbf_fill_launch(h, a);
    *variant = jbf_active_variant(a);
    return KDE_OK;
}

extern "C" int kde_jbf_variant_count(void) { return jbf_variant_count(); }
extern "C" const char* kde_jbf_variant_name(int variant) { return jbf_variant_name(variant); }

// -----------------------------------------------------------------------------------------------------
// host-fed JBF (kde_jbf_feed_*): chunks of frames copied in, filtered and copied out on three streams
// -----------------------------------------------------------------------------------------------------
// The streams, the slot ring and the chunk loop are FeedRing's (kde_feed_ring.h); the feed owns the device buffers.
struct JbfFeedSlot {
    DevBuf<float> depth;            // [chunk][H][W] f32: the copied-in depth, or the widened uint16 depth
    DevBuf<uint16_t> depth16;       // [chunk][H][W] landing area of uint16 depth
    DevBuf<uint8_t> bgr;            // [chunk][H][W][3]
    DevBuf<uint8_t> guide;          // [chunk][H][W][3]: K0's output (presmooth = 1 only)
    DevBuf<float> out;              // [chunk][H][W]
    int frames = 0;                 // device capacity in frames
};

struct kde_jbf_feed : FeedRing {
    kde_jbf* jbf = nullptr;
    JbfFeedSlot buf[kFeedSlots];
};

extern "C" int kde_jbf_feed_create(kde_jbf_feed** out, kde_jbf* jbf, int chunk_frames)
{
    KDE_REQUIRE(out, "kde_jbf_feed_create: null out");
    *out = nullptr;
    KDE_REQUIRE(jbf, "kde_jbf_feed_create: null jbf handle");
    KDE_REQUIRE(chunk_frames >= 1 && chunk_frames <= 65535, "kde_jbf_feed_create: chunk_frames=%d outside 1..65535", chunk_frames);
    KDE_ON_DEVICE(jbf, "kde_jbf_feed_create");
    kde_jbf_feed* f = new (std::nothrow) kde_jbf_feed;
    if (!f) return fail(KDE_ERR_NOMEM, "kde_jbf_feed_create: out of host memory");
    f->jbf = jbf;
    const int rc = f->open("kde_jbf_feed_create", jbf->device, chunk_frames);
    if (rc != KDE_OK) {
        delete f;
        return rc;
    }
    *out = f;
    return KDE_OK;
}

extern "C" int kde_jbf_feed_destroy(kde_jbf_feed* f)
{
    delete f;
    return KDE_OK;
}

extern "C" int kde_jbf_feed_last_stats(kde_jbf_feed* f, kde_feed_stats* out)
{
    KDE_REQUIRE(f && out, "kde_jbf_feed_last_stats: null argument");
    *out = f->stats;
    return KDE_OK;
}

extern "C" int kde_jbf_feed_process(kde_jbf_feed* f, int n, const void* depth_host, int depth_format, const uint8_t* bgr_host,
                                    float* filtered_host)
{
    const auto t0 = FeedRing::Clock::now();
    KDE_REQUIRE(f, "kde_jbf_feed_process: null feed");
    KDE_REQUIRE(depth_host && bgr_host && filtered_host, "kde_jbf_feed_process: null host buffer");
    KDE_REQUIRE(n >= 1, "kde_jbf_feed_process: n=%d < 1", n);
    KDE_REQUIRE(depth_format == KDE_DEPTH_F32 || depth_format == KDE_DEPTH_U16, "kde_jbf_feed_process: unknown depth_format %d",
                depth_format);
    KDE_ON_DEVICE(f, "kde_jbf_feed_process");
    kde_jbf* h = f->jbf;
    const size_t px = (size_t)h->width * h->height;
    const bool u16 = depth_format == KDE_DEPTH_U16;
    auto prepare = [&](int k, int cf, FeedSlotDev& dev) -> int {
        JbfFeedSlot& s = f->buf[k];
        if (s.frames < cf) {
            const size_t m = px * cf;
            s.frames = 0;
            KDE_TRY(s.depth.alloc(m));
            KDE_TRY(s.bgr.alloc(m * 3));
            KDE_TRY(s.out.alloc(m));
            s.guide.release();
            s.depth16.release();
            s.frames = cf;
        }
        if (h->p.presmooth && s.guide.n < px * 3 * cf) KDE_TRY(s.guide.alloc(px * 3 * s.frames));
        if (u16 && s.depth16.n < px * cf) KDE_TRY(s.depth16.alloc(px * s.frames));
        KDE_REQUIRE(s.depth.n >= px * cf && s.bgr.n >= px * 3 * cf && s.out.n >= px * cf &&
                        (!h->p.presmooth || s.guide.n >= px * 3 * cf) && (!u16 || s.depth16.n >= px * cf),
                    "kde_jbf_feed_process: internal error: slot %d is smaller than a chunk", k);
        dev.depth = u16 ? static_cast<void*>(s.depth16.p) : static_cast<void*>(s.depth.p);
        dev.bgr = s.bgr.p;
        dev.out = s.out.p;
        return KDE_OK;
    };
    // widen (u16) + K0 + K1 into the slot's own buffers: the handle's smooth / filtered / n_last stay untouched
    auto compute = [&](int k, int fr) -> int {
        JbfFeedSlot& s = f->buf[k];
        if (u16) KDE_TRY(launch_widen_u16(s.depth16.p, s.depth.p, px * fr, f->comp));
        const uint8_t* guide = s.bgr.p;
        if (h->p.presmooth) {
            KDE_TRY(jbf_presmooth(h, fr, s.bgr.p, s.guide.p, f->comp));
            guide = s.guide.p;
        }
        return jbf_filter(h, fr, s.depth.p, guide, s.out.p, f->comp);
    };
    return f->process(t0, px, n, depth_host, u16 ? sizeof(uint16_t) : sizeof(float), bgr_host, filtered_host, sizeof(float), prepare,
                      compute);
}

// =====================================================================================================
// MarkovRandomField
// =====================================================================================================
struct kde_mrf {
    int device = -1;
    int width, height, max_batch, window;
    float color_sigma, smooth_sigma;
    DevBuf<float> filtered;          // Filtered_Device
    PinnedBuf<float> filtered_host;  // Filtered_Host (MarkovRandomField.h:16)
    int n_last = 0;                  // frames of the last call that wrote Filtered_Device
};

extern "C" int kde_mrf_create(kde_mrf** out, int width, int height, int max_batch, int window, float color_sigma, float smooth_sigma)
{
    KDE_REQUIRE(out, "kde_mrf_create: null out");
    *out = nullptr;
    KDE_REQUIRE(width >= 1 && height >= 1 && batch_ok(max_batch), "kde_mrf_create: bad size");
    if (window <= 0) window = 5;                  // MarkovRandomField.cpp:3
    if (color_sigma < 0.0f) color_sigma = 50.0f;  // :5
    if (smooth_sigma < 0.0f) smooth_sigma = 150.0f;  // :6
    KDE_REQUIRE(window <= 31 && (window & 1), "kde_mrf_create: window must be odd <= 31");
    kde_mrf* h = new_handle<kde_mrf>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_mrf_create: out of host memory");
    h->window = window; h->color_sigma = color_sigma; h->smooth_sigma = smooth_sigma;
    int rc = h->filtered.alloc((size_t)width * height * max_batch);
    if (rc != KDE_OK) { delete h; return rc; }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_mrf_destroy(kde_mrf* h) { delete h; return KDE_OK; }

extern "C" int kde_mrf_process_batch(kde_mrf* h, int n, const float* depth_dev, const uint8_t* bgr_dev, float* filtered_dev, void* stream)
{
    KDE_REQUIRE(h && depth_dev && bgr_dev, "kde_mrf_process_batch: null argument");
    KDE_ON_DEVICE(h, "kde_mrf_process_batch");
    KDE_REQUIRE(n >= 1 && n <= 65535 && (filtered_dev || n <= h->max_batch), "kde_mrf_process_batch: bad n");
    MrfLaunch a{h->width, h->height, n, h->window, depth_dev, bgr_dev, filtered_dev ? filtered_dev : h->filtered.p,
                h->color_sigma, h->smooth_sigma};
    KDE_TRY(launch_mrf(a, as_stream(stream)));
    if (!filtered_dev) h->n_last = n;
    return KDE_OK;
}

// float* MarkovRandomField::getFiltered_Host() (MarkovRandomField.h:16; the reference refreshes it after every Process,
// MarkovRandomField.cu:48): here a lazy copy of the object's own Filtered_Device, never of a caller's output buffer
extern "C" int kde_mrf_filtered_host(kde_mrf* h, void* stream, const float** out)
{
    KDE_REQUIRE(h && out, "kde_mrf_filtered_host: null argument");
    const size_t px = (size_t)h->width * h->height;
    const int frames = h->n_last > 0 ? std::min(h->n_last, h->max_batch) : 1;
    return host_mirror("kde_mrf_filtered_host", h->device, h->filtered.p, px * frames, px * h->max_batch, h->filtered_host,
                       as_stream(stream), out);
}

KDE_DEVICE_GETTER(kde_mrf_filtered_device, kde_mrf, float, h->filtered.p)
