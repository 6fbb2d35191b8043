// kde_api_speckle.cpp — DepthSpeckleFilter (kde_speckle_*): the connected components of a depth frame under a depth-difference
// link, and the frame without those smaller than min_size, for a batch of frames on the device (speckle_kernels.hip).  No
// reference counterpart: the complement of DepthHoleFilling -- invalidate first, then fill.
#include "kde_handles.h"

struct kde_speckle {
    int device = -1;                        // -1: created on a host without a device (no buffers; the launch refuses)
    int width = 0, height = 0, max_batch = 1;
    kde_speckle_params p{};
    unsigned groups = 0;                    // workgroups per frame
    DepthStage stage;                       // the last filter_batch; depth [max_batch][H][W]
    DevBuf<int32_t> parent;                 // [max_batch][H][W]
    DevBuf<uint32_t> size;                  // [max_batch][H][W]
    DevBuf<uint32_t> partial;               // [max_batch][groups][3]
    DevBuf<uint32_t> counts;                // removed[max_batch], components[max_batch], capped[max_batch]
    PinnedBuf<uint32_t> removed_host, components_host, capped_host;
};

static const kde_speckle_params kSpeckleDefaults = {64, 10.0f, 0.02f, 4, 0.0f, FLT_MAX};

// components below 64 pixels go; a link holds within 10 mm + 2 % of the nearer depth; 4-connected; every finite positive depth
extern "C" int kde_speckle_default_params(kde_speckle_params* p)
{
    KDE_REQUIRE(p, "kde_speckle_default_params: null argument");
    *p = kSpeckleDefaults;
    return KDE_OK;
}

static int check_diff(const char* who, const char* name, float v)
{
    KDE_REQUIRE(std::isfinite(v) && v >= 0.0f, "%s: %s=%g must be finite and >= 0", who, name, (double)v);
    return KDE_OK;
}

extern "C" int kde_speckle_create(kde_speckle** out, int width, int height, int max_batch, const kde_speckle_params* p)
{
    const char* who = "kde_speckle_create";
    KDE_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    KDE_TRY(check_frame_batch(who, width, height, max_batch));
    KDE_REQUIRE(width <= kRegMaxSide && height <= kRegMaxSide, "%s: a side above %d", who, kRegMaxSide);
    const kde_speckle_params q = p ? *p : kSpeckleDefaults;
    KDE_REQUIRE(q.min_size >= 1 && q.min_size <= kSpeckleMaxSize, "%s: min_size=%d outside 1..%d", who, q.min_size, kSpeckleMaxSize);
    KDE_TRY(check_diff(who, "max_diff", q.max_diff));
    KDE_TRY(check_diff(who, "rel_diff", q.rel_diff));
    KDE_REQUIRE(q.connectivity == 4 || q.connectivity == 8, "%s: connectivity=%d is neither 4 nor 8", who, q.connectivity);
    KDE_TRY(check_z_range(who, q.z_min, q.z_max));
    kde_speckle* h = new_handle<kde_speckle>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    h->p = q;
    h->groups = speckle_groups(width, height);
    if (h->device >= 0) {
        const size_t px = (size_t)max_batch * width * height;
        int rc = h->counts.alloc((size_t)max_batch * 3);
        if (rc == KDE_OK) rc = h->partial.alloc((size_t)max_batch * h->groups * 3);
        if (rc == KDE_OK) rc = h->stage.depth.alloc(px);
        if (rc == KDE_OK) rc = h->parent.alloc(px);
        if (rc == KDE_OK) rc = h->size.alloc(px);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_speckle_destroy(kde_speckle* h)
{
    delete h;
    return KDE_OK;
}

static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return !(a0 + a_bytes <= b0 || b0 + b_bytes <= a0);
}

extern "C" int kde_speckle_filter_batch(kde_speckle* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev,
                                        int32_t* labels_dev, void* stream)
{
    const char* who = "kde_speckle_filter_batch";
    KDE_REQUIRE(h && depth_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_depth_in(who, depth_dev, depth_format));
    KDE_TRY(check_depth_out(who, out_dev, out_format));
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(labels_dev) % sizeof(int32_t) == 0, "%s: labels_dev is not 4-byte aligned", who);
    // The apply step reads a pixel and then writes it, and every step before it only reads the input: exactly in place is
    // safe.  Any other overlap lets one thread write what another has yet to read.
    const size_t px = (size_t)n * h->width * h->height;
    const size_t in_bytes = px * depth_element(depth_format), out_bytes = px * depth_element(out_format);
    void* const w = h->stage.written(out_dev);
    if (w && !(out_dev == depth_dev && out_format == depth_format))
        KDE_REQUIRE(!overlap(w, out_bytes, depth_dev, in_bytes),
                    "%s: %s overlaps depth_dev (in place is supported only with out_dev == depth_dev and out_format == depth_format)", who,
                    out_dev ? "out_dev" : "the object-owned output buffer, which out_dev == NULL selects,");
    if (labels_dev) {
        KDE_REQUIRE(!overlap(labels_dev, px * sizeof(int32_t), depth_dev, in_bytes), "%s: labels_dev overlaps depth_dev", who);
        KDE_REQUIRE(!w || !overlap(labels_dev, px * sizeof(int32_t), w, out_bytes), "%s: labels_dev overlaps %s", who,
                    out_dev ? "out_dev" : "the object-owned output buffer, which out_dev == NULL selects");
    }
    KDE_TRY(check_has_device(who, h->device));
    SpeckleLaunch a{};
    a.n = n;
    a.w = h->width;
    a.h = h->height;
    a.min_size = h->p.min_size;
    a.connectivity = h->p.connectivity;
    a.max_diff = h->p.max_diff;
    a.rel_diff = h->p.rel_diff;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    a.depth = depth_dev;
    a.depth_format = depth_format;
    a.out = w;
    a.out_format = out_format;
    a.labels = labels_dev;
    a.parent = h->parent.p;
    a.size = h->size.p;
    a.partial = h->partial.p;
    a.removed = h->counts.p;
    a.components = h->counts.p + h->max_batch;
    a.capped = h->counts.p + 2 * (size_t)h->max_batch;
    KDE_TRY(launch_speckle(a, as_stream(stream)));
    h->stage.finished(n, out_format, a.out);
    return KDE_OK;
}

KDE_STAGE_DEPTH_GETTERS(kde_speckle_depth_device, kde_speckle_depth_host, kde_speckle, "kde_speckle_filter_batch", (size_t)h->width * h->height)
KDE_STAGE_COUNT_GETTERS(kde_speckle_removed_device, kde_speckle_removed_host, kde_speckle, "kde_speckle_filter_batch", h->counts.p, h->removed_host)
KDE_STAGE_COUNT_GETTERS(kde_speckle_components_device, kde_speckle_components_host, kde_speckle, "kde_speckle_filter_batch",
                        h->counts.p + h->max_batch, h->components_host)
KDE_STAGE_COUNT_GETTERS(kde_speckle_capped_device, kde_speckle_capped_host, kde_speckle, "kde_speckle_filter_batch",
                        h->counts.p + 2 * (size_t)h->max_batch, h->capped_host)
