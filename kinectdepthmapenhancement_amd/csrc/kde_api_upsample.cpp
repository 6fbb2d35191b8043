// kde_api_upsample.cpp — GuidedDepthUpsampling (kde_upsample_*): a low-resolution depth frame brought to the size of its colour
// image by joint bilateral upsampling, for a batch of frames on the device (upsample_kernels.hip).  No reference counterpart:
// the reference's depth and colour come from a Kinect v1 at one size.
#include "kde_handles.h"

struct kde_upsample {
    int device = -1;                        // -1: created on a host without a device (no buffers; the launch refuses)
    int width = 0, height = 0, max_batch = 1;   // the source (low-resolution) frame
    int out_w = 0, out_h = 0;
    kde_upsample_params p{};
    float sx = 1.0f, sy = 1.0f;
    unsigned groups = 0;                    // workgroups per frame
    DepthStage stage;                       // the last depth_batch; depth [max_batch][out_h][out_w]
    std::vector<float> range_host;          // range[766]
    DevBuf<int> nearest;                    // gx_of[src_w], then gy_of[src_h]
    DevBuf<float> range;                    // [766]
    DevBuf<uint32_t> partial;               // [max_batch][groups]
    DevBuf<uint32_t> filled;                // [max_batch]
    PinnedBuf<uint32_t> filled_host;
};

static const kde_upsample_params kUpsampleDefaults = {2, 30.0f, 0.0f, 0.0f, FLT_MAX};

// gx_of[q] for q = 0 .. count - 1: the output pixel that is low-resolution sample q
static void nearest_of(int count, float scale, int out_count, int* table)
{
    for (int q = 0; q < count; q++) {
        const float g = rintf(((float)q + 0.5f) / scale - 0.5f);
        table[q] = (int)std::min(std::max(g, 0.0f), (float)(out_count - 1));
    }
}

// the widest tap window of any tile along one axis: x0(last) - x0(first) + 2r, with the kernel's own x0
static int widest_window(int out_count, int tile, float scale, int radius)
{
    int widest = 0;
    for (int first = 0; first < out_count; first += tile) {
        const int last = std::min(first + tile - 1, out_count - 1);
        widest = std::max(widest, upsample_floor(last, scale) - upsample_floor(first, scale) + 2 * radius);
    }
    return widest;
}

// radius 2, sigma_color 30 (K0's constant, the same squared-L1 form), no guard, every finite positive depth
extern "C" int kde_upsample_default_params(kde_upsample_params* p)
{
    KDE_REQUIRE(p, "kde_upsample_default_params: null argument");
    *p = kUpsampleDefaults;
    return KDE_OK;
}

extern "C" int kde_upsample_create(kde_upsample** out, int src_w, int src_h, int out_w, int out_h, int max_batch, const kde_upsample_params* p)
{
    const char* who = "kde_upsample_create";
    KDE_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    KDE_TRY(check_frame_batch(who, src_w, src_h, max_batch));
    KDE_REQUIRE(frame_ok(out_w, out_h), "%s: bad size", who);
    KDE_REQUIRE(src_w <= kRegMaxSide && src_h <= kRegMaxSide && out_w <= kRegMaxSide && out_h <= kRegMaxSide,
                "%s: a side above %d is not an exact float", who, kRegMaxSide);
    KDE_REQUIRE(out_w >= src_w && out_h >= src_h, "%s: the output %d x %d is smaller than the source %d x %d (this is an upsampler)", who,
                out_w, out_h, src_w, src_h);
    const kde_upsample_params q = p ? *p : kUpsampleDefaults;
    KDE_REQUIRE(q.radius >= 1 && q.radius <= kUpsampleMaxRadius, "%s: radius=%d outside 1..%d", who, q.radius, kUpsampleMaxRadius);
    KDE_TRY(check_sigma(who, "sigma_color", q.sigma_color));
    KDE_TRY(check_max_gap(who, q.max_gap));
    KDE_TRY(check_z_range(who, q.z_min, q.z_max));
    const float sx = (float)src_w / (float)out_w, sy = (float)src_h / (float)out_h;
    // never met (upsample_kernels.hip derives 42 x 18 for any sizes this far): the kernel's LDS arrays rest on it
    KDE_REQUIRE(widest_window(out_w, kUpsampleTileW, sx, q.radius) <= kUpsampleWinW && widest_window(out_h, kUpsampleTileH, sy, q.radius) <= kUpsampleWinH,
                "%s: a tile's tap window exceeds %d x %d", who, kUpsampleWinW, kUpsampleWinH);
    kde_upsample* h = new_handle<kde_upsample>(src_w, src_h, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    h->out_w = out_w;
    h->out_h = out_h;
    h->p = q;
    h->sx = sx;
    h->sy = sy;
    h->groups = upsample_groups(out_w, out_h);
    std::vector<int> nearest;
    try {
        h->range_host.resize(kColourRange);
        nearest.resize((size_t)src_w + src_h);
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    }
    colour_range_table(q.sigma_color, h->range_host.data());
    nearest_of(src_w, sx, out_w, nearest.data());
    nearest_of(src_h, sy, out_h, nearest.data() + src_w);
    if (h->device >= 0) {
        int rc = h->filled.alloc((size_t)max_batch);
        if (rc == KDE_OK) rc = h->partial.alloc((size_t)max_batch * h->groups);
        if (rc == KDE_OK) rc = h->stage.depth.alloc((size_t)max_batch * out_w * out_h);
        if (rc == KDE_OK) rc = h->range.alloc((size_t)kColourRange);
        if (rc == KDE_OK) rc = h->nearest.alloc(nearest.size());
        if (rc == KDE_OK && hipMemcpy(h->range.p, h->range_host.data(), kColourRange * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(KDE_ERR_HIP, "%s: the range table could not be copied to the device", who);
        if (rc == KDE_OK && hipMemcpy(h->nearest.p, nearest.data(), nearest.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(KDE_ERR_HIP, "%s: the nearest-pixel tables could not be copied to the device", who);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_upsample_destroy(kde_upsample* h)
{
    delete h;
    return KDE_OK;
}

extern "C" int kde_upsample_range_table(kde_upsample* h, float* table_host, int capacity)
{
    return copy_range_table("kde_upsample_range_table", h ? &h->range_host : nullptr, table_host, capacity);
}

extern "C" int kde_upsample_depth_batch(kde_upsample* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev, int bgr_frames,
                                        int out_format, void* out_dev, void* stream)
{
    const char* who = "kde_upsample_depth_batch";
    KDE_REQUIRE(h && depth_dev && bgr_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_bgr_frames(who, bgr_frames, n));
    KDE_TRY(check_depth_in(who, depth_dev, depth_format));
    KDE_TRY(check_depth_out(who, out_dev, out_format));
    KDE_TRY(check_has_device(who, h->device));
    UpsampleLaunch a{};
    a.n = n;
    a.sw = h->width;
    a.sh = h->height;
    a.ow = h->out_w;
    a.oh = h->out_h;
    a.radius = h->p.radius;
    a.sx = h->sx;
    a.sy = h->sy;
    a.max_gap = h->p.max_gap;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    a.depth = depth_dev;
    a.depth_format = depth_format;
    a.bgr = bgr_dev;
    a.bgr_frames = bgr_frames;
    a.out = h->stage.written(out_dev);
    a.out_format = out_format;
    a.gx_of = h->nearest.p;
    a.gy_of = h->nearest.p + h->width;
    a.range = h->range.p;
    a.partial = h->partial.p;
    a.filled = h->filled.p;
    KDE_TRY(launch_upsample(a, as_stream(stream)));
    h->stage.finished(n, out_format, a.out);
    return KDE_OK;
}

KDE_STAGE_DEPTH_GETTERS(kde_upsample_depth_device, kde_upsample_depth_host, kde_upsample, "kde_upsample_depth_batch", (size_t)h->out_w * h->out_h)
KDE_STAGE_COUNT_GETTERS(kde_upsample_filled_device, kde_upsample_filled_host, kde_upsample, "kde_upsample_depth_batch", h->filled.p, h->filled_host)
