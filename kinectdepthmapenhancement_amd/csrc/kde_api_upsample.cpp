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
    int n_last = 0;                         // frames of the last depth_batch (0: none yet)
    int format_last = KDE_DEPTH_F32;        // its out_format
    void* out_last = nullptr;               // where it wrote: depth or the caller's buffer
    std::vector<float> range_host;          // range[766]
    DevBuf<int> nearest;                    // gx_of[src_w], then gy_of[src_h]
    DevBuf<float> range;                    // [766]
    DevBuf<uint32_t> partial;               // [max_batch][groups]
    DevBuf<uint32_t> filled;                // [max_batch]
    DevBuf<float> depth;                    // [max_batch][out_h][out_w]: floats, or uint16 in the same bytes
    PinnedBuf<uint32_t> filled_host;
    PinnedBuf<float> depth_host;
};

static const kde_upsample_params kUpsampleDefaults = {2, 30.0f, 0.0f, 0.0f, FLT_MAX};

static bool depth_format_ok(int f) { return f == KDE_DEPTH_F32 || f == KDE_DEPTH_U16; }
static size_t depth_element(int f) { return f == KDE_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float); }

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
    KDE_REQUIRE(std::isfinite(q.sigma_color) && q.sigma_color > 0.0f, "%s: sigma_color=%g must be finite and > 0", who, (double)q.sigma_color);
    KDE_REQUIRE(std::isfinite(q.max_gap) && q.max_gap >= 0.0f, "%s: max_gap=%g must be finite and >= 0 (0: no guard)", who, (double)q.max_gap);
    KDE_REQUIRE(std::isfinite(q.z_min) && q.z_min >= 0.0f, "%s: z_min=%g must be finite and >= 0", who, (double)q.z_min);
    KDE_REQUIRE(q.z_min < q.z_max, "%s: z_min=%g must be below z_max=%g", who, (double)q.z_min, (double)q.z_max);
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
        h->range_host.resize(kUpsampleRange);
        nearest.resize((size_t)src_w + src_h);
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    }
    for (int k = 0; k < kUpsampleRange; k++)
        h->range_host[k] = (float)std::exp(-(double)(k * k) / (2.0 * (double)q.sigma_color * (double)q.sigma_color));
    nearest_of(src_w, sx, out_w, nearest.data());
    nearest_of(src_h, sy, out_h, nearest.data() + src_w);
    if (h->device >= 0) {
        int rc = h->filled.alloc((size_t)max_batch);
        if (rc == KDE_OK) rc = h->partial.alloc((size_t)max_batch * h->groups);
        if (rc == KDE_OK) rc = h->depth.alloc((size_t)max_batch * out_w * out_h);
        if (rc == KDE_OK) rc = h->range.alloc((size_t)kUpsampleRange);
        if (rc == KDE_OK) rc = h->nearest.alloc(nearest.size());
        if (rc == KDE_OK && hipMemcpy(h->range.p, h->range_host.data(), kUpsampleRange * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
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
    const char* who = "kde_upsample_range_table";
    KDE_REQUIRE(h && table_host, "%s: null argument", who);
    KDE_REQUIRE(capacity >= kUpsampleRange, "%s: capacity=%d is below the %d entries of the table", who, capacity, kUpsampleRange);
    std::memcpy(table_host, h->range_host.data(), kUpsampleRange * sizeof(float));
    return KDE_OK;
}

extern "C" int kde_upsample_depth_batch(kde_upsample* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev, int bgr_frames,
                                        int out_format, void* out_dev, void* stream)
{
    const char* who = "kde_upsample_depth_batch";
    KDE_REQUIRE(h && depth_dev && bgr_dev, "%s: null argument", who);
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "%s: n=%d outside 1..max_batch=%d", who, n, h->max_batch);
    KDE_REQUIRE(bgr_frames == 1 || bgr_frames == n, "%s: bgr_frames=%d is neither 1 nor n=%d", who, bgr_frames, n);
    KDE_REQUIRE(depth_format_ok(depth_format), "%s: the unknown depth format %d", who, depth_format);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(depth_dev) % depth_element(depth_format) == 0, "%s: depth_dev is not %d-byte aligned", who,
                (int)depth_element(depth_format));
    KDE_REQUIRE(depth_format_ok(out_format), "%s: the unknown output format %d", who, out_format);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(out_dev) % depth_element(out_format) == 0, "%s: out_dev is not %d-byte aligned", who,
                (int)depth_element(out_format));
    KDE_ON_DEVICE(h, who);
    if (h->device < 0) return fail(KDE_ERR_HIP, "%s: the handle was created on a host without a device", who);
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
    a.out = out_dev ? out_dev : h->depth.p;
    a.out_format = out_format;
    a.gx_of = h->nearest.p;
    a.gy_of = h->nearest.p + h->width;
    a.range = h->range.p;
    a.partial = h->partial.p;
    a.filled = h->filled.p;
    KDE_TRY(launch_upsample(a, as_stream(stream)));
    h->n_last = n;
    h->format_last = out_format;
    h->out_last = a.out;
    return KDE_OK;
}

extern "C" int kde_upsample_depth_device(kde_upsample* h, void** out)
{
    KDE_REQUIRE(h && out, "kde_upsample_depth_device: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_upsample_depth_device: kde_upsample_depth_batch was not called");
    *out = h->out_last;
    return KDE_OK;
}

extern "C" int kde_upsample_depth_host(kde_upsample* h, void* stream, const void** out)
{
    const char* who = "kde_upsample_depth_host";
    KDE_REQUIRE(h && out, "%s: null argument", who);
    KDE_REQUIRE(h->n_last > 0, "%s: kde_upsample_depth_batch was not called", who);
    KDE_ON_DEVICE(h, who);
    const size_t px = (size_t)h->out_w * h->out_h;
    KDE_TRY(h->depth_host.ensure((size_t)h->max_batch * px));
    hipStream_t s = as_stream(stream);
    KDE_HIP_TRY(hipMemcpyAsync(h->depth_host.p, h->out_last, (size_t)h->n_last * px * depth_element(h->format_last), hipMemcpyDeviceToHost, s));
    KDE_HIP_TRY(hipStreamSynchronize(s));
    *out = h->depth_host.p;
    return KDE_OK;
}

extern "C" int kde_upsample_filled_device(kde_upsample* h, uint32_t** out)
{
    KDE_REQUIRE(h && out, "kde_upsample_filled_device: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_upsample_filled_device: kde_upsample_depth_batch was not called");
    *out = h->filled.p;
    return KDE_OK;
}

extern "C" int kde_upsample_filled_host(kde_upsample* h, void* stream, const uint32_t** out)
{
    KDE_REQUIRE(h && out, "kde_upsample_filled_host: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_upsample_filled_host: kde_upsample_depth_batch was not called");
    return host_mirror("kde_upsample_filled_host", h->device, h->filled.p, (size_t)h->n_last, (size_t)h->max_batch, h->filled_host,
                       as_stream(stream), out);
}
