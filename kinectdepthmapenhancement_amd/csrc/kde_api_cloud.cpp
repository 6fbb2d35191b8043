// kde_api_cloud.cpp — PointCloudXYZRGB (kde_cloud_*): the output step of the reference, main.cpp:211-300, for a batch of
// frames on the device (cloud_kernels.hip): XYZRGB records, compacted in raster order or organised.
#include "kde_handles.h"

static_assert(sizeof(kde_cloud_point) == 16, "kde_cloud_point is a 16-byte record");

struct kde_cloud {
    int device = -1;                        // -1: created on a host without a device (no buffers; build_batch refuses)
    int width = 0, height = 0, max_batch = 1;
    kde_cloud_params p{};
    Camera cam{};                           // width, height from create; the rest from set_camera
    bool cam_set = false;
    int n_last = 0;                         // frames of the last build_batch (0: none yet)
    kde_cloud_point* out_last = nullptr;    // where the last build_batch wrote: points or the caller's buffer
    DevBuf<uint32_t> seg;                   // [max_batch][segments]
    DevBuf<uint32_t> counts;                // [max_batch]
    DevBuf<kde_cloud_point> points;         // [max_batch][H][W]
    PinnedBuf<uint32_t> counts_host;
    PinnedBuf<kde_cloud_point> points_host;
    std::vector<uint64_t> offsets;          // [n_last + 1] of the last points_host
};

static const kde_cloud_params kCloudDefaults = {50.0f, 15000.0f, 1000.0f, 1, 0};   // main.cpp:227-230

// main.cpp:211-300: its literals
extern "C" int kde_cloud_default_params(kde_cloud_params* p)
{
    KDE_REQUIRE(p, "kde_cloud_default_params: null argument");
    *p = kCloudDefaults;
    return KDE_OK;
}

// main.cpp:211-300: the clouds of main.cpp:211-216
extern "C" int kde_cloud_create(kde_cloud** out, int width, int height, int max_batch, const kde_cloud_params* p)
{
    KDE_REQUIRE(out, "kde_cloud_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_cloud_create", width, height, max_batch));
    const kde_cloud_params q = p ? *p : kCloudDefaults;
    KDE_REQUIRE(std::isfinite(q.z_min) && std::isfinite(q.z_max) && q.z_min < q.z_max,
                "kde_cloud_create: z_min=%g, z_max=%g must be finite with z_min < z_max", (double)q.z_min, (double)q.z_max);
    KDE_REQUIRE(std::isfinite(q.divisor) && q.divisor > 0.0f, "kde_cloud_create: divisor=%g must be finite and > 0", (double)q.divisor);
    kde_cloud* h = new_handle<kde_cloud>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_cloud_create: out of host memory");
    h->p = q;
    h->p.negate_z = q.negate_z != 0;
    h->p.organized = q.organized != 0;
    h->cam.width = width;
    h->cam.height = height;
    if (h->device >= 0) {
        const size_t px = (size_t)width * height;
        int rc = h->seg.alloc((size_t)max_batch * cloud_segments(px));
        if (rc == KDE_OK) rc = h->counts.alloc((size_t)max_batch);
        if (rc == KDE_OK) rc = h->points.alloc((size_t)max_batch * px);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

// main.cpp:211-300 holds its clouds in shared pointers
extern "C" int kde_cloud_destroy(kde_cloud* h)
{
    delete h;
    return KDE_OK;
}

// main.cpp:211-300 reads clouds made by convertor.projectiveToReal (main.cpp:168): the camera of DimensionConvertor.cpp:3-13
extern "C" int kde_cloud_set_camera(kde_cloud* h, const double* K9)
{
    KDE_REQUIRE(h && K9, "kde_cloud_set_camera: null argument");
    h->cam.fx = (float)K9[0];
    h->cam.fy = (float)K9[4];
    h->cam.cx = (int)K9[2];
    h->cam.cy = (int)K9[5];
    h->cam_set = true;
    return KDE_OK;
}

// main.cpp:211-300: the loop over the pixels for one method, n frames at once
extern "C" int kde_cloud_build_batch(kde_cloud* h, int n, const kde_error3d_source* src, const uint8_t* bgr_dev, int bgr_frames,
                                     kde_cloud_point* out_dev, void* stream)
{
    const char* who = "kde_cloud_build_batch";
    KDE_REQUIRE(h && src && bgr_dev, "%s: null argument", who);
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "%s: n=%d outside 1..max_batch=%d", who, n, h->max_batch);
    KDE_REQUIRE(bgr_frames == 1 || bgr_frames == n, "%s: bgr_frames=%d is neither 1 nor n=%d", who, bgr_frames, n);
    KDE_REQUIRE(src->format == KDE_SRC_POINTS_F32 || src->format == KDE_SRC_DEPTH_F32 || src->format == KDE_SRC_DEPTH_U16,
                "%s: the source has the unknown format %d", who, src->format);
    KDE_REQUIRE(src->data_dev, "%s: the source has a null data_dev", who);
    const uintptr_t align = src->format == KDE_SRC_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(src->data_dev) % align == 0, "%s: the source is not %d-byte aligned", who, (int)align);
    KDE_REQUIRE(src->format == KDE_SRC_POINTS_F32 || h->cam_set, "%s: the source is a depth map but kde_cloud_set_camera was not called", who);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(out_dev) % 16 == 0, "%s: out_dev is not 16-byte aligned", who);
    KDE_ON_DEVICE(h, who);
    if (h->device < 0) return fail(KDE_ERR_HIP, "%s: the handle was created on a host without a device", who);
    CloudLaunch a{};
    a.n = n;
    a.src = src->data_dev;
    a.format = src->format;
    a.bgr = bgr_dev;
    a.bgr_frames = bgr_frames;
    a.cam = h->cam;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    a.divisor = h->p.divisor;
    a.negate_z = h->p.negate_z;
    a.organized = h->p.organized;
    a.seg = h->seg.p;
    a.counts = h->counts.p;
    a.out = out_dev ? out_dev : h->points.p;
    KDE_TRY(launch_cloud(a, as_stream(stream)));
    h->n_last = n;
    h->out_last = a.out;
    return KDE_OK;
}

// main.cpp:211-300: input .. result, the records of the last call
extern "C" int kde_cloud_points_device(kde_cloud* h, kde_cloud_point** out)
{
    KDE_REQUIRE(h && out, "kde_cloud_points_device: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_cloud_points_device: kde_cloud_build_batch was not called");
    *out = h->out_last;
    return KDE_OK;
}

// main.cpp:211-300: the sizes of its clouds
extern "C" int kde_cloud_counts_device(kde_cloud* h, uint32_t** out)
{
    KDE_REQUIRE(h && out, "kde_cloud_counts_device: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_cloud_counts_device: kde_cloud_build_batch was not called");
    *out = h->counts.p;
    return KDE_OK;
}

// main.cpp:211-300 builds its clouds on the host: the counts in pinned memory, ready when the call returns
extern "C" int kde_cloud_counts_host(kde_cloud* h, void* stream, const uint32_t** out)
{
    KDE_REQUIRE(h && out, "kde_cloud_counts_host: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_cloud_counts_host: kde_cloud_build_batch was not called");
    return host_mirror("kde_cloud_counts_host", h->device, h->counts.p, (size_t)h->n_last, (size_t)h->max_batch, h->counts_host,
                       as_stream(stream), out);
}

// main.cpp:211-300 builds its clouds on the host: the frames back to back in pinned memory
extern "C" int kde_cloud_points_host(kde_cloud* h, void* stream, const kde_cloud_point** out, const uint64_t** offsets)
{
    const char* who = "kde_cloud_points_host";
    KDE_REQUIRE(h && out && offsets, "%s: null argument", who);
    KDE_REQUIRE(h->n_last > 0, "%s: kde_cloud_build_batch was not called", who);
    const uint32_t* counts = nullptr;
    KDE_TRY(host_mirror(who, h->device, h->counts.p, (size_t)h->n_last, (size_t)h->max_batch, h->counts_host, as_stream(stream), &counts));
    const size_t px = (size_t)h->width * h->height;
    const int n = h->n_last;
    try {
        h->offsets.assign((size_t)n + 1, 0);
    } catch (const std::bad_alloc&) {
        return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    }
    for (int f = 0; f < n; f++) {
        KDE_REQUIRE(counts[f] <= px, "%s: count[%d]=%u exceeds the frame", who, f, counts[f]);
        h->offsets[f + 1] = h->offsets[f] + (h->p.organized ? px : (size_t)counts[f]);
    }
    const size_t total = h->offsets[n];
    KDE_TRY(h->points_host.ensure(total ? total : 1));
    hipStream_t s = as_stream(stream);
    if (h->p.organized) {
        KDE_HIP_TRY(hipMemcpyAsync(h->points_host.p, h->out_last, total * sizeof(kde_cloud_point), hipMemcpyDeviceToHost, s));
    } else {
        for (int f = 0; f < n; f++) {
            if (counts[f] == 0) continue;
            KDE_HIP_TRY(hipMemcpyAsync(h->points_host.p + h->offsets[f], h->out_last + (size_t)f * px,
                                       (size_t)counts[f] * sizeof(kde_cloud_point), hipMemcpyDeviceToHost, s));
        }
    }
    KDE_HIP_TRY(hipStreamSynchronize(s));
    *out = h->points_host.p;
    *offsets = h->offsets.data();
    return KDE_OK;
}
