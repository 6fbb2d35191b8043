// kde_api_holefill.cpp — DepthHoleFilling (kde_holefill_*): the holes of a depth frame filled from their valid neighbours under
// the guide of its colour image, for a batch of frames on the device (holefill_kernels.hip).  No reference counterpart: the
// reference's TOFDepthInterpolation ends in a projection whose optimisation is commented out.
#include "kde_handles.h"

struct kde_holefill {
    int device = -1;                        // -1: created on a host without a device (no buffers; the launch refuses)
    int width = 0, height = 0, max_batch = 1;
    kde_holefill_params p{};
    int fuse = 1;                           // passes per launch: p.passes_per_launch, or the library's choice for the radius
    unsigned groups = 0;                    // workgroups per frame
    DepthStage stage;                       // the last fill_batch; depth [max_batch][H][W]
    std::vector<float> space_host;          // space[(2r + 1)^2]
    std::vector<float> range_host;          // range[766]
    DevBuf<float> space, range;
    DevBuf<float> state[2];                 // [max_batch][H][W] each: the state between two launches
    DevBuf<uint8_t> pass;                   // [max_batch][H][W]: pass_of of a call without pass_of_dev
    DevBuf<uint32_t> partial;               // [max_batch][groups][2]
    DevBuf<uint32_t> counts;                // filled[max_batch], then remaining[max_batch]
    PinnedBuf<uint32_t> filled_host, remaining_host;
};

static const kde_holefill_params kHolefillDefaults = {2, 8, 3, 2.0f, 30.0f, 0.0f, 0, 0.0f, FLT_MAX, 0};
// the library's passes per launch for radius 1, 2, 3: measured on the MI355X ("Depth hole filling").  At radius 3
// with the guard fusing did not beat one pass per launch on any frame set: the choice there is 1.
static const int kHolefillFuse[kHolefillMaxRadius + 1] = {0, 4, 2, 2};

// radius 2, 8 passes, 3 taps, sigma_space 2, sigma_color 30 (K0's constant, the same squared-L1 form), no guard, every finite
// positive depth, the library's passes per launch
extern "C" int kde_holefill_default_params(kde_holefill_params* p)
{
    KDE_REQUIRE(p, "kde_holefill_default_params: null argument");
    *p = kHolefillDefaults;
    return KDE_OK;
}

extern "C" int kde_holefill_create(kde_holefill** out, int width, int height, int max_batch, const kde_holefill_params* p)
{
    const char* who = "kde_holefill_create";
    KDE_REQUIRE(out, "%s: null out", who);
    *out = nullptr;
    KDE_TRY(check_frame_batch(who, width, height, max_batch));
    KDE_REQUIRE(width <= kRegMaxSide && height <= kRegMaxSide, "%s: a side above %d", who, kRegMaxSide);
    const kde_holefill_params q = p ? *p : kHolefillDefaults;
    KDE_REQUIRE(q.radius >= 1 && q.radius <= kHolefillMaxRadius, "%s: radius=%d outside 1..%d", who, q.radius, kHolefillMaxRadius);
    KDE_REQUIRE(q.iterations >= 1 && q.iterations <= kHolefillMaxIterations, "%s: iterations=%d outside 1..%d", who, q.iterations,
                kHolefillMaxIterations);
    const int side = 2 * q.radius + 1, taps = side * side - 1;
    KDE_REQUIRE(q.min_taps >= 1 && q.min_taps <= taps, "%s: min_taps=%d outside 1..%d (radius %d)", who, q.min_taps, taps, q.radius);
    KDE_TRY(check_sigma(who, "sigma_space", q.sigma_space));
    KDE_TRY(check_sigma(who, "sigma_color", q.sigma_color));
    KDE_TRY(check_max_gap(who, q.max_gap));
    KDE_REQUIRE(q.gap_rule == 0 || q.gap_rule == 1, "%s: gap_rule=%d is neither 0 (heaviest) nor 1 (farthest)", who, q.gap_rule);
    KDE_TRY(check_z_range(who, q.z_min, q.z_max));
    KDE_REQUIRE(q.passes_per_launch >= 0 && q.passes_per_launch <= kHolefillMaxFuse, "%s: passes_per_launch=%d outside 0..%d", who,
                q.passes_per_launch, kHolefillMaxFuse);
    kde_holefill* h = new_handle<kde_holefill>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    h->p = q;
    h->fuse = q.passes_per_launch ? q.passes_per_launch : (q.radius == 3 && q.max_gap > 0.0f) ? 1 : kHolefillFuse[q.radius];
    h->groups = holefill_groups(width, height);
    try {
        h->space_host.resize((size_t)side * side);
        h->range_host.resize(kColourRange);
    } catch (const std::bad_alloc&) {
        delete h;
        return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    }
    for (int dy = -q.radius; dy <= q.radius; dy++)
        for (int dx = -q.radius; dx <= q.radius; dx++)
            h->space_host[(size_t)(dy + q.radius) * side + dx + q.radius] =
                (float)std::exp(-(double)(dx * dx + dy * dy) / (2.0 * (double)q.sigma_space * (double)q.sigma_space));
    colour_range_table(q.sigma_color, h->range_host.data());
    if (h->device >= 0) {
        const size_t px = (size_t)max_batch * width * height;
        const bool states = q.iterations > h->fuse;         // more than one launch
        int rc = h->counts.alloc((size_t)max_batch * 2);
        if (rc == KDE_OK) rc = h->partial.alloc((size_t)max_batch * h->groups * 2);
        if (rc == KDE_OK) rc = h->stage.depth.alloc(px);
        if (rc == KDE_OK) rc = h->pass.alloc(px);
        if (rc == KDE_OK && states) rc = h->state[0].alloc(px);
        if (rc == KDE_OK && q.iterations > 2 * h->fuse) rc = h->state[1].alloc(px);
        if (rc == KDE_OK) rc = h->space.alloc(h->space_host.size());
        if (rc == KDE_OK) rc = h->range.alloc((size_t)kColourRange);
        if (rc == KDE_OK && hipMemcpy(h->space.p, h->space_host.data(), h->space_host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(KDE_ERR_HIP, "%s: the space table could not be copied to the device", who);
        if (rc == KDE_OK && hipMemcpy(h->range.p, h->range_host.data(), kColourRange * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            rc = fail(KDE_ERR_HIP, "%s: the range table could not be copied to the device", who);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

extern "C" int kde_holefill_destroy(kde_holefill* h)
{
    delete h;
    return KDE_OK;
}

extern "C" int kde_holefill_space_table(kde_holefill* h, float* table_host, int capacity)
{
    const char* who = "kde_holefill_space_table";
    KDE_REQUIRE(h && table_host, "%s: null argument", who);
    const int count = (int)h->space_host.size();
    KDE_REQUIRE(capacity >= count, "%s: capacity=%d is below the %d entries of the table", who, capacity, count);
    std::memcpy(table_host, h->space_host.data(), (size_t)count * sizeof(float));
    return KDE_OK;
}

extern "C" int kde_holefill_range_table(kde_holefill* h, float* table_host, int capacity)
{
    return copy_range_table("kde_holefill_range_table", h ? &h->range_host : nullptr, table_host, capacity);
}

extern "C" int kde_holefill_passes_per_launch(kde_holefill* h, int* out)
{
    KDE_REQUIRE(h && out, "kde_holefill_passes_per_launch: null argument");
    *out = h->fuse;
    return KDE_OK;
}

extern "C" int kde_holefill_fill_batch(kde_holefill* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev, int bgr_frames,
                                       int out_format, void* out_dev, uint8_t* pass_of_dev, void* stream)
{
    const char* who = "kde_holefill_fill_batch";
    KDE_REQUIRE(h && depth_dev && bgr_dev, "%s: null argument", who);
    KDE_TRY(check_batch_n(who, n, h->max_batch));
    KDE_TRY(check_bgr_frames(who, bgr_frames, n));
    KDE_TRY(check_depth_in(who, depth_dev, depth_format));
    KDE_TRY(check_depth_out(who, out_dev, out_format));
    // a workgroup reads the halo of its tile while its neighbours write theirs
    KDE_TRY(h->stage.check_not_in_place(who, depth_dev, depth_format, out_dev, out_format, (size_t)n * h->width * h->height));
    KDE_TRY(check_has_device(who, h->device));
    HolefillLaunch a{};
    a.n = n;
    a.w = h->width;
    a.h = h->height;
    a.radius = h->p.radius;
    a.iterations = h->p.iterations;
    a.fuse = h->fuse;
    a.min_taps = h->p.min_taps;
    a.gap_rule = h->p.gap_rule;
    a.max_gap = h->p.max_gap;
    a.z_min = h->p.z_min;
    a.z_max = h->p.z_max;
    a.depth = depth_dev;
    a.depth_format = depth_format;
    a.bgr = bgr_dev;
    a.bgr_frames = bgr_frames;
    a.out = h->stage.written(out_dev);
    a.out_format = out_format;
    a.state[0] = h->state[0].p;
    a.state[1] = h->state[1].p;
    a.pass = pass_of_dev ? pass_of_dev : h->pass.p;
    a.space = h->space.p;
    a.range = h->range.p;
    a.partial = h->partial.p;
    a.filled = h->counts.p;
    a.remaining = h->counts.p + h->max_batch;
    KDE_TRY(launch_holefill(a, as_stream(stream)));
    h->stage.finished(n, out_format, a.out);
    return KDE_OK;
}

KDE_STAGE_DEPTH_GETTERS(kde_holefill_depth_device, kde_holefill_depth_host, kde_holefill, "kde_holefill_fill_batch", (size_t)h->width * h->height)
KDE_STAGE_COUNT_GETTERS(kde_holefill_filled_device, kde_holefill_filled_host, kde_holefill, "kde_holefill_fill_batch", h->counts.p, h->filled_host)
KDE_STAGE_COUNT_GETTERS(kde_holefill_remaining_device, kde_holefill_remaining_host, kde_holefill, "kde_holefill_fill_batch",
                        h->counts.p + h->max_batch, h->remaining_host)
