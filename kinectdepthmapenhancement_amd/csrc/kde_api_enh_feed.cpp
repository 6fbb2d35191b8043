// kde_api_enh_feed.cpp — the enhanced cloud as a depth map (kde_points_to_depth, stream_kernels.hip) and
// KinectDepthEnhancement::Process on frames in host memory (kde_enh_feed_*), on the ring of kde_feed_ring.h.
#include "kde_feed_ring.h"

extern "C" int kde_points_to_depth(size_t n_points, const kde_float3* points_dev, int depth_format, void* depth_dev, void* stream)
{
    if (n_points == 0) return KDE_OK;       // nothing to write: no launch, and no argument is looked at
    KDE_REQUIRE(depth_format == KDE_DEPTH_F32 || depth_format == KDE_DEPTH_U16, "kde_points_to_depth: unknown depth_format %d",
                depth_format);
    KDE_REQUIRE(points_dev && depth_dev, "kde_points_to_depth: null argument");
    const uintptr_t out_align = depth_format == KDE_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(points_dev) % sizeof(float) == 0, "kde_points_to_depth: points_dev is not 4-byte aligned");
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(depth_dev) % out_align == 0, "kde_points_to_depth: depth_dev is not %d-byte aligned",
                (int)out_align);
    return launch_points_to_depth(points_dev, depth_dev, n_points, depth_format == KDE_DEPTH_U16, as_stream(stream));
}

// -----------------------------------------------------------------------------------------------------
// host-fed KinectDepthEnhancement (kde_enh_feed_*)
// -----------------------------------------------------------------------------------------------------
struct EnhFeedSlot {
    DevBuf<float> depth;            // [chunk][H][W] f32: the copied-in depth, or the widened uint16 depth
    DevBuf<uint16_t> depth16;       // [chunk][H][W] landing area of uint16 depth
    DevBuf<uint8_t> bgr;            // [chunk][H][W][3]
    DevBuf<uint8_t> out;            // [chunk][H][W] of 12, 4 or 2 bytes: what the copy-out reads
};

struct kde_enh_feed : FeedRing {
    kde_enh* enh = nullptr;
    EnhFeedSlot buf[kFeedSlots];
};

extern "C" int kde_enh_feed_create(kde_enh_feed** out, kde_enh* enh, int chunk_frames)
{
    KDE_REQUIRE(out, "kde_enh_feed_create: null out");
    *out = nullptr;
    KDE_REQUIRE(enh, "kde_enh_feed_create: null enh handle");
    KDE_REQUIRE(chunk_frames >= 1 && chunk_frames <= enh->max_batch, "kde_enh_feed_create: chunk_frames=%d outside 1..max_batch=%d",
                chunk_frames, enh->max_batch);
    KDE_ON_DEVICE(enh->NASP, "kde_enh_feed_create");
    kde_enh_feed* f = new (std::nothrow) kde_enh_feed;
    if (!f) return fail(KDE_ERR_NOMEM, "kde_enh_feed_create: out of host memory");
    f->enh = enh;
    const int rc = f->open("kde_enh_feed_create", enh->NASP->device, chunk_frames);
    if (rc != KDE_OK) {
        delete f;
        return rc;
    }
    *out = f;
    return KDE_OK;
}

extern "C" int kde_enh_feed_destroy(kde_enh_feed* f)
{
    delete f;
    return KDE_OK;
}

extern "C" int kde_enh_feed_last_stats(kde_enh_feed* f, kde_feed_stats* out)
{
    KDE_REQUIRE(f && out, "kde_enh_feed_last_stats: null argument");
    *out = f->stats;
    return KDE_OK;
}

extern "C" int kde_enh_feed_process(kde_enh_feed* f, int n, const void* depth_host, int depth_format, const uint8_t* bgr_host,
                                    int out_format, void* out_host)
{
    const auto t0 = FeedRing::Clock::now();
    KDE_REQUIRE(f, "kde_enh_feed_process: null feed");
    KDE_REQUIRE(depth_host && bgr_host && out_host, "kde_enh_feed_process: null host buffer");
    KDE_REQUIRE(n >= 1, "kde_enh_feed_process: n=%d < 1", n);
    KDE_REQUIRE(depth_format == KDE_DEPTH_F32 || depth_format == KDE_DEPTH_U16, "kde_enh_feed_process: unknown depth_format %d",
                depth_format);
    KDE_REQUIRE(out_format == KDE_OUT_POINTS_F32 || out_format == KDE_OUT_DEPTH_F32 || out_format == KDE_OUT_DEPTH_U16,
                "kde_enh_feed_process: unknown out_format %d", out_format);
    KDE_ON_DEVICE(f, "kde_enh_feed_process");
    kde_enh* h = f->enh;
    const size_t px = (size_t)h->width * h->height;
    const bool u16 = depth_format == KDE_DEPTH_U16;
    const size_t osz = out_format == KDE_OUT_POINTS_F32 ? sizeof(kde_float3) : out_format == KDE_OUT_DEPTH_F32 ? sizeof(float) : sizeof(uint16_t);
    // a slot grows to what a call needs (chunks are at most max_batch frames): another depth or output format, or a longer
    // chunk than the calls before, reallocates only the buffer that is too small
    auto prepare = [&](int k, int cf, FeedSlotDev& dev) -> int {
        EnhFeedSlot& s = f->buf[k];
        if (s.depth.n < px * cf) KDE_TRY(s.depth.alloc(px * cf));
        if (u16 && s.depth16.n < px * cf) KDE_TRY(s.depth16.alloc(px * cf));
        if (s.bgr.n < px * 3 * cf) KDE_TRY(s.bgr.alloc(px * 3 * cf));
        if (s.out.n < px * cf * osz) KDE_TRY(s.out.alloc(px * cf * osz));
        dev.depth = u16 ? static_cast<void*>(s.depth16.p) : static_cast<void*>(s.depth.p);
        dev.bgr = s.bgr.p;
        dev.out = s.out.p;
        return KDE_OK;
    };
    // widen (u16), Process on the borrowed object, then its optimized points into the slot as the call's output format:
    // the copy-out reads the slot, so the next chunk's Process may overwrite the object's buffers
    auto compute = [&](int k, int fr) -> int {
        EnhFeedSlot& s = f->buf[k];
        if (u16) KDE_TRY(launch_widen_u16(s.depth16.p, s.depth.p, px * fr, f->comp));
        KDE_TRY(kde_enh_process_batch(h, fr, s.depth.p, s.bgr.p, f->comp));
        const kde_float3* optimized = h->Projector->optimized.p;
        if (out_format == KDE_OUT_POINTS_F32) {
            KDE_HIP_TRY(hipMemcpyAsync(s.out.p, optimized, px * fr * sizeof(kde_float3), hipMemcpyDeviceToDevice, f->comp));
            return KDE_OK;
        }
        return launch_points_to_depth(optimized, s.out.p, px * fr, out_format == KDE_OUT_DEPTH_U16, f->comp);
    };
    return f->process(t0, px, n, depth_host, u16 ? sizeof(uint16_t) : sizeof(float), bgr_host, out_host, osz, prepare, compute);
}
