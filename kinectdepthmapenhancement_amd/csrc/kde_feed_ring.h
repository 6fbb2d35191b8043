// kde_feed_ring.h — what the host-fed entry points share (kde_jbf_feed_*, kde_enh_feed_*): three non-blocking streams, a
// ring of slots with their events and pinned staging buffers, and the chunk loop that overlaps the copy-in of one chunk,
// the kernels of the next older and the copy-out of the one before that.  A feed derives from FeedRing, owns the device
// buffers of its slots and gives the loop two callbacks: one that sizes a slot, one that launches a chunk's kernels.
#pragma once

#include "kde_handles.h"

#include <chrono>

namespace kde {

// Slot ring: chunk c uses slot c % kFeedSlots.  Three slots let the copy-in of chunk c, the kernels of c - 1 and the
// copy-out of c - 2 run at the same time; the next use of a slot waits for its copy-out (the H2D stream waits on the
// slot's d2h_done event), so the only host waits are on the feed's own events.
constexpr int kFeedSlots = 3;

struct FeedRingSlot {
    PinnedBuf<uint8_t> in_host;     // pageable inputs: depth bytes then bgr bytes of one chunk
    PinnedBuf<uint8_t> out_host;    // pageable outputs: one chunk
    hipEvent_t ev[6] = {};          // h2d start / done, compute start / done, d2h start / done (timing enabled)
};

// the device side of a slot as the loop sees it: where a chunk's depth and colour land and where its output is read
struct FeedSlotDev {
    void* depth = nullptr;          // [chunk][H][W] of the call's depth element
    uint8_t* bgr = nullptr;         // [chunk][H][W][3]
    const void* out = nullptr;      // [chunk][H][W] of the call's output element
};

// true when [p, p + bytes) is pinned host memory the DMA engines can read directly (both ends are checked; the
// header requires the extent to lie in one allocation).  Errors and hipMemoryTypeUnregistered mean pageable.
inline bool host_pinned(const void* p, size_t bytes)
{
    const char* ends[2] = {static_cast<const char*>(p), static_cast<const char*>(p) + bytes - 1};
    for (const char* q : ends) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, q) != hipSuccess) {
            (void)hipGetLastError();     // the lookup of an unknown pointer leaves a sticky error behind
            return false;
        }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}

inline float span_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) {
        (void)hipGetLastError();
        return 0.0f;
    }
    return ms;
}

struct FeedRing {
    using Clock = std::chrono::steady_clock;
    int device = -1;
    int chunk = 1;
    hipStream_t h2d = nullptr, comp = nullptr, d2h = nullptr;
    FeedRingSlot slot[kFeedSlots];
    kde_feed_stats stats{};

    FeedRing() = default;
    FeedRing(const FeedRing&) = delete;
    FeedRing& operator=(const FeedRing&) = delete;
    ~FeedRing()
    {
        // a call always ends with every slot idle (or fails after synchronising its streams), so nothing is in flight here
        for (FeedRingSlot& s : slot)
            for (hipEvent_t& e : s.ev)
                if (e) (void)hipEventDestroy(e);
        if (h2d) (void)hipStreamDestroy(h2d);
        if (comp) (void)hipStreamDestroy(comp);
        if (d2h) (void)hipStreamDestroy(d2h);
    }

    // the streams and events of a feed of `device` (the current one) that works in chunks of `chunk_frames`
    int open(const char* who, int device_, int chunk_frames)
    {
        device = device_;
        chunk = chunk_frames;
        hipError_t e = hipStreamCreateWithFlags(&h2d, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&comp, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&d2h, hipStreamNonBlocking);
        for (FeedRingSlot& s : slot)
            for (hipEvent_t& ev : s.ev)
                if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e != hipSuccess) return fail(KDE_ERR_HIP, "%s: stream / event creation failed: %s", who, hipGetErrorString(e));
        return KDE_OK;
    }

    // One blocking call: n frames of px pixels from depth_host (dsz bytes per pixel) and bgr_host to out_host (osz bytes
    // per pixel).  prepare(k, cf, dev) sizes slot k for chunks of cf frames and says where its buffers are; compute(k, fr)
    // launches the kernels of a chunk of fr frames in slot k on `comp`.  t0 is the caller's entry time (stats.wall_ms).
    // On failure the three streams are synchronised, so that no copy is in flight into or out of the caller's memory, and
    // `stats` keeps the previous call's record.
    template <class Prepare, class Compute>
    int process(Clock::time_point t0, size_t px, int n, const void* depth_host, size_t dsz, const uint8_t* bgr_host,
                void* out_host, size_t osz, Prepare prepare, Compute compute)
    {
        kde_feed_stats st{};
        const int rc = run(px, n, depth_host, dsz, bgr_host, out_host, osz, st, prepare, compute);
        if (rc != KDE_OK) {
            (void)hipStreamSynchronize(h2d);
            (void)hipStreamSynchronize(comp);
            (void)hipStreamSynchronize(d2h);
            return rc;
        }
        st.wall_ms = std::chrono::duration<float, std::milli>(Clock::now() - t0).count();
        stats = st;
        return KDE_OK;
    }

private:
    template <class Prepare, class Compute>
    int run(size_t px, int n, const void* depth_host, size_t dsz, const uint8_t* bgr_host, void* out_host, size_t osz,
            kde_feed_stats& st, Prepare& prepare, Compute& compute)
    {
        const int cf = std::min(chunk, n);                          // frames per chunk in this call
        const int chunks = (n + cf - 1) / cf;
        const int used = std::min(chunks, kFeedSlots);
        const bool in_pinned = host_pinned(depth_host, px * n * dsz) && host_pinned(bgr_host, px * n * 3);
        const bool out_pinned = host_pinned(out_host, px * n * osz);
        st.frames = n;
        st.chunks = chunks;
        st.chunk_frames = cf;
        st.inputs_staged = in_pinned ? 0 : 1;
        st.outputs_staged = out_pinned ? 0 : 1;

        // every slot is idle between calls: (re)size what this call uses.  Every launch and copy below stays inside the
        // extents prepare() vouches for (px * fr <= px * cf elements per chunk)
        FeedSlotDev dev[kFeedSlots];
        for (int k = 0; k < used; k++) {
            KDE_TRY(prepare(k, cf, dev[k]));
            if (!in_pinned) KDE_TRY(slot[k].in_host.ensure(px * cf * (dsz + 3)));
            if (!out_pinned) KDE_TRY(slot[k].out_host.ensure(px * cf * osz));
        }

        const uint8_t* dsrc = static_cast<const uint8_t*>(depth_host);
        uint8_t* odst = static_cast<uint8_t*>(out_host);
        // chunk c's pageable output: wait for its copy-out, then hand it to the caller
        auto drain = [&](int c) -> int {
            FeedRingSlot& s = slot[c % kFeedSlots];
            const int fr = std::min(cf, n - c * cf);
            KDE_HIP_TRY(hipEventSynchronize(s.ev[5]));
            memcpy(odst + px * cf * c * osz, s.out_host.p, px * fr * osz);
            return KDE_OK;
        };
        // chunk c's three spans, read once its last event has completed and before its slot is recorded again
        auto harvest = [&](int c) -> int {
            FeedRingSlot& s = slot[c % kFeedSlots];
            KDE_HIP_TRY(hipEventSynchronize(s.ev[5]));
            st.h2d_ms += span_ms(s.ev[0], s.ev[1]);
            st.compute_ms += span_ms(s.ev[2], s.ev[3]);
            st.d2h_ms += span_ms(s.ev[4], s.ev[5]);
            return KDE_OK;
        };
        for (int c = 0; c < chunks; c++) {
            const int k = c % kFeedSlots;
            FeedRingSlot& s = slot[k];
            const int fr = std::min(cf, n - c * cf);
            const size_t first = (size_t)c * cf;
            if (c >= kFeedSlots) {                        // the slot's previous chunk: its output to the caller, its spans,
                if (!out_pinned) KDE_TRY(drain(c - kFeedSlots));
                KDE_TRY(harvest(c - kFeedSlots));         // and its staging buffers are free again
            }
            // 1. copy-in, once the slot has been consumed
            const void* din = dsrc + px * first * dsz;
            const uint8_t* cin = bgr_host + px * first * 3;
            if (!in_pinned) {
                memcpy(s.in_host.p, din, px * fr * dsz);
                memcpy(s.in_host.p + px * fr * dsz, cin, px * fr * 3);
                din = s.in_host.p;
                cin = s.in_host.p + px * fr * dsz;
            }
            if (c >= kFeedSlots) KDE_HIP_TRY(hipStreamWaitEvent(h2d, s.ev[5], 0));   // the slot's previous copy-out
            KDE_HIP_TRY(hipEventRecord(s.ev[0], h2d));
            KDE_HIP_TRY(hipMemcpyAsync(dev[k].depth, din, px * fr * dsz, hipMemcpyHostToDevice, h2d));
            KDE_HIP_TRY(hipMemcpyAsync(dev[k].bgr, cin, px * fr * 3, hipMemcpyHostToDevice, h2d));
            KDE_HIP_TRY(hipEventRecord(s.ev[1], h2d));
            // 2. the chunk's kernels, into the slot's own output buffer
            KDE_HIP_TRY(hipStreamWaitEvent(comp, s.ev[1], 0));
            KDE_HIP_TRY(hipEventRecord(s.ev[2], comp));
            KDE_TRY(compute(k, fr));
            KDE_HIP_TRY(hipEventRecord(s.ev[3], comp));
            // 3. copy-out
            KDE_HIP_TRY(hipStreamWaitEvent(d2h, s.ev[3], 0));
            KDE_HIP_TRY(hipEventRecord(s.ev[4], d2h));
            void* dst = out_pinned ? static_cast<void*>(odst + px * first * osz) : static_cast<void*>(s.out_host.p);
            KDE_HIP_TRY(hipMemcpyAsync(dst, dev[k].out, px * fr * osz, hipMemcpyDeviceToHost, d2h));
            KDE_HIP_TRY(hipEventRecord(s.ev[5], d2h));
            st.h2d_bytes += px * fr * (dsz + 3);
            st.d2h_bytes += px * fr * osz;
        }
        for (int c = std::max(0, chunks - kFeedSlots); c < chunks; c++) {
            if (!out_pinned) KDE_TRY(drain(c));
            KDE_TRY(harvest(c));
        }
        return KDE_OK;
    }
};

}  // namespace kde
