// kde_depth_stage.h — what the depth-in / depth-out stages share (kde_api_reg.cpp, kde_api_undist.cpp, kde_api_upsample.cpp,
// kde_api_holefill.cpp): n depth frames in as float32 or uint16, n frames out in either format into the caller's buffer or
// the object's own, a record of where the last call wrote, per-frame counts on the device or through a pinned mirror.
// Included by kde_handles.h, whose rules it builds on; depth_format_ok / depth_element / kColourRange are in kde_internal.h,
// where the launchers read them too.  Every check takes `who`, the entry point's name, and words its refusal as that entry
// point always did; the ORDER of the checks belongs to each entry point and stays there ("Depth stages").
#pragma once

namespace kde {

// ---- what a create() checks ---------------------------------------------------------------------------
// why: what follows "must be finite and >= 0" where a stage has a reason of its own to give
inline int check_z_range(const char* who, float z_min, float z_max, const char* why = "")
{
    KDE_REQUIRE(std::isfinite(z_min) && z_min >= 0.0f, "%s: z_min=%g must be finite and >= 0%s", who, (double)z_min, why);
    KDE_REQUIRE(z_min < z_max, "%s: z_min=%g must be below z_max=%g", who, (double)z_min, (double)z_max);
    return KDE_OK;
}

inline int check_max_gap(const char* who, float max_gap)
{
    KDE_REQUIRE(std::isfinite(max_gap) && max_gap >= 0.0f, "%s: max_gap=%g must be finite and >= 0 (0: no guard)", who, (double)max_gap);
    return KDE_OK;
}

inline int check_sigma(const char* who, const char* name, float sigma)
{
    KDE_REQUIRE(std::isfinite(sigma) && sigma > 0.0f, "%s: %s=%g must be finite and > 0", who, name, (double)sigma);
    return KDE_OK;
}

// ---- what a batch call checks -------------------------------------------------------------------------
inline int check_batch_n(const char* who, int n, int max_batch)
{
    KDE_REQUIRE(n >= 1 && n <= max_batch, "%s: n=%d outside 1..max_batch=%d", who, n, max_batch);
    return KDE_OK;
}

inline int check_bgr_frames(const char* who, int bgr_frames, int n)
{
    KDE_REQUIRE(bgr_frames == 1 || bgr_frames == n, "%s: bgr_frames=%d is neither 1 nor n=%d", who, bgr_frames, n);
    return KDE_OK;
}

// validation never dereferences a device pointer: its format and its alignment are all that is asked of it
inline int check_depth_in(const char* who, const void* depth_dev, int depth_format)
{
    KDE_REQUIRE(depth_format_ok(depth_format), "%s: the unknown depth format %d", who, depth_format);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(depth_dev) % depth_element(depth_format) == 0, "%s: depth_dev is not %d-byte aligned", who,
                (int)depth_element(depth_format));
    return KDE_OK;
}

// out_dev == nullptr (the object-owned buffer) is aligned for either format
inline int check_depth_out(const char* who, const void* out_dev, int out_format)
{
    KDE_REQUIRE(depth_format_ok(out_format), "%s: the unknown output format %d", who, out_format);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(out_dev) % depth_element(out_format) == 0, "%s: out_dev is not %d-byte aligned", who,
                (int)depth_element(out_format));
    return KDE_OK;
}

// the last check in front of a launch: the handle's device is current, and there is one (device -1: created without buffers)
inline int check_has_device(const char* who, int device)
{
    KDE_TRY(check_on_device(device, who));
    if (device < 0) return fail(KDE_ERR_HIP, "%s: the handle was created on a host without a device", who);
    return KDE_OK;
}

// ---- the member every depth-stage handle embeds as `stage` ----------------------------------------------
struct DepthStage {
    int n_last = 0;                         // frames of the last batch call (0: none yet)
    int format_last = KDE_DEPTH_F32;        // its out_format
    void* out_last = nullptr;               // where it wrote: depth or the caller's buffer
    DevBuf<float> depth;                    // [max_batch][output frame]: floats, or uint16 in the same bytes
    PinnedBuf<float> depth_host;

    void* written(void* out_dev) const { return out_dev ? out_dev : static_cast<void*>(depth.p); }
    void finished(int n, int out_format, void* out)
    {
        n_last = n;
        format_last = out_format;
        out_last = out;
    }
    // batch: the name of the stage's batch function, which a getter asks to have been called
    int called(const char* who, const char* batch) const
    {
        KDE_REQUIRE(n_last > 0, "%s: %s was not called", who, batch);
        return KDE_OK;
    }
    int depth_device(const char* who, const char* batch, void** out) const
    {
        KDE_TRY(called(who, batch));
        *out = out_last;
        return KDE_OK;
    }
    // the frames of the last call in pinned memory, ready when the call returns; px: the pixels of an output frame
    int depth_host_copy(const char* who, const char* batch, int device, int max_batch, size_t px, hipStream_t s, const void** out)
    {
        KDE_TRY(called(who, batch));
        KDE_TRY(check_on_device(device, who));
        KDE_TRY(depth_host.ensure((size_t)max_batch * px));
        KDE_HIP_TRY(hipMemcpyAsync(depth_host.p, out_last, (size_t)n_last * px * depth_element(format_last), hipMemcpyDeviceToHost, s));
        KDE_HIP_TRY(hipStreamSynchronize(s));
        *out = depth_host.p;
        return KDE_OK;
    }
    // For a stage whose workgroups read their neighbours' input while those write (DepthHoleFilling; the gathers and the scatter
    // of the other three allow what they allow).  The buffer that is written is the caller's or the object's own, which a caller
    // holds after *_depth_device (a device-less object has none).  px: the pixels of the whole call; out_px: those it writes,
    // where they are fewer (DepthDecimation); 0, the default, means the same as px.
    int check_not_in_place(const char* who, const void* depth_dev, int depth_format, void* out_dev, int out_format, size_t px,
                           size_t out_px = 0) const
    {
        const void* w = written(out_dev);
        if (!w) return KDE_OK;
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(depth_dev), d1 = d0 + px * depth_element(depth_format);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(w), o1 = o0 + (out_px ? out_px : px) * depth_element(out_format);
        KDE_REQUIRE(o1 <= d0 || d1 <= o0, "%s: %s overlaps depth_dev (in place is not supported)", who,
                    out_dev ? "out_dev" : "the object-owned output buffer, which out_dev == NULL selects,");
        return KDE_OK;
    }
};

// extern "C" *_depth_device / *_depth_host of a stage; px: the pixels of an output frame, from h
#define KDE_STAGE_DEPTH_GETTERS(fn_device, fn_host, handle, batch, px)                                                        \
    extern "C" int fn_device(handle* h, void** out)                                                                           \
    {                                                                                                                         \
        KDE_REQUIRE(h && out, #fn_device ": null argument");                                                                  \
        return h->stage.depth_device(#fn_device, batch, out);                                                                 \
    }                                                                                                                         \
    extern "C" int fn_host(handle* h, void* stream, const void** out)                                                         \
    {                                                                                                                         \
        KDE_REQUIRE(h && out, #fn_host ": null argument");                                                                    \
        return h->stage.depth_host_copy(#fn_host, batch, h->device, h->max_batch, (px), as_stream(stream), out);              \
    }

// extern "C" *_device / *_host of a per-frame count: dev is its device array [max_batch], host its PinnedBuf, both from h
#define KDE_STAGE_COUNT_GETTERS(fn_device, fn_host, handle, batch, dev, host)                                                 \
    extern "C" int fn_device(handle* h, uint32_t** out)                                                                       \
    {                                                                                                                         \
        KDE_REQUIRE(h && out, #fn_device ": null argument");                                                                  \
        KDE_TRY(h->stage.called(#fn_device, batch));                                                                          \
        *out = (dev);                                                                                                         \
        return KDE_OK;                                                                                                        \
    }                                                                                                                         \
    extern "C" int fn_host(handle* h, void* stream, const uint32_t** out)                                                     \
    {                                                                                                                         \
        KDE_REQUIRE(h && out, #fn_host ": null argument");                                                                    \
        KDE_TRY(h->stage.called(#fn_host, batch));                                                                            \
        return host_mirror(#fn_host, h->device, (dev), (size_t)h->stage.n_last, (size_t)h->max_batch, (host), as_stream(stream), out); \
    }

// ---- the range table of a colour guide ----------------------------------------------------------------
// table[k] for k = |db| + |dg| + |dr| = 0 .. kColourRange - 1, as kde_hip.h states it
inline void colour_range_table(float sigma_color, float* table)
{
    for (int k = 0; k < kColourRange; k++) table[k] = (float)std::exp(-(double)(k * k) / (2.0 * (double)sigma_color * (double)sigma_color));
}

// the body of a *_range_table getter; range_host: the handle's table, nullptr for a null handle
inline int copy_range_table(const char* who, const std::vector<float>* range_host, float* table_host, int capacity)
{
    KDE_REQUIRE(range_host && table_host, "%s: null argument", who);
    KDE_REQUIRE(capacity >= kColourRange, "%s: capacity=%d is below the %d entries of the table", who, capacity, kColourRange);
    std::memcpy(table_host, range_host->data(), kColourRange * sizeof(float));
    return KDE_OK;
}

}  // namespace kde
