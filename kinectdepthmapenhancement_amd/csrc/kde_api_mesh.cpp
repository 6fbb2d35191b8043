// kde_api_mesh.cpp — OrganizedMesh (kde_mesh_*): the surface of main.cpp:211-300 as a triangle mesh of the organised grid, for a
// batch of frames on the device (mesh_kernels.hip): the dense cloud's records as vertices, index triples in raster order.
#include "kde_handles.h"

static_assert(sizeof(kde_mesh_triangle) == 12, "kde_mesh_triangle is a 12-byte record");
static_assert(sizeof(kde_mesh_params) == 32, "kde_mesh_params: five floats and three ints");

struct kde_mesh {
    int device = -1;                        // -1: created on a host without a device (no buffers; build_batch refuses)
    int width = 0, height = 0, max_batch = 1;
    kde_mesh_params p{};
    Camera cam{};                           // width, height from create; the rest from set_camera
    bool cam_set = false;
    int n_last = 0;                         // frames of the last build_batch (0: none yet)
    kde_cloud_point* vertices_last = nullptr;     // where the last build_batch wrote: the own buffers or the caller's
    kde_mesh_triangle* triangles_last = nullptr;
    DevBuf<uint32_t> seg, tri_seg;          // [max_batch][segments]
    DevBuf<uint32_t> counts, tri_counts;    // [max_batch]
    DevBuf<uint8_t> mask;                   // [max_batch][table pixels / 8]
    DevBuf<uint32_t> group_rank;            // [max_batch][table pixels / 64]
    DevBuf<uint8_t> code;                   // [max_batch][table pixels]
    DevBuf<kde_cloud_point> vertices;       // [max_batch][H][W]
    DevBuf<kde_mesh_triangle> triangles;    // [max_batch][2 (W-1) (H-1)]
    PinnedBuf<uint32_t> counts_host, tri_counts_host;
    PinnedBuf<kde_cloud_point> vertices_host;
    PinnedBuf<kde_mesh_triangle> triangles_host;
    std::vector<uint64_t> offsets, tri_offsets;   // [n_last + 1] of the last vertices_host / triangles_host
    size_t tri_slot() const { return 2 * (size_t)(width - 1) * (height - 1); }
};

// main.cpp:227-230 and the link of kde_speckle_default_params
static const kde_mesh_params kMeshDefaults = {50.0f, 15000.0f, 1000.0f, 1, 10.0f, 0.02f, KDE_MESH_DIAG_ADAPTIVE, 0};

// main.cpp:211-300: its literals; the mesh's own are the speckle filter's link and the adaptive cut
extern "C" int kde_mesh_default_params(kde_mesh_params* p)
{
    KDE_REQUIRE(p, "kde_mesh_default_params: null argument");
    *p = kMeshDefaults;
    return KDE_OK;
}

// main.cpp:211-300: the clouds of main.cpp:211-216, with faces
extern "C" int kde_mesh_create(kde_mesh** out, int width, int height, int max_batch, const kde_mesh_params* p)
{
    KDE_REQUIRE(out, "kde_mesh_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_mesh_create", width, height, max_batch));
    KDE_REQUIRE(width >= 2 && height >= 2, "kde_mesh_create: width=%d, height=%d must both be >= 2 (a quad has two rows and two columns)",
                width, height);
    const kde_mesh_params q = p ? *p : kMeshDefaults;
    KDE_REQUIRE(std::isfinite(q.z_min) && std::isfinite(q.z_max) && q.z_min < q.z_max,
                "kde_mesh_create: z_min=%g, z_max=%g must be finite with z_min < z_max", (double)q.z_min, (double)q.z_max);
    KDE_REQUIRE(std::isfinite(q.divisor) && q.divisor > 0.0f, "kde_mesh_create: divisor=%g must be finite and > 0", (double)q.divisor);
    KDE_REQUIRE(std::isfinite(q.max_diff) && q.max_diff >= 0.0f, "kde_mesh_create: max_diff=%g must be finite and >= 0", (double)q.max_diff);
    KDE_REQUIRE(std::isfinite(q.rel_diff) && q.rel_diff >= 0.0f, "kde_mesh_create: rel_diff=%g must be finite and >= 0", (double)q.rel_diff);
    KDE_REQUIRE(q.diagonal >= KDE_MESH_DIAG_AD && q.diagonal <= KDE_MESH_DIAG_ADAPTIVE,
                "kde_mesh_create: diagonal=%d is none of KDE_MESH_DIAG_AD, _BC, _ADAPTIVE (0..2)", q.diagonal);
    kde_mesh* h = new_handle<kde_mesh>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_mesh_create: out of host memory");
    h->p = q;
    h->p.negate_z = q.negate_z != 0;
    h->p.flip_winding = q.flip_winding != 0;
    h->cam.width = width;
    h->cam.height = height;
    if (h->device >= 0) {
        const size_t px = (size_t)width * height, tp = mesh_table_pixels(px), b = (size_t)max_batch;
        int rc = h->seg.alloc(b * cloud_segments(px));
        if (rc == KDE_OK) rc = h->tri_seg.alloc(b * cloud_segments(px));
        if (rc == KDE_OK) rc = h->counts.alloc(b);
        if (rc == KDE_OK) rc = h->tri_counts.alloc(b);
        if (rc == KDE_OK) rc = h->mask.alloc(b * (tp / 8));
        if (rc == KDE_OK) rc = h->group_rank.alloc(b * (tp / kMeshGroupPixels));
        if (rc == KDE_OK) rc = h->code.alloc(b * tp);
        if (rc == KDE_OK) rc = h->vertices.alloc(b * px);
        if (rc == KDE_OK) rc = h->triangles.alloc(b * h->tri_slot());
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

// main.cpp:211-300 holds its clouds in shared pointers
extern "C" int kde_mesh_destroy(kde_mesh* h)
{
    delete h;
    return KDE_OK;
}

// main.cpp:211-300 reads clouds made by convertor.projectiveToReal (main.cpp:168): the camera of DimensionConvertor.cpp:3-13
extern "C" int kde_mesh_set_camera(kde_mesh* h, const double* K9)
{
    KDE_REQUIRE(h && K9, "kde_mesh_set_camera: null argument");
    h->cam.fx = (float)K9[0];
    h->cam.fy = (float)K9[4];
    h->cam.cx = (int)K9[2];
    h->cam.cy = (int)K9[5];
    h->cam_set = true;
    return KDE_OK;
}

// main.cpp:211-300: the loop over the pixels for one method, n frames at once, and the faces between the points it keeps
extern "C" int kde_mesh_build_batch(kde_mesh* h, int n, const kde_error3d_source* src, const uint8_t* bgr_dev, int bgr_frames,
                                    kde_cloud_point* vertices_out_dev, kde_mesh_triangle* triangles_out_dev, void* stream)
{
    const char* who = "kde_mesh_build_batch";
    KDE_REQUIRE(h && src && bgr_dev, "%s: null argument", who);
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "%s: n=%d outside 1..max_batch=%d", who, n, h->max_batch);
    KDE_REQUIRE(bgr_frames == 1 || bgr_frames == n, "%s: bgr_frames=%d is neither 1 nor n=%d", who, bgr_frames, n);
    KDE_REQUIRE(src->format == KDE_SRC_POINTS_F32 || src->format == KDE_SRC_DEPTH_F32 || src->format == KDE_SRC_DEPTH_U16,
                "%s: the source has the unknown format %d", who, src->format);
    KDE_REQUIRE(src->data_dev, "%s: the source has a null data_dev", who);
    const uintptr_t align = src->format == KDE_SRC_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(src->data_dev) % align == 0, "%s: the source is not %d-byte aligned", who, (int)align);
    KDE_REQUIRE(src->format == KDE_SRC_POINTS_F32 || h->cam_set, "%s: the source is a depth map but kde_mesh_set_camera was not called", who);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(vertices_out_dev) % 16 == 0, "%s: vertices_out_dev is not 16-byte aligned", who);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(triangles_out_dev) % 4 == 0, "%s: triangles_out_dev is not 4-byte aligned", who);
    KDE_ON_DEVICE(h, who);
    if (h->device < 0) return fail(KDE_ERR_HIP, "%s: the handle was created on a host without a device", who);
    MeshLaunch a{};
    a.cloud.n = n;
    a.cloud.src = src->data_dev;
    a.cloud.format = src->format;
    a.cloud.bgr = bgr_dev;
    a.cloud.bgr_frames = bgr_frames;
    a.cloud.cam = h->cam;
    a.cloud.z_min = h->p.z_min;
    a.cloud.z_max = h->p.z_max;
    a.cloud.divisor = h->p.divisor;
    a.cloud.negate_z = h->p.negate_z;
    a.cloud.organized = 0;
    a.cloud.seg = h->seg.p;
    a.cloud.counts = h->counts.p;
    a.cloud.out = vertices_out_dev ? vertices_out_dev : h->vertices.p;
    a.max_diff = h->p.max_diff;
    a.rel_diff = h->p.rel_diff;
    a.diagonal = h->p.diagonal;
    a.flip_winding = h->p.flip_winding;
    a.mask = h->mask.p;
    a.group_rank = h->group_rank.p;
    a.code = h->code.p;
    a.tri_seg = h->tri_seg.p;
    a.tri_counts = h->tri_counts.p;
    a.triangles = triangles_out_dev ? triangles_out_dev : h->triangles.p;
    KDE_TRY(launch_mesh(a, as_stream(stream)));
    h->n_last = n;
    h->vertices_last = a.cloud.out;
    h->triangles_last = a.triangles;
    return KDE_OK;
}

#define KDE_MESH_DEVICE_GETTER(fn, type, expr)                                      \
    extern "C" int fn(kde_mesh* h, type** out)                                      \
    {                                                                               \
        KDE_REQUIRE(h && out, #fn ": null argument");                               \
        KDE_REQUIRE(h->n_last > 0, #fn ": kde_mesh_build_batch was not called");    \
        *out = (expr);                                                              \
        return KDE_OK;                                                              \
    }
// main.cpp:211-300: input .. result and their sizes, and the faces, of the last call
KDE_MESH_DEVICE_GETTER(kde_mesh_vertices_device, kde_cloud_point, h->vertices_last)
KDE_MESH_DEVICE_GETTER(kde_mesh_triangles_device, kde_mesh_triangle, h->triangles_last)
KDE_MESH_DEVICE_GETTER(kde_mesh_counts_device, uint32_t, h->counts.p)
KDE_MESH_DEVICE_GETTER(kde_mesh_tri_counts_device, uint32_t, h->tri_counts.p)

// main.cpp:211-300 builds its clouds on the host: the counts in pinned memory, ready when the call returns
extern "C" int kde_mesh_counts_host(kde_mesh* h, void* stream, const uint32_t** out)
{
    KDE_REQUIRE(h && out, "kde_mesh_counts_host: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_mesh_counts_host: kde_mesh_build_batch was not called");
    return host_mirror("kde_mesh_counts_host", h->device, h->counts.p, (size_t)h->n_last, (size_t)h->max_batch, h->counts_host,
                       as_stream(stream), out);
}

// main.cpp:211-300 has no faces: their number per frame in pinned memory, as its cloud->size()
extern "C" int kde_mesh_tri_counts_host(kde_mesh* h, void* stream, const uint32_t** out)
{
    KDE_REQUIRE(h && out, "kde_mesh_tri_counts_host: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_mesh_tri_counts_host: kde_mesh_build_batch was not called");
    return host_mirror("kde_mesh_tri_counts_host", h->device, h->tri_counts.p, (size_t)h->n_last, (size_t)h->max_batch,
                       h->tri_counts_host, as_stream(stream), out);
}

namespace {
// the first counts[f] records of every frame's slot of `slot` records, back to back in pinned memory behind offsets[n + 1]
template <typename T>
int packed_host(const char* who, kde_mesh* h, const uint32_t* counts_dev, PinnedBuf<uint32_t>& counts_host, const T* dev, size_t slot,
                PinnedBuf<T>& host, std::vector<uint64_t>& offsets, hipStream_t s, const T** out, const uint64_t** offsets_out)
{
    const uint32_t* counts = nullptr;
    KDE_TRY(host_mirror(who, h->device, counts_dev, (size_t)h->n_last, (size_t)h->max_batch, counts_host, s, &counts));
    const int n = h->n_last;
    try {
        offsets.assign((size_t)n + 1, 0);
    } catch (const std::bad_alloc&) {
        return fail(KDE_ERR_NOMEM, "%s: out of host memory", who);
    }
    for (int f = 0; f < n; f++) {
        KDE_REQUIRE(counts[f] <= slot, "%s: count[%d]=%u exceeds the frame's slot", who, f, counts[f]);
        offsets[f + 1] = offsets[f] + counts[f];
    }
    const size_t total = offsets[n];
    KDE_TRY(host.ensure(total ? total : 1));
    for (int f = 0; f < n; f++) {
        if (counts[f] == 0) continue;
        KDE_HIP_TRY(hipMemcpyAsync(host.p + offsets[f], dev + (size_t)f * slot, (size_t)counts[f] * sizeof(T), hipMemcpyDeviceToHost, s));
    }
    KDE_HIP_TRY(hipStreamSynchronize(s));
    *out = host.p;
    *offsets_out = offsets.data();
    return KDE_OK;
}
}  // namespace

// main.cpp:211-300 builds its clouds on the host: the frames' vertices back to back in pinned memory
extern "C" int kde_mesh_vertices_host(kde_mesh* h, void* stream, const kde_cloud_point** out, const uint64_t** offsets)
{
    const char* who = "kde_mesh_vertices_host";
    KDE_REQUIRE(h && out && offsets, "%s: null argument", who);
    KDE_REQUIRE(h->n_last > 0, "%s: kde_mesh_build_batch was not called", who);
    return packed_host(who, h, h->counts.p, h->counts_host, h->vertices_last, (size_t)h->width * h->height, h->vertices_host, h->offsets,
                       as_stream(stream), out, offsets);
}

// main.cpp:211-300 has no faces: the frames' triangles back to back in pinned memory, like its points
extern "C" int kde_mesh_triangles_host(kde_mesh* h, void* stream, const kde_mesh_triangle** out, const uint64_t** offsets)
{
    const char* who = "kde_mesh_triangles_host";
    KDE_REQUIRE(h && out && offsets, "%s: null argument", who);
    KDE_REQUIRE(h->n_last > 0, "%s: kde_mesh_build_batch was not called", who);
    return packed_host(who, h, h->tri_counts.p, h->tri_counts_host, h->triangles_last, h->tri_slot(), h->triangles_host, h->tri_offsets,
                       as_stream(stream), out, offsets);
}
