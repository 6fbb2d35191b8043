// kde_api_error3d.cpp — MeanError3D (kde_error3d_*): the reference's quality figure, main.cpp:220-308, for a batch of
// frames and up to eight candidate results on the device (error3d_kernels.hip).
#include "kde_handles.h"

static_assert(sizeof(kde_error3d_result) == 16, "kde_error3d_result is a 16-byte record");

struct kde_error3d {
    int device = -1;                        // -1: created on a host without a device (no buffers; compare_batch refuses)
    int width = 0, height = 0, max_batch = 1;
    int max_candidates = 1;
    Camera cam{};                           // width, height from create; the rest from set_camera
    bool cam_set = false;
    float z_min = 50.0f, z_max = 15000.0f;  // main.cpp:227
    int n_last = 0, m_last = 0;             // frames and candidates of the last compare_batch (0: none yet)
    DevBuf<Error3dPartial> partials;        // [max_batch][max_candidates][segments]
    DevBuf<kde_error3d_result> results;     // [max_batch][max_candidates]
    PinnedBuf<kde_error3d_result> results_host;
};

// main.cpp:220-308: the accumulators of main.cpp:217-218, per frame and candidate
extern "C" int kde_error3d_create(kde_error3d** out, int width, int height, int max_batch, int max_candidates)
{
    KDE_REQUIRE(out, "kde_error3d_create: null out");
    *out = nullptr;
    KDE_TRY(check_frame_batch("kde_error3d_create", width, height, max_batch));
    KDE_REQUIRE(max_candidates >= 1 && max_candidates <= kError3dMaxCandidates, "kde_error3d_create: max_candidates=%d outside 1..%d",
                max_candidates, kError3dMaxCandidates);
    kde_error3d* h = new_handle<kde_error3d>(width, height, max_batch);
    if (!h) return fail(KDE_ERR_NOMEM, "kde_error3d_create: out of host memory");
    h->max_candidates = max_candidates;
    h->cam.width = width;
    h->cam.height = height;
    if (h->device >= 0) {
        const size_t pairs = (size_t)max_batch * max_candidates;
        int rc = h->partials.alloc(pairs * error3d_segments((size_t)width * height));
        if (rc == KDE_OK) rc = h->results.alloc(pairs);
        if (rc != KDE_OK) {
            delete h;
            return rc;
        }
    }
    *out = h;
    return KDE_OK;
}

// main.cpp:220-308 keeps its accumulators on the stack
extern "C" int kde_error3d_destroy(kde_error3d* h)
{
    delete h;
    return KDE_OK;
}

// main.cpp:220-308 reads clouds made by convertor.projectiveToReal (main.cpp:168): the camera of DimensionConvertor.cpp:3-13
extern "C" int kde_error3d_set_camera(kde_error3d* h, const double* K9)
{
    KDE_REQUIRE(h && K9, "kde_error3d_set_camera: null argument");
    h->cam.fx = (float)K9[0];
    h->cam.fy = (float)K9[4];
    h->cam.cx = (int)K9[2];
    h->cam.cy = (int)K9[5];
    h->cam_set = true;
    return KDE_OK;
}

// main.cpp:220-308: the literals 50.0f and 15000.0f of its validity tests
extern "C" int kde_error3d_set_range(kde_error3d* h, float z_min, float z_max)
{
    KDE_REQUIRE(h, "kde_error3d_set_range: null handle");
    KDE_REQUIRE(std::isfinite(z_min) && std::isfinite(z_max) && z_min < z_max,
                "kde_error3d_set_range: z_min=%g, z_max=%g must be finite with z_min < z_max", (double)z_min, (double)z_max);
    h->z_min = z_min;
    h->z_max = z_max;
    return KDE_OK;
}

static int error3d_check_source(const kde_error3d* h, const kde_error3d_source& s, const char* what, int index)
{
    const char* who = "kde_error3d_compare_batch";
    KDE_REQUIRE(s.format == KDE_SRC_POINTS_F32 || s.format == KDE_SRC_DEPTH_F32 || s.format == KDE_SRC_DEPTH_U16,
                "%s: %s %d has the unknown format %d", who, what, index, s.format);
    KDE_REQUIRE(s.data_dev, "%s: %s %d has a null data_dev", who, what, index);
    const uintptr_t align = s.format == KDE_SRC_DEPTH_U16 ? sizeof(uint16_t) : sizeof(float);
    KDE_REQUIRE(reinterpret_cast<uintptr_t>(s.data_dev) % align == 0, "%s: %s %d is not %d-byte aligned", who, what, index, (int)align);
    KDE_REQUIRE(s.format == KDE_SRC_POINTS_F32 || h->cam_set, "%s: %s %d is a depth map but kde_error3d_set_camera was not called", who,
                what, index);
    return KDE_OK;
}

// main.cpp:220-308: the loop over the pixels, for n frames and m candidates at once
extern "C" int kde_error3d_compare_batch(kde_error3d* h, int n, int m, const kde_error3d_source* candidates,
                                         const kde_error3d_source* truth, int truth_frames, void* stream)
{
    KDE_REQUIRE(h && candidates && truth, "kde_error3d_compare_batch: null argument");
    KDE_REQUIRE(n >= 1 && n <= h->max_batch, "kde_error3d_compare_batch: n=%d outside 1..max_batch=%d", n, h->max_batch);
    KDE_REQUIRE(m >= 1 && m <= h->max_candidates, "kde_error3d_compare_batch: m=%d outside 1..max_candidates=%d", m, h->max_candidates);
    KDE_REQUIRE(truth_frames == 1 || truth_frames == n, "kde_error3d_compare_batch: truth_frames=%d is neither 1 nor n=%d", truth_frames, n);
    Error3dLaunch a{};
    for (int c = 0; c < m; c++) {
        KDE_TRY(error3d_check_source(h, candidates[c], "candidate", c));
        a.cand[c] = candidates[c].data_dev;
        a.cand_format[c] = candidates[c].format;
    }
    KDE_TRY(error3d_check_source(h, *truth, "truth", 0));
    KDE_ON_DEVICE(h, "kde_error3d_compare_batch");
    if (h->device < 0) return fail(KDE_ERR_HIP, "kde_error3d_compare_batch: the handle was created on a host without a device");
    a.n = n;
    a.m = m;
    a.truth = truth->data_dev;
    a.truth_format = truth->format;
    a.truth_frames = truth_frames;
    a.cam = h->cam;
    a.z_min = h->z_min;
    a.z_max = h->z_max;
    a.partials = h->partials.p;
    a.results = h->results.p;
    KDE_TRY(launch_error3d(a, as_stream(stream)));
    h->n_last = n;
    h->m_last = m;
    return KDE_OK;
}

// main.cpp:220-308: input_average .. result_average and their counts, [n][m] of the last call
extern "C" int kde_error3d_results_device(kde_error3d* h, kde_error3d_result** out)
{
    KDE_REQUIRE(h && out, "kde_error3d_results_device: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_error3d_results_device: kde_error3d_compare_batch was not called");
    *out = h->results.p;
    return KDE_OK;
}

// main.cpp:220-308 computes on the host: the table in pinned memory, ready when the call returns
extern "C" int kde_error3d_results_host(kde_error3d* h, void* stream, const kde_error3d_result** out)
{
    KDE_REQUIRE(h && out, "kde_error3d_results_host: null argument");
    KDE_REQUIRE(h->n_last > 0, "kde_error3d_results_host: kde_error3d_compare_batch was not called");
    return host_mirror("kde_error3d_results_host", h->device, h->results.p, (size_t)h->n_last * h->m_last,
                       (size_t)h->max_batch * h->max_candidates, h->results_host, as_stream(stream), out);
}
