// decimate_demo.cpp — the multi-resolution chain on the classes of include/kde/kde.hpp:
//   DepthDecimation (depth and guide, k = 2) -> JointBilateralFilter at the small size -> GuidedDepthUpsampling back under the
//   full-resolution guide.
//   The scene is a wall at 2000 mm with a box at 1200 mm in front of it, +-6 mm of depth noise and 3 % dropouts.  The lower
//   median of a 2 x 2 block closes almost every dropout, lowers the noise and never invents a depth between the box and the
//   wall, which an average pool does along the whole outline of the box; the filter then runs on a quarter of the pixels (it
//   blends a little along the outline, as it does at any size), and the upsampler puts the outline back where the
//   full-resolution colour has it.  Everything stays on the device.
// Usage: decimate_demo [W H] (multiples of 2).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 640, H = argc > 2 ? std::atoi(argv[2]) : 480, K = 2;
    if (W < 64 || H < 64 || W % K || H % K) return 1;
    const size_t px = (size_t)W * H;
    std::vector<float> depth(px);
    std::vector<uint8_t> bgr(px * 3);
    const auto in_box = [&](int x, int y) { return x > W / 3 + 1 && x < W / 2 + 1 && y > H / 4 + 1 && y < H / 2 + 1; };   // odd edges: blocks straddle them
    size_t holes_in = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            n ^= n >> 15;
            n *= 2246822519u;
            n ^= n >> 13;
            const float z = in_box(x, y) ? 1200.0f : 2000.0f;
            depth[(size_t)y * W + x] = n % 100 < 3 ? 0.0f : z + (float)((n >> 8) % 13) - 6.0f;
            holes_in += n % 100 < 3;
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            c[0] = (uint8_t)((in_box(x, y) ? 200 : 50) + (n >> 12) % 5);
            c[1] = (uint8_t)((in_box(x, y) ? 60 : 120) + (n >> 16) % 5);
            c[2] = (uint8_t)((in_box(x, y) ? 40 : 160) + (n >> 20) % 5);
        }
    float *raw = nullptr, *small = nullptr, *full = nullptr;
    uint8_t *guide = nullptr, *small_guide = nullptr;
    int w = 0, h = 0;
    uint32_t filled = 0, mixed = 0, up_filled = 0;
    size_t between_small = 0, between_full = 0, wrong_side = 0, judged = 0;
    double raw_err = 0.0, small_err = 0.0, full_err = 0.0;
    double Ks[9] = {0};
    try {
        kde_decimate_params p = kde::DepthDecimation::defaultParams();     // factor 2, the lower median, min_valid 1
        p.max_gap = 100.0f;                                                // only counts the blocks on the outline: mixed[]
        kde::DepthDecimation decimate(W, H, 1, p);
        w = decimate.outWidth();
        h = decimate.outHeight();
        const size_t spx = (size_t)w * h;
        if (hipMalloc(&raw, px * sizeof(float)) != hipSuccess || hipMalloc(&small, spx * sizeof(float)) != hipSuccess ||
            hipMalloc(&full, px * sizeof(float)) != hipSuccess || hipMalloc(&guide, px * 3) != hipSuccess ||
            hipMalloc(&small_guide, spx * 3) != hipSuccess)
            return 1;
        if (hipMemcpy(raw, depth.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(guide, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
            return 1;
        decimate.decimate(1, raw, small);
        decimate.decimateColor(1, guide, small_guide);
        filled = decimate.filled_Host()[0];
        mixed = decimate.mixed_Host()[0];
        const double Kfull[9] = {525.0 * W / 640, 0.0, (W - 1) / 2.0, 0.0, 525.0 * W / 640, (H - 1) / 2.0, 0.0, 0.0, 1.0};
        decimate.intrinsics(static_cast<const double*>(Kfull), Ks);        // the camera of the small image
        std::vector<float> low(spx);
        if (hipMemcpy(low.data(), small, spx * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        kde::ref::JointBilateralFilter jbf(w, h);
        jbf.ProcessBatch(1, small, small_guide);                           // a quarter of the pixels
        kde_upsample_params u = kde::GuidedDepthUpsampling::defaultParams();
        u.sigma_color = 10.0f;
        u.max_gap = 100.0f;
        kde::GuidedDepthUpsampling up(w, h, W, H, 1, u);
        up.upsample(1, jbf.getFiltered_Device(), guide, 1, full);
        up_filled = up.filled_Host()[0];
        std::vector<float> back(px);
        if (hipMemcpy(back.data(), full, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) between_small += low[(size_t)y * w + x] > 1250.0f && low[(size_t)y * w + x] < 1950.0f;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t at = (size_t)y * W + x;
                const float z = back[at], truth = in_box(x, y) ? 1200.0f : 2000.0f;
                if (z == 0.0f) continue;
                between_full += z > 1250.0f && z < 1950.0f;
                wrong_side += std::fabs(z - truth) > 100.0f;
                const float zs = low[(size_t)(y / K) * w + x / K];
                if (depth[at] != 0.0f && zs != 0.0f && std::fabs(z - truth) <= 100.0f && std::fabs(zs - truth) <= 100.0f) {
                    raw_err += std::fabs(depth[at] - truth);
                    small_err += std::fabs(zs - truth);
                    full_err += std::fabs(z - truth);
                    ++judged;
                }
            }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(raw);
    (void)hipFree(small);
    (void)hipFree(full);
    (void)hipFree(guide);
    (void)hipFree(small_guide);
    raw_err /= (double)judged;
    small_err /= (double)judged;
    full_err /= (double)judged;
    const size_t spx = (size_t)w * h;
    const bool camera = std::fabs(Ks[2] - ((W - 1) / 2.0 + 0.5) / K + 0.5) < 1e-12 && std::fabs(Ks[0] - 525.0 * W / 640 / K) < 1e-12;
    if (filled < spx * 99 / 100 || filled > spx || mixed == 0 || mixed > (uint32_t)(2 * (w + h)) || between_small != 0 || between_full > px / 100 ||
        wrong_side > px / 100 || up_filled < px * 99 / 100 || !(small_err < raw_err) || !(full_err < raw_err) || !camera) {
        std::fprintf(stderr, "decimate_demo: %u of %zu small pixels filled (%zu dropouts in), %u mixed, %zu / %zu between the surfaces, %zu on the wrong "
                             "side, %u of %zu upsampled, error %.2f -> %.2f -> %.2f mm, camera %s\n",
                     filled, spx, holes_in, mixed, between_small, between_full, wrong_side, up_filled, px, raw_err, small_err, full_err,
                     camera ? "ok" : "wrong");
        return 1;
    }
    std::printf("decimate_demo ok %dx%d -> %dx%d -> %dx%d: %zu dropouts in, %zu small pixels empty, %u blocks on the outline and none of them "
                "between the surfaces (%zu pixels after the filter, which blends along the outline), noise %.2f -> %.2f -> %.2f mm\n",
                W, H, w, h, W, H, holes_in, spx - filled, mixed, between_full, raw_err, small_err, full_err);
    return 0;
}
