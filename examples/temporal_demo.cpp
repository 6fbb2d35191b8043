// temporal_demo.cpp — a live depth sequence through the front end, frame by frame, on the classes of include/kde/kde.hpp:
//   DepthSpeckleFilter -> DepthTemporalFilter -> DepthHoleFilling -> JointBilateralFilter
//   The scene is a wall at 2000 mm with a box at 1200 mm that moves 4 pixels per frame; every frame carries +-6 mm of depth
//   noise and 3 % dropouts, drawn anew.  The temporal filter halves the noise of the wall, holds the wall over the dropouts and,
//   because the guide shows the box arriving and leaving, keeps no trace of the box where it was: a dropout in the box's trail
//   is a hole that the hole filler then closes from the wall, not a ghost of the box.  Everything stays on the device.
// Usage: temporal_demo [W H].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"

static unsigned hash3(unsigned x, unsigned y, unsigned t)
{
    unsigned n = x * 2654435761u ^ y * 40503u ^ t * 2246822519u;
    n ^= n >> 15;
    n *= 2246822519u;
    n ^= n >> 13;
    return n;
}

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 320, H = argc > 2 ? std::atoi(argv[2]) : 240, N = 12;
    if (W < 160 || H < 120) return 1;
    const size_t px = (size_t)W * H;
    const int bw = W / 5, bh = H / 3, by0 = H / 3;
    std::vector<float> depth(px), back(px), filled(px);
    std::vector<uint8_t> bgr(px * 3);
    float *raw = nullptr, *smooth = nullptr, *full = nullptr;
    uint8_t* guide = nullptr;
    if (hipMalloc(&raw, px * sizeof(float)) != hipSuccess || hipMalloc(&smooth, px * sizeof(float)) != hipSuccess ||
        hipMalloc(&full, px * sizeof(float)) != hipSuccess || hipMalloc(&guide, px * 3) != hipSuccess)
        return 1;
    double raw_err = 0.0, smooth_err = 0.0;
    size_t wall = 0, ghosts = 0, holes_in = 0, holes_kept = 0, wrong = 0;
    uint32_t remaining = 0, held = 0, changed = 0;
    try {
        kde::DepthSpeckleFilter speckle(W, H);
        kde::DepthTemporalFilter temporal(W, H);                          // alpha 0.4, 10 mm + 2 %, 3 of 8, colour step 48
        kde::DepthHoleFilling fill(W, H);
        kde::ref::JointBilateralFilter jbf(W, H);
        for (int t = 0; t < N; ++t) {
            const int bx0 = W / 8 + 4 * t, bx1 = bx0 + bw;
            const auto in_box = [&](int x, int y) { return x >= bx0 && x < bx1 && y >= by0 && y < by0 + bh; };
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const unsigned n = hash3((unsigned)x, (unsigned)y, (unsigned)t);
                    const float z = in_box(x, y) ? 1200.0f : 2000.0f;
                    depth[(size_t)y * W + x] = n % 100 < 3 ? 0.0f : z + (float)((n >> 8) % 13) - 6.0f;
                    uint8_t* c = &bgr[((size_t)y * W + x) * 3];
                    c[0] = (uint8_t)((in_box(x, y) ? 200 : 50) + (n >> 12) % 5);
                    c[1] = (uint8_t)((in_box(x, y) ? 60 : 120) + (n >> 16) % 5);
                    c[2] = (uint8_t)((in_box(x, y) ? 40 : 160) + (n >> 20) % 5);
                }
            if (hipMemcpy(raw, depth.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(guide, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
                return 1;
            speckle.filter(1, raw, raw);                                  // in place
            temporal.filter(1, raw, guide, smooth);                      // the next frame of the sequence
            fill.fill(1, smooth, guide, 1, full);
            jbf.ProcessBatch(1, full, guide);
            held += temporal.held_Host()[0];
            changed += temporal.changed_Host()[0];
            if (t < N - 4) continue;                                      // judged on the last frames, when the state has settled
            remaining += fill.remaining_Host()[0];
            if (hipMemcpy(back.data(), smooth, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(filled.data(), full, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)
                return 1;
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const size_t at = (size_t)y * W + x;
                    const bool box = in_box(x, y);
                    const float z = back[at], truth = box ? 1200.0f : 2000.0f;
                    holes_in += depth[at] == 0.0f;
                    holes_kept += z == 0.0f;
                    ghosts += !box && z != 0.0f && std::fabs(z - 1200.0f) < 100.0f;
                    wrong += std::fabs(filled[at] - truth) > 100.0f;
                    if (!box && depth[at] != 0.0f && z != 0.0f && (x < W / 8 || x >= bx1 + 8)) {      // the wall the box never covered
                        raw_err += std::fabs(depth[at] - truth);
                        smooth_err += std::fabs(z - truth);
                        ++wall;
                    }
                }
        }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(raw);
    (void)hipFree(smooth);
    (void)hipFree(full);
    (void)hipFree(guide);
    raw_err /= (double)wall;
    smooth_err /= (double)wall;
    if (!(smooth_err < 0.7 * raw_err) || ghosts != 0 || held == 0 || changed == 0 || holes_kept * 4 > holes_in || remaining != 0 || wrong != 0) {
        std::fprintf(stderr, "temporal_demo: wall error %.2f -> %.2f mm, %zu ghosts, held %u, changed %u, %zu of %zu holes left by the temporal "
                             "filter, %u after the fill, %zu pixels on the wrong surface\n",
                     raw_err, smooth_err, ghosts, held, changed, holes_kept, holes_in, remaining, wrong);
        return 1;
    }
    std::printf("temporal_demo ok %dx%d x %d frames: wall noise %.2f -> %.2f mm, %u dropouts held, no ghost of the moving box, every hole closed\n",
                W, H, N, raw_err, smooth_err, held);
    return 0;
}
