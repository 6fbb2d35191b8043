// holefill_demo.cpp — colour-guided filling of depth holes in front of the filters, on the classes of include/kde/kde.hpp:
//   a uint16 depth frame of a wall with a box in front of it carries what a Kinect's frame carries -- a shadow band of 8 pixels
//   left of the box and a few dropped samples -- and a hole too wide to close.  kde::DepthHoleFilling closes the band from the
//   wall (gap_rule 1: a shadow belongs to the background) and the dropped samples from their surface, leaves the middle of the
//   wide hole alone, and the result goes into kde::JointBilateralFilter as it is.  Everything stays on the device.
// Usage: holefill_demo [W H].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 640, H = argc > 2 ? std::atoi(argv[2]) : 480;
    if (W < 160 || H < 120) return 1;
    const size_t px = (size_t)W * H;
    const int bx0 = W / 3, bx1 = W / 2, by0 = H / 4, by1 = H / 2;          // the box
    const int hx0 = 3 * W / 4 - 30, hx1 = 3 * W / 4 + 30, hy0 = 3 * H / 4 - 30, hy1 = 3 * H / 4 + 30;     // a 60 x 60 hole in the wall
    const auto in_box = [&](int x, int y) { return x >= bx0 && x < bx1 && y >= by0 && y < by1; };
    const auto in_shadow = [&](int x, int y) { return x >= bx0 - 8 && x < bx0 && y >= by0 && y < by1; };
    const auto in_wide = [&](int x, int y) { return x >= hx0 && x < hx1 && y >= hy0 && y < hy1; };
    std::vector<uint16_t> depth(px);
    std::vector<uint8_t> bgr(px * 3);
    size_t holes = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            const bool hole = in_shadow(x, y) || in_wide(x, y) || n % 97 == 0;
            depth[(size_t)y * W + x] = hole ? (uint16_t)0 : (uint16_t)(in_box(x, y) ? 1200 : 2000);
            holes += hole;
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            c[0] = (uint8_t)((in_box(x, y) ? 200 : 50) + (n >> 7) % 5);
            c[1] = (uint8_t)((in_box(x, y) ? 60 : 120) + (n >> 11) % 5);
            c[2] = (uint8_t)((in_box(x, y) ? 40 : 160) + (n >> 17) % 5);
        }
    uint16_t* raw = nullptr;
    float* full = nullptr;
    uint8_t* guide = nullptr;
    uint8_t* pass_of = nullptr;
    if (hipMalloc(&raw, px * sizeof(uint16_t)) != hipSuccess || hipMalloc(&full, px * sizeof(float)) != hipSuccess ||
        hipMalloc(&guide, px * 3) != hipSuccess || hipMalloc(&pass_of, px) != hipSuccess)
        return 1;
    if (hipMemcpy(raw, depth.data(), px * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(guide, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    uint32_t filled = 0, remaining = 0;
    int k = 0;
    size_t flying = 0, wrong_side = 0, shadow_on_box = 0, middle_filled = 0;
    try {
        kde_holefill_params p = kde::DepthHoleFilling::defaultParams();    // r = 2, 8 passes: a fill reaches 16 pixels
        p.sigma_color = 10.0f;                                             // the box's colour is far from the wall's
        p.max_gap = 100.0f;                                                // no blend across more than 100 mm,
        p.gap_rule = 1;                                                    // and where two surfaces are in reach, the far one
        kde::DepthHoleFilling fill(W, H, 1, p);
        k = fill.passesPerLaunch();
        fill.fill(1, raw, guide, 1, full, pass_of);                        // uint16 in, float out
        filled = fill.filled_Host()[0];
        remaining = fill.remaining_Host()[0];
        kde::ref::JointBilateralFilter jbf(W, H);
        jbf.ProcessBatch(1, full, guide);                                  // holes closed from here on
        std::vector<float> back(px);
        std::vector<uint8_t> pass(px);
        if (hipMemcpy(back.data(), full, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(pass.data(), pass_of, px, hipMemcpyDeviceToHost) != hipSuccess)
            return 1;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float z = back[(size_t)y * W + x];
                if (in_wide(x, y) && x >= hx0 + 20 && x < hx1 - 20 && y >= hy0 + 20 && y < hy1 - 20) middle_filled += z != 0.0f || pass[(size_t)y * W + x] != 255;
                if (z == 0.0f) continue;
                flying += z > 1250.0f && z < 1950.0f;
                wrong_side += in_box(x, y) ? z > 1600.0f : z < 1600.0f;
                shadow_on_box += in_shadow(x, y) && z < 1600.0f;
            }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(raw);
    (void)hipFree(full);
    (void)hipFree(guide);
    (void)hipFree(pass_of);
    if (filled + remaining != holes || remaining == 0 || remaining > 60 * 60 || flying != 0 || wrong_side != 0 || shadow_on_box != 0 ||
        middle_filled != 0) {
        std::fprintf(stderr, "holefill_demo: %u of %zu holes filled, %u remain, %zu between the surfaces, %zu on the wrong side of the colour "
                             "edge, %zu shadow pixels on the box, %zu filled beyond reach\n",
                     filled, holes, remaining, flying, wrong_side, shadow_on_box, middle_filled);
        return 1;
    }
    std::printf("holefill_demo ok %dx%d, %d passes per launch: %u of %zu holes filled, %u remain in the middle of the 60 x 60 hole, none "
                "between the surfaces, the shadow band on the wall\n", W, H, k, filled, holes, remaining);
    return 0;
}
