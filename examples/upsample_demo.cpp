// upsample_demo.cpp — colour-guided depth upsampling in front of the filters, on the classes of include/kde/kde.hpp:
//   a uint16 depth frame of a quarter of the colour image's size in each direction (what a 320 x 240 ToF head beside a
//   colour camera delivers once it is registered into the colour view) is brought to the colour image's size by
//   kde::GuidedDepthUpsampling with the flying-pixel guard, and the result goes into kde::JointBilateralFilter as it is.
//   Everything stays on the device.
// Usage: upsample_demo [W H] (the colour image's size, multiples of 4).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 640, H = argc > 2 ? std::atoi(argv[2]) : 480;
    const int w = W / 4, h = H / 4;
    if (w < 1 || h < 1) return 1;
    const size_t px = (size_t)W * H, spx = (size_t)w * h;
    std::vector<uint16_t> depth(spx);                      // a wall with a box in front of it, a few dropped samples
    std::vector<uint8_t> bgr(px * 3);                      // the box has a colour of its own
    const auto in_box = [&](int x, int y) { return x > W / 3 && x < W / 2 && y > H / 4 && y < H / 2; };
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            depth[(size_t)y * w + x] = (n % 53 == 0) ? (uint16_t)0 : (uint16_t)(in_box(4 * x + 2, 4 * y + 2) ? 1200 : 2000);
        }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            const unsigned n = ((unsigned)x * 40503u) ^ ((unsigned)y * 2654435761u);
            c[0] = (uint8_t)((in_box(x, y) ? 200 : 50) + (n >> 7) % 5);
            c[1] = (uint8_t)((in_box(x, y) ? 60 : 120) + (n >> 11) % 5);
            c[2] = (uint8_t)((in_box(x, y) ? 40 : 160) + (n >> 17) % 5);
        }
    uint16_t* low = nullptr;
    float* full = nullptr;
    uint8_t* guide = nullptr;
    if (hipMalloc(&low, spx * sizeof(uint16_t)) != hipSuccess || hipMalloc(&full, px * sizeof(float)) != hipSuccess ||
        hipMalloc(&guide, px * 3) != hipSuccess)
        return 1;
    if (hipMemcpy(low, depth.data(), spx * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(guide, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    uint32_t filled = 0;
    size_t flying = 0, wrong_side = 0;
    try {
        kde_upsample_params p = kde::GuidedDepthUpsampling::defaultParams();
        p.sigma_color = 10.0f;                             // the box's colour is far from the wall's
        p.max_gap = 100.0f;                                // no blend across more than 100 mm
        kde::GuidedDepthUpsampling up(w, h, W, H, 1, p);
        up.upsample(1, low, guide, 1, full);               // uint16 in, float out
        filled = up.filled_Host()[0];
        kde::ref::JointBilateralFilter jbf(W, H);
        jbf.ProcessBatch(1, full, guide);                  // depth and colour of one size from here on
        std::vector<float> back(px);
        if (hipMemcpy(back.data(), full, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float z = back[(size_t)y * W + x];
                if (z == 0.0f) continue;
                flying += z > 1250.0f && z < 1950.0f;
                wrong_side += in_box(x, y) ? z > 1600.0f : z < 1600.0f;
            }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(low);
    (void)hipFree(full);
    (void)hipFree(guide);
    if (filled < px * 9 / 10 || filled > px || flying != 0 || wrong_side > px / 100) {
        std::fprintf(stderr, "upsample_demo: %u of %zu pixels got a depth, %zu between the surfaces, %zu on the wrong side of the colour edge\n",
                     filled, px, flying, wrong_side);
        return 1;
    }
    std::printf("upsample_demo ok %dx%d -> %dx%d: %u of %zu pixels got a depth, none between the surfaces, %zu on the wrong side of the colour edge\n",
                w, h, W, H, filled, px, wrong_side);
    return 0;
}
