// speckle_demo.cpp — wrong depth taken away in front of the hole filler, on the classes of include/kde/kde.hpp:
//   a uint16 depth frame of a wall with a box in front of it carries what a time-of-flight sensor's frame carries -- flying pixels
//   half way between the two surfaces along the box's left and right edges -- and what a Kinect's carries: a shadow band of 8
//   pixels left of the box with a few speckles of random depth inside it.  kde::DepthSpeckleFilter labels the frame's connected
//   components and sets those below 64 pixels to 0 (in place); kde::DepthHoleFilling then closes the band and the holes the
//   flying pixels left, from the surfaces and not from the outliers.  Everything stays on the device.
// Usage: speckle_demo [W H].
#include <hip/hip_runtime.h>

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
    const auto in_box = [&](int x, int y) { return x >= bx0 && x < bx1 && y >= by0 && y < by1; };
    const auto in_shadow = [&](int x, int y) { return x >= bx0 - 8 && x < bx0 && y >= by0 && y < by1; };
    std::vector<uint16_t> depth(px);
    std::vector<uint8_t> bgr(px * 3);
    size_t outliers = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            uint16_t d = in_box(x, y) ? 1200 : 2000;
            if (in_shadow(x, y)) d = (n >> 3) % 16 == 0 ? (uint16_t)(600 + (n >> 9) % 500) : (uint16_t)0;           // speckles in the band, nearer than either surface
            else if (y >= by0 && y < by1 && (x == bx0 || x == bx1 - 1) && (n >> 5) % 2 == 0) d = 1600;              // flying pixels
            outliers += d != 0 && d != 1200 && d != 2000;
            depth[(size_t)y * W + x] = d;
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            c[0] = (uint8_t)((in_box(x, y) ? 200 : 50) + (n >> 7) % 5);
            c[1] = (uint8_t)((in_box(x, y) ? 60 : 120) + (n >> 11) % 5);
            c[2] = (uint8_t)((in_box(x, y) ? 40 : 160) + (n >> 17) % 5);
        }
    uint16_t* raw = nullptr;
    float* full = nullptr;
    uint8_t* guide = nullptr;
    int32_t* labels = nullptr;
    if (hipMalloc(&raw, px * sizeof(uint16_t)) != hipSuccess || hipMalloc(&full, px * sizeof(float)) != hipSuccess ||
        hipMalloc(&guide, px * 3) != hipSuccess || hipMalloc(&labels, px * sizeof(int32_t)) != hipSuccess)
        return 1;
    if (hipMemcpy(raw, depth.data(), px * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(guide, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    uint32_t removed = 0, components = 0, capped = 0, remaining = 0;
    size_t between = 0, wrong_side = 0;
    try {
        kde::DepthSpeckleFilter speckle(W, H);                             // 64 pixels, 10 mm + 2 %, 4-connected
        speckle.filter(1, raw, raw, labels);                               // uint16, in place
        removed = speckle.removed_Host()[0];
        components = speckle.components_Host()[0];
        capped = speckle.capped_Host()[0];
        kde_holefill_params p = kde::DepthHoleFilling::defaultParams();
        p.sigma_color = 10.0f;
        p.max_gap = 100.0f;
        p.gap_rule = 1;
        kde::DepthHoleFilling fill(W, H, 1, p);
        fill.fill(1, raw, guide, 1, full);
        remaining = fill.remaining_Host()[0];
        std::vector<float> back(px);
        if (hipMemcpy(back.data(), full, px * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const float z = back[(size_t)y * W + x];
                if (z == 0.0f) continue;
                between += z > 1250.0f && z < 1950.0f;
                wrong_side += in_box(x, y) ? z > 1600.0f : z < 1600.0f;
            }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(raw);
    (void)hipFree(full);
    (void)hipFree(guide);
    (void)hipFree(labels);
    if (removed != outliers || components != 2 || capped != 0 || remaining != 0 || between != 0 || wrong_side != 0) {
        std::fprintf(stderr, "speckle_demo: %u of %zu outliers removed, %u components kept, capped %u, %u holes remain, %zu between the "
                             "surfaces, %zu on the wrong side of the colour edge\n",
                     removed, outliers, components, capped, remaining, between, wrong_side);
        return 1;
    }
    std::printf("speckle_demo ok %dx%d: %u outliers removed, the wall and the box kept, every hole closed from its surface\n", W, H, removed);
    return 0;
}
