// undist_demo.cpp — lens undistortion in front of the registration, on the classes of include/kde/kde.hpp:
//   a depth camera and a colour camera that both have barrel distortion (what a ToF head beside an RGB camera, calibrated with
//   OpenCV, delivers) are brought into pinhole views by two kde::LensUndistortion objects -- the uint16 depth with the guarded
//   bilinear rule, the colour image with the bilinear one -- and the undistorted depth is then warped into the colour camera's
//   view by kde::DepthRegistration.  Everything stays on the device.
// Usage: undist_demo [W H].
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 640, H = argc > 2 ? std::atoi(argv[2]) : 480;
    const size_t px = (size_t)W * H;
    std::vector<uint16_t> depth(px);                       // the sensor's own format: a wall with a box in front of it
    std::vector<uint8_t> bgr(px * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const bool box = x > W / 3 && x < W / 2 && y > H / 4 && y < H / 2;
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            depth[(size_t)y * W + x] = (n % 97 == 0) ? (uint16_t)0 : (uint16_t)((box ? 1200 : 2000) + (n >> 9) % 3);
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            const int check = ((x / 16) + (y / 16)) & 1;
            c[0] = (uint8_t)(check ? 220 : 40);
            c[1] = (uint8_t)(90 + 80 * y / H);
            c[2] = (uint8_t)(box ? 200 : 60);
        }
    uint16_t* raw = nullptr;
    float *flat = nullptr, *registered = nullptr;
    uint8_t *dbgr = nullptr, *flat_bgr = nullptr;
    if (hipMalloc(&raw, px * sizeof(uint16_t)) != hipSuccess || hipMalloc(&flat, px * sizeof(float)) != hipSuccess ||
        hipMalloc(&registered, px * sizeof(float)) != hipSuccess || hipMalloc(&dbgr, px * 3) != hipSuccess ||
        hipMalloc(&flat_bgr, px * 3) != hipSuccess)
        return 1;
    if (hipMemcpy(raw, depth.data(), px * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dbgr, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    const double fd = 575.8 * W / 640.0, fc = 1.02 * fd;
    const kde::Mat33d Kd{{fd, 0.0, W / 2.0 - 0.4, 0.0, fd, H / 2.0 + 0.3, 0.0, 0.0, 1.0}};
    const kde::Mat33d Kc{{fc, 0.0, W / 2.0 + 0.7, 0.0, fc, H / 2.0 - 0.6, 0.0, 0.0, 1.0}};
    const double dist_d[8] = {-0.12, 0.03, 0.0008, -0.0005, 0.0, 0.0, 0.0, 0.0};       // k1, k2, p1, p2, k3, k4, k5, k6
    const double dist_c[8] = {-0.21, 0.08, -0.0004, 0.0006, -0.01, 0.0, 0.0, 0.0};
    const double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    const double t[3] = {25.0, 0.0, 0.0};
    uint32_t kept = 0, filled = 0;
    size_t coloured = 0;
    try {
        kde_undist_params p = kde::LensUndistortion::defaultParams();
        p.depth_interp = 1;                                // blend where the four taps agree ...
        p.max_gap = 50.0f;                                 // ... to 50 mm; never across the box's edge or a hole
        kde::LensUndistortion depth_view(W, H, W, H, 1, p);
        depth_view.setCalibration(Kd, dist_d);             // the pinhole view keeps Kd
        kde::LensUndistortion color_view(W, H, W, H);
        color_view.setCalibration(Kc, dist_c);
        depth_view.undistortDepth(1, raw, flat);           // uint16 in, float out
        color_view.undistortColor(1, dbgr, 1, flat_bgr);
        kept = depth_view.filled_Host()[0];
        kde::DepthRegistration reg(W, H, W, H, 1);
        reg.setCalibration(Kd, Kc, R, t);                  // two pinhole cameras from here on
        reg.registerDepth(1, flat, registered);
        filled = reg.filled_Host()[0];
        std::vector<uint8_t> back(px * 3);
        if (hipMemcpy(back.data(), flat_bgr, px * 3, hipMemcpyDeviceToHost) != hipSuccess) return 1;
        for (size_t i = 0; i < px; ++i) coloured += (back[3 * i] | back[3 * i + 1] | back[3 * i + 2]) != 0;
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(raw);
    (void)hipFree(flat);
    (void)hipFree(registered);
    (void)hipFree(dbgr);
    (void)hipFree(flat_bgr);
    if (kept < px * 8 / 10 || kept > px || filled < px * 7 / 10 || filled > px || coloured < px * 9 / 10) {
        std::fprintf(stderr, "undist_demo: %u of %zu pixels got a depth, %u registered, %zu coloured\n", kept, px, filled, coloured);
        return 1;
    }
    std::printf("undist_demo ok %dx%d: %u of %zu pixels got a depth, %u registered, %zu coloured\n", W, H, kept, px, filled, coloured);
    return 0;
}
