// reg_demo.cpp — registration in front of the reference's pipeline, on the classes of include/kde/kde.hpp:
//   a synthetic depth frame as a depth camera 25 mm beside the colour camera sees it (what a sensor without OpenNI's
//   SetViewPoint delivers, Kinect.cpp:71-75) is warped into the colour camera's view by kde::DepthRegistration, and the float
//   result goes straight into KinectDepthEnhancement::ProcessBatch (main.cpp:198-202), both on the device.
// Usage: reg_demo [W H].  The scene is kde_demo's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 640, H = argc > 2 ? std::atoi(argv[2]) : 480;
    const int rows = 15, cols = 20;
    const size_t px = (size_t)W * H;
    std::vector<uint16_t> depth(px);                       // the sensor's own format
    std::vector<uint8_t> bgr(px * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float z = 2000.0f + 1.5f * x * 640.0f / W - 0.8f * y * 480.0f / H;
            const bool box = x > W / 3 && x < W / 2 && y > H / 4 && y < H / 2;
            if (box) z = 1200.0f;
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            depth[(size_t)y * W + x] = (uint16_t)(z + (float)((n >> 9) % 7) - 3.0f);
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            c[0] = (uint8_t)((box ? 40 : 150 + 60 * x / W) + (n >> 7) % 5);
            c[1] = (uint8_t)((box ? 170 : 90 + 80 * y / H) + (n >> 11) % 5);
            c[2] = (uint8_t)((box ? 200 : 60) + (n >> 17) % 5);
        }
    uint16_t* raw = nullptr;
    float* registered = nullptr;
    uint8_t* dbgr = nullptr;
    if (hipMalloc(&raw, px * sizeof(uint16_t)) != hipSuccess || hipMalloc(&registered, px * sizeof(float)) != hipSuccess ||
        hipMalloc(&dbgr, px * 3) != hipSuccess)
        return 1;
    if (hipMemcpy(raw, depth.data(), px * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dbgr, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    const double fd = 575.8 * W / 640.0, fc = 1.02 * fd;   // two cameras: focal lengths 2 % apart, principal points no integers
    const kde::Mat33d Kd{{fd, 0.0, W / 2.0 - 0.4, 0.0, fd, H / 2.0 + 0.3, 0.0, 0.0, 1.0}};
    const kde::Mat33d Kc{{fc, 0.0, W / 2.0 + 0.7, 0.0, fc, H / 2.0 - 0.6, 0.0, 0.0, 1.0}};
    const double a = 1.0 * 3.14159265358979323846 / 180.0;
    const double R[9] = {std::cos(a), 0.0, std::sin(a), 0.0, 1.0, 0.0, -std::sin(a), 0.0, std::cos(a)};
    const double t[3] = {25.0, 0.0, 0.0};                  // the Kinect's baseline
    uint32_t filled = 0;
    size_t enhanced = 0;
    try {
        kde_reg_params p = kde::DepthRegistration::defaultParams();
        p.max_splat = 2;                                   // fc > fd: a source pixel is a little more than one target pixel wide
        kde::DepthRegistration reg(W, H, W, H, 1, p);
        reg.setCalibration(Kd, Kc, R, t);
        reg.registerDepth(1, raw, registered);             // uint16 in, float out: what Process takes
        filled = reg.filled_Host()[0];
        KinectDepthEnhancement KDE(W, H, 1);               // main.cpp:77-78
        KDE.SetParametor(rows, cols, Kc);                  // the registered depth is seen by the colour camera
        KDE.ProcessBatch(1, registered, dbgr);             // :200
        const float3* pts = KDE.getOptimizedPoints_Host();
        for (size_t i = 0; i < px; ++i) enhanced += pts[i].z > 50.0f && pts[i].z < 15000.0f;
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(raw);
    (void)hipFree(registered);
    (void)hipFree(dbgr);
    if (filled < px * 8 / 10 || filled > px || enhanced < px / 2) {
        std::fprintf(stderr, "reg_demo: %u of %zu target pixels reached, %zu enhanced\n", filled, px, enhanced);
        return 1;
    }
    std::printf("reg_demo ok %dx%d: %u of %zu target pixels reached, %zu enhanced points\n", W, H, filled, px, enhanced);
    return 0;
}
