// compare_demo.cpp — the comparison of the reference's main.cpp on the classes of include/kde/kde.hpp, with the quality
// figure computed on the device:
//   INPUT, JointBilateralFilter, MarkovRandomField, RegionGrowingBilateralFilter and KinectDepthEnhancement on one frame
//   (main.cpp:159-202), then kde::MeanError3D compares the five results with the averaged depth in one call and the five
//   `error` lines of main.cpp:303-308 are printed.
// Usage: compare_demo [W H].  The scene is kde_demo's; the "input" is that scene with a deterministic +-3 mm disturbance, the
// "averaged depth" the scene itself.  The filtered depth maps go in as depth-map sources (the cloud projectiveToReal makes of
// them, main.cpp:182, :189, :196), the enhanced cloud as it is (:202).
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
    std::vector<float> averaged(px), depth(px);
    std::vector<uint8_t> bgr(px * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float z = 2000.0f + 1.5f * x * 640.0f / W - 0.8f * y * 480.0f / H;
            const bool box = x > W / 3 && x < W / 2 && y > H / 4 && y < H / 2;
            if (box) z = 1200.0f;
            const bool hole = x > 2 * W / 3 && x < 2 * W / 3 + W / 40 && y > H / 2 && y < H / 2 + H / 30;
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            averaged[(size_t)y * W + x] = hole ? 0.0f : z;
            depth[(size_t)y * W + x] = hole ? 0.0f : z + (float)((n >> 9) % 7) - 3.0f;
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            c[0] = (uint8_t)((box ? 40 : 150 + 60 * x / W) + (n >> 7) % 5);
            c[1] = (uint8_t)((box ? 170 : 90 + 80 * y / H) + (n >> 11) % 5);
            c[2] = (uint8_t)((box ? 200 : 60) + (n >> 17) % 5);
        }
    float *inputDepth_Device = nullptr, *bufferDepth_Device = nullptr;
    float3* inputPoints_Device = nullptr;
    uint8_t* dbgr = nullptr;
    if (hipMalloc(&inputDepth_Device, px * sizeof(float)) != hipSuccess || hipMalloc(&bufferDepth_Device, px * sizeof(float)) != hipSuccess ||
        hipMalloc(&inputPoints_Device, px * sizeof(float3)) != hipSuccess || hipMalloc(&dbgr, px * 3) != hipSuccess)
        return 1;
    if (hipMemcpy(inputDepth_Device, depth.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||      // main.cpp:160
        hipMemcpy(bufferDepth_Device, averaged.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||  // :162
        hipMemcpy(dbgr, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)                                   // :163
        return 1;
    const double f = 575.8 * W / 640.0;
    const kde::Mat33d K{{f, 0.0, W / 2.0, 0.0, f, H / 2.0, 0.0, 0.0, 1.0}};
    const kde::GpuImage8UC3 Color_Device{dbgr, H, W, (size_t)W * 3};
    const char* names[5] = {"input", "jbf", "mrf", "rgbf", "result"};
    kde_error3d_result table[5];
    try {
        JointBilateralFilter JBF(W, H);                                               // main.cpp:67
        MarkovRandomField MRF(W, H);                                                  // :69
        DimensionConvertor convertor;                                                 // :71-72
        convertor.setCameraParameters(K, W, H);
        RegionGrowingBilateralFilter RGBF(W, H);                                      // :74-75
        RGBF.SetParametor(rows, cols, K);
        KinectDepthEnhancement KDE(W, H);                                             // :77-78
        KDE.SetParametor(rows, cols, K);
        convertor.projectiveToReal(inputDepth_Device, inputPoints_Device);           // :168
        JBF.Process(inputDepth_Device, Color_Device);                                 // :179
        MRF.Process(inputDepth_Device, Color_Device);                                 // :186
        RGBF.Process(inputDepth_Device, inputPoints_Device, Color_Device);            // :193
        KDE.Process(inputDepth_Device, Color_Device);                                 // :200
        kde::MeanError3D error(W, H, 1, 5);
        error.setCamera(K);
        const kde_error3d_source candidates[5] = {
            kde::MeanError3D::source(inputPoints_Device),                             // :171
            kde::MeanError3D::source(JBF.getFiltered_Device()),                       // :182
            kde::MeanError3D::source(MRF.getFiltered_Device()),                       // :189
            kde::MeanError3D::source(RGBF.getRefinedDepth_Device()),                  // :196
            kde::MeanError3D::source(KDE.getOptimizedPoints_Device()),                // :202
        };
        error.compare(1, 5, candidates, kde::MeanError3D::source(bufferDepth_Device));   // :175, :220-301
        const kde_error3d_result* r = error.results_Host();
        for (int i = 0; i < 5; ++i) table[i] = r[i];
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(inputDepth_Device);
    (void)hipFree(bufferDepth_Device);
    (void)hipFree(inputPoints_Device);
    (void)hipFree(dbgr);
    std::printf("error \n");                                                          // main.cpp:303-308
    for (int i = 0; i < 5; ++i) std::printf("%s %f\n", names[i], table[i].mean);
    for (int i = 0; i < 5; ++i)
        if (table[i].count < px / 2 || !std::isfinite(table[i].mean)) {
            std::fprintf(stderr, "%s: %u valid pixels of %zu\n", names[i], table[i].count, px);
            return 1;
        }
    std::printf("compare_demo ok %dx%d valid %u %u %u %u %u\n", W, H, table[0].count, table[1].count, table[2].count, table[3].count,
                table[4].count);
    return 0;
}
