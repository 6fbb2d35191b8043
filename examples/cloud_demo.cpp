// cloud_demo.cpp — the output step of the reference's main.cpp on the classes of include/kde/kde.hpp:
//   KinectDepthEnhancement::Process on one synthetic frame (main.cpp:200-202), then kde::PointCloudXYZRGB turns the enhanced
//   points and the colour image into the coloured cloud of main.cpp:211-300 (valid pixels only, metres, z negated, packed
//   rgb) on the device, and kde::writePcd saves it as a binary PCD v0.7 file.
// Usage: cloud_demo [W H [out.pcd]].  The scene is kde_demo's.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"
#include "../include/kde/pcd_io.hpp"

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 640, H = argc > 2 ? std::atoi(argv[2]) : 480;
    const char* path = argc > 3 ? argv[3] : "cloud_demo.pcd";
    const int rows = 15, cols = 20;
    const size_t px = (size_t)W * H;
    std::vector<float> depth(px);
    std::vector<uint8_t> bgr(px * 3);
    size_t holes = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float z = 2000.0f + 1.5f * x * 640.0f / W - 0.8f * y * 480.0f / H;
            const bool box = x > W / 3 && x < W / 2 && y > H / 4 && y < H / 2;
            if (box) z = 1200.0f;
            const bool hole = x > 2 * W / 3 && x < 2 * W / 3 + W / 40 && y > H / 2 && y < H / 2 + H / 30;
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            depth[(size_t)y * W + x] = hole ? 0.0f : z + (float)((n >> 9) % 7) - 3.0f;
            holes += hole;
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            c[0] = (uint8_t)((box ? 40 : 150 + 60 * x / W) + (n >> 7) % 5);
            c[1] = (uint8_t)((box ? 170 : 90 + 80 * y / H) + (n >> 11) % 5);
            c[2] = (uint8_t)((box ? 200 : 60) + (n >> 17) % 5);
        }
    float* inputDepth_Device = nullptr;
    uint8_t* dbgr = nullptr;
    if (hipMalloc(&inputDepth_Device, px * sizeof(float)) != hipSuccess || hipMalloc(&dbgr, px * 3) != hipSuccess) return 1;
    if (hipMemcpy(inputDepth_Device, depth.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||      // main.cpp:160
        hipMemcpy(dbgr, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)                                   // :163
        return 1;
    const double f = 575.8 * W / 640.0;
    const kde::Mat33d K{{f, 0.0, W / 2.0, 0.0, f, H / 2.0, 0.0, 0.0, 1.0}};
    const kde::GpuImage8UC3 Color_Device{dbgr, H, W, (size_t)W * 3};
    uint32_t count = 0, input_count = 0;
    kde_cloud_point first{}, last{};
    try {
        KinectDepthEnhancement KDE(W, H);                                             // main.cpp:77-78
        KDE.SetParametor(rows, cols, K);
        KDE.Process(inputDepth_Device, Color_Device);                                 // :200
        kde::PointCloudXYZRGB cloud(W, H);
        cloud.setCamera(K);
        cloud.build(1, kde::MeanError3D::source(inputDepth_Device), dbgr);            // :233-237, the input as a depth map
        input_count = cloud.counts_Host()[0];
        cloud.build(1, kde::MeanError3D::source(KDE.getOptimizedPoints_Device()), dbgr);   // :202, :286-290
        const uint64_t* offsets = nullptr;
        const kde_cloud_point* points = cloud.points_Host(&offsets);
        count = (uint32_t)offsets[1];
        if (count != cloud.counts_Host()[0] || count == 0) {
            std::fprintf(stderr, "cloud_demo: %u records for %u valid pixels\n", count, cloud.counts_Host()[0]);
            return 1;
        }
        first = points[0];
        last = points[count - 1];
        for (uint32_t i = 0; i < count; ++i)
            if (!(points[i].z < -0.05f && points[i].z > -15.0f) || (points[i].rgb >> 24) != 0) {
                std::fprintf(stderr, "cloud_demo: record %u is (%g, %g, %g, %08x)\n", i, points[i].x, points[i].y, points[i].z, points[i].rgb);
                return 1;
            }
        if (!kde::writePcd(path, points, count)) {                                    // result->points as a file
            std::fprintf(stderr, "cloud_demo: cannot write %s\n", path);
            return 1;
        }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(inputDepth_Device);
    (void)hipFree(dbgr);
    if (input_count != px - holes) {
        std::fprintf(stderr, "cloud_demo: the input has %zu valid pixels, its cloud %u points\n", px - holes, input_count);
        return 1;
    }
    std::printf("first (%f, %f, %f) #%06x\nlast  (%f, %f, %f) #%06x\n", first.x, first.y, first.z, first.rgb, last.x, last.y, last.z, last.rgb);
    std::printf("cloud_demo ok %dx%d input %u result %u points -> %s\n", W, H, input_count, count, path);
    return 0;
}
