// normals_demo.cpp — kde::NormalMapGenerator through include/kde/kde.hpp, as the reference's KinectDepthEnhancement
// drives it (setNormalEstimationMethods(CM), generateNormalMap(points), getNormalMap()).
// Usage: normals_demo OUT_DIR [W H]. Builds a frame of points in millimetres (a tilted plane with a box in front of it and
// a hole), runs CM then BILATERAL, and writes points.f32, cm.f32 and bilateral.f32 (W*H*3 floats each) into OUT_DIR.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/kde/kde.hpp"

static bool save(const std::string& path, const std::vector<float>& v)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s OUT_DIR [W H]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int W = argc > 3 ? std::atoi(argv[2]) : 160, H = argc > 3 ? std::atoi(argv[3]) : 120;
    const size_t px = (size_t)W * H;
    std::vector<float> pts(px * 3);
    const float f = 575.8f * W / 640.0f;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float z = 2000.0f + 1.5f * x - 0.8f * y;
            if (x > W / 3 && x < W / 2 && y > H / 4 && y < H / 2) z = 1200.0f;   // a box in front
            if (x > 2 * W / 3 && x < 2 * W / 3 + 6 && y > H / 2 && y < H / 2 + 6) z = 0.0f;   // a hole
            float* p = &pts[((size_t)y * W + x) * 3];
            p[0] = (x - W / 2) / f * z;
            p[1] = (H / 2 - y) / f * z;
            p[2] = z;
        }
    float3* dpts = nullptr;
    if (hipMalloc(&dpts, px * sizeof(float3)) != hipSuccess) return 1;
    if (hipMemcpy(dpts, pts.data(), px * sizeof(float3), hipMemcpyHostToDevice) != hipSuccess) return 1;
    std::vector<float> cm(px * 3), bil(px * 3);
    try {
        NormalMapGenerator nmg(W, H);
        nmg.setNormalEstimationMethods(NormalMapGenerator::CM);
        nmg.generateNormalMap(dpts);
        if (hipMemcpy(cm.data(), nmg.getNormalMap(), px * sizeof(float3), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        nmg.setNormalEstimationMethods(NormalMapGenerator::BILATERAL);
        nmg.generateNormalMap(dpts);
        if (hipMemcpy(bil.data(), nmg.getNormalMap(), px * sizeof(float3), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        const kde::HostImage8UC3& img = nmg.getNormalImg();
        std::printf("normal image %dx%d, first pixel %d %d %d\n", img.cols, img.rows, img.at(0, 0)[0], img.at(0, 0)[1],
                    img.at(0, 0)[2]);
        bool threw = false;
        try {
            nmg.setNormalEstimationMethods(NormalMapGenerator::SDC);
        } catch (const kde::Error& e) {
            threw = e.code() == KDE_ERR_UNSUPPORTED;
        }
        if (!threw) {
            std::fprintf(stderr, "SDC was accepted\n");
            return 1;
        }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(dpts);
    if (!save(dir + "/points.f32", pts) || !save(dir + "/cm.f32", cm) || !save(dir + "/bilateral.f32", bil)) return 1;
    std::printf("normals_demo ok %dx%d\n", W, H);
    return 0;
}
