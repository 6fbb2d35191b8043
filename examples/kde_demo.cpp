// kde_demo.cpp — the reference's "PROPOSED" method (main.cpp:198-202) on the classes of include/kde/kde.hpp:
//   KinectDepthEnhancement KDE(W, H); KDE.SetParametor(rows, cols, K); KDE.Process(depth_device, color_device);
//   KDE.getOptimizedPoints_Host()
// Usage: kde_demo OUT_DIR [W H].  The scene is les_demo's.  Writes the two inputs of Process as raw little-endian arrays
// (kde_in_depth.bin float32 [H][W], kde_in_bgr.bin uint8 [H][W][3]) so that another binding can repeat the call, and the
// enhanced cloud as kde_optimized.bin (float32 [H][W][3]); prints the number of merged regions, the number of pixels with a
// valid enhanced depth and the CRC-32 of the enhanced cloud.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../include/kde/kde.hpp"

static bool save_raw(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
    return std::fclose(f) == 0 && ok;
}

static uint32_t crc32_of(const void* data, size_t bytes)   // the CRC-32 of zlib (reflected 0xEDB88320)
{
    uint32_t c = 0xFFFFFFFFu;
    const uint8_t* p = static_cast<const uint8_t*>(data);
    for (size_t i = 0; i < bytes; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s OUT_DIR [W H]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int W = argc > 3 ? std::atoi(argv[2]) : 640, H = argc > 3 ? std::atoi(argv[3]) : 480;
    const int rows = 15, cols = 20;
    const size_t px = (size_t)W * H;
    std::vector<float> depth(px);
    std::vector<uint8_t> bgr(px * 3);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            float z = 2000.0f + 1.5f * x * 640.0f / W - 0.8f * y * 480.0f / H;
            const bool box = x > W / 3 && x < W / 2 && y > H / 4 && y < H / 2;
            if (box) z = 1200.0f;
            if (x > 2 * W / 3 && x < 2 * W / 3 + W / 40 && y > H / 2 && y < H / 2 + H / 30) z = 0.0f;   // a hole
            depth[(size_t)y * W + x] = z;
            uint8_t* c = &bgr[((size_t)y * W + x) * 3];
            const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u);
            c[0] = (uint8_t)((box ? 40 : 150 + 60 * x / W) + (n >> 7) % 5);
            c[1] = (uint8_t)((box ? 170 : 90 + 80 * y / H) + (n >> 11) % 5);
            c[2] = (uint8_t)((box ? 200 : 60) + (n >> 17) % 5);
        }
    if (!save_raw(dir + "/kde_in_depth.bin", depth.data(), px * sizeof(float)) || !save_raw(dir + "/kde_in_bgr.bin", bgr.data(), px * 3))
        return 1;
    float* ddepth = nullptr;
    uint8_t* dbgr = nullptr;
    if (hipMalloc(&ddepth, px * sizeof(float)) != hipSuccess || hipMalloc(&dbgr, px * 3) != hipSuccess) return 1;
    if (hipMemcpy(ddepth, depth.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dbgr, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    const double f = 575.8 * W / 640.0;
    const kde::Mat33d K{{f, 0.0, W / 2.0, 0.0, f, H / 2.0, 0.0, 0.0, 1.0}};
    const kde::GpuImage8UC3 color{dbgr, H, W, (size_t)W * 3};
    int regions = 0;
    size_t valid = 0;
    uint32_t crc = 0;
    try {
        KinectDepthEnhancement KDE(W, H);
        KDE.SetParametor(rows, cols, K);
        KDE.Process(ddepth, color);                                                   // main.cpp:200
        const float3* optimized = KDE.getOptimizedPoints_Host();                      // :201
        for (size_t i = 0; i < px; ++i) valid += optimized[i].z > 50.0f;
        crc = crc32_of(optimized, px * sizeof(float3));
        if (!save_raw(dir + "/kde_optimized.bin", optimized, px * sizeof(float3))) return 1;
        std::vector<int> merged(px);
        if (hipMemcpy(merged.data(), KDE.getMergedClusterLabel_Device(), px * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        std::vector<char> is_region((size_t)rows * cols, 0);
        for (size_t i = 0; i < px; ++i)
            if (merged[i] > -1 && merged[i] < rows * cols && !is_region[(size_t)merged[i]]) {
                is_region[(size_t)merged[i]] = 1;
                ++regions;
            }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(ddepth);
    (void)hipFree(dbgr);
    if (regions < 1 || regions > rows * cols || valid < px / 2) {
        std::fprintf(stderr, "%d regions, %zu valid pixels of %zu\n", regions, valid, px);
        return 1;
    }
    std::printf("kde_demo ok %dx%d regions %d valid %zu crc32 %08x\n", W, H, regions, valid, crc);
    return 0;
}
