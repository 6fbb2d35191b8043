// les_demo.cpp — KinectDepthEnhancement::Process up to the superpixel merging (KinectDepthEnhancement.cpp:58-76) on the classes
// of include/kde/kde.hpp: nasp_demo's chain (JBF->Process, Convertor->projectiveToReal, NormalGenerator->generateNormalMap (CM),
// NASP->Segmentation(color, points, normals, 10, 50, 50, 150, 1)) plus spMerging->labelImage(NASP normals, labels, centres,
// variance).  Usage: les_demo OUT_DIR [W H].  The scene is nasp_demo's.  Writes les_segments.ppm and les_normals.ppm into
// OUT_DIR, and the three inputs of labelImage as raw little-endian arrays (les_in_normals.bin, les_in_labels.bin,
// les_in_centers.bin) so that another binding can repeat the call; prints the number of merged regions and the CRC-32 of the
// merged label image.
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

static bool save_ppm(const std::string& path, const kde::HostImage8UC3& img)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%d %d\n255\n", img.cols, img.rows);
    std::vector<uint8_t> rgb(img.px.size());
    for (size_t i = 0; i + 2 < img.px.size(); i += 3) {       // BGR -> RGB
        rgb[i] = img.px[i + 2];
        rgb[i + 1] = img.px[i + 1];
        rgb[i + 2] = img.px[i];
    }
    const bool ok = std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
    return std::fclose(f) == 0 && ok;
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
    float* ddepth = nullptr;
    uint8_t* dbgr = nullptr;
    float3* dpts = nullptr;
    if (hipMalloc(&ddepth, px * sizeof(float)) != hipSuccess || hipMalloc(&dbgr, px * 3) != hipSuccess ||
        hipMalloc(&dpts, px * sizeof(float3)) != hipSuccess)
        return 1;
    if (hipMemcpy(ddepth, depth.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dbgr, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    const double f = 575.8 * W / 640.0;
    const kde::Mat33d K{{f, 0.0, W / 2.0, 0.0, f, H / 2.0, 0.0, 0.0, 1.0}};
    const kde::GpuImage8UC3 color{dbgr, H, W, (size_t)W * 3};
    int superpixels = 0, unassigned = 0, regions = 0;
    uint32_t crc = 0;
    try {
        JointBilateralFilter JBF(W, H);
        DimensionConvertor Convertor;
        NormalMapGenerator NormalGenerator(W, H);
        NormalAdaptiveSuperpixel NASP(W, H);
        LabelEquivalenceSeg spMerging(W, H);
        spMerging.setClusterCount(rows * cols);
        NASP.SetParametor(rows, cols, K);                                             // KinectDepthEnhancement.cpp:51
        Convertor.setCameraParameters(K, W, H);                                       // :52
        NormalGenerator.setNormalEstimationMethods(NormalMapGenerator::CM);           // :53
        JBF.Process(ddepth, color);                                                   // :58
        Convertor.projectiveToReal(JBF.getFiltered_Device(), dpts);                   // :60
        NormalGenerator.generateNormalMap(dpts);                                      // :65
        NASP.Segmentation(color, dpts, NormalGenerator.getNormalMap(), 10.0f, 50.0f, 50.0f, 150.0f, 1);   // :67
        spMerging.labelImage(NASP.getNormalsDevice(), NASP.getLabelDevice(), NASP.getCentersDevice(),
                             NASP.getNormalsVarianceDevice());                                           // :76
        if (!save_ppm(dir + "/les_segments.ppm", spMerging.getSegmentResult())) return 1;
        if (!save_ppm(dir + "/les_normals.ppm", spMerging.getNormalImg())) return 1;
        const int* merged = spMerging.getMergedClusterLabel_Host();
        std::vector<char> is_region((size_t)rows * cols, 0);
        for (size_t i = 0; i < px; ++i)
            if (merged[i] > -1 && merged[i] < rows * cols && !is_region[(size_t)merged[i]]) {
                is_region[(size_t)merged[i]] = 1;
                ++regions;
            }
        crc = crc32_of(merged, px * sizeof(int));
        if (!save_raw(dir + "/les_in_normals.bin", NASP.getNormalsHost(), (size_t)rows * cols * sizeof(float3))) return 1;
        if (!save_raw(dir + "/les_in_centers.bin", NASP.getCentersHost(), (size_t)rows * cols * sizeof(float3))) return 1;
        std::vector<int> labels(px);
        if (hipMemcpy(labels.data(), NASP.getLabelDevice(), px * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 1;
        if (!save_raw(dir + "/les_in_labels.bin", labels.data(), px * sizeof(int))) return 1;
        std::vector<char> seen((size_t)rows * cols, 0);
        for (size_t i = 0; i < px; ++i) {
            if (labels[i] < 0) ++unassigned;
            else if (labels[i] < rows * cols && !seen[(size_t)labels[i]]) {
                seen[(size_t)labels[i]] = 1;
                ++superpixels;
            }
        }
        const float* var = NASP.getNormalsVarianceHost();
        const float3* nrm = NASP.getNormalsHost();
        std::printf("superpixels %d of %d, unassigned pixels %d, superpixel 0: normal %g %g %g variance %g\n", superpixels,
                    rows * cols, unassigned, nrm[0].x, nrm[0].y, nrm[0].z, var[0]);
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(ddepth);
    (void)hipFree(dbgr);
    (void)hipFree(dpts);
    if (superpixels < rows * cols / 2) {
        std::fprintf(stderr, "only %d superpixels\n", superpixels);
        return 1;
    }
    if (regions < 1 || regions > superpixels) {
        std::fprintf(stderr, "%d regions from %d superpixels\n", regions, superpixels);
        return 1;
    }
    std::printf("les_demo ok %dx%d regions %d crc32 %08x\n", W, H, regions, crc);
    return 0;
}
