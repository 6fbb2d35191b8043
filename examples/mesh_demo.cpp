// mesh_demo.cpp — a synthetic frame as a shaded surface: kde::OrganizedMesh turns the depth map and the colour image into
//   the dense cloud of main.cpp:211-300 (the vertices) and the triangles of the organised grid on the device, and
//   kde::writePly saves both as a binary PLY 1.0 file.
// Usage: mesh_demo [W H [out.ply]].  The scene is cloud_demo's: a slanted wall, a box in front of it, a hole.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/kde/kde.hpp"
#include "../include/kde/ply_io.hpp"

int main(int argc, char** argv)
{
    const int W = argc > 2 ? std::atoi(argv[1]) : 640, H = argc > 2 ? std::atoi(argv[2]) : 480;
    const char* path = argc > 3 ? argv[3] : "mesh_demo.ply";
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
    float* ddepth = nullptr;
    uint8_t* dbgr = nullptr;
    if (hipMalloc(&ddepth, px * sizeof(float)) != hipSuccess || hipMalloc(&dbgr, px * 3) != hipSuccess) return 1;
    if (hipMemcpy(ddepth, depth.data(), px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dbgr, bgr.data(), px * 3, hipMemcpyHostToDevice) != hipSuccess)
        return 1;
    const double f = 575.8 * W / 640.0;
    const kde::Mat33d K{{f, 0.0, W / 2.0, 0.0, f, H / 2.0, 0.0, 0.0, 1.0}};
    uint32_t nv = 0, nt = 0;
    try {
        kde::OrganizedMesh mesh(W, H);
        mesh.setCamera(K);
        mesh.build(1, kde::MeanError3D::source(ddepth), dbgr);
        const uint64_t *voff = nullptr, *toff = nullptr;
        const kde_cloud_point* vertices = mesh.vertices_Host(&voff);
        const kde_mesh_triangle* triangles = mesh.triangles_Host(&toff);
        nv = mesh.counts_Host()[0];
        nt = mesh.triCounts_Host()[0];
        if (voff[1] != nv || toff[1] != nt || nv != px - holes || nt == 0 || nt > 2 * (size_t)(W - 1) * (H - 1)) {
            std::fprintf(stderr, "mesh_demo: %u vertices (%zu valid pixels), %u triangles\n", nv, px - holes, nt);
            return 1;
        }
        for (uint32_t i = 0; i < nt; ++i)
            if (triangles[i].v0 >= nv || triangles[i].v1 >= nv || triangles[i].v2 >= nv) {
                std::fprintf(stderr, "mesh_demo: triangle %u is (%u, %u, %u) of %u vertices\n", i, triangles[i].v0, triangles[i].v1, triangles[i].v2, nv);
                return 1;
            }
        if (!kde::writePly(path, vertices, nv, triangles, nt)) {
            std::fprintf(stderr, "mesh_demo: cannot write %s\n", path);
            return 1;
        }
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    (void)hipFree(ddepth);
    (void)hipFree(dbgr);
    // the file says what the device counted
    std::FILE* in = std::fopen(path, "rb");
    if (!in) return 1;
    char line[128];
    unsigned long fv = 0, ff = 0;
    while (std::fgets(line, sizeof line, in) && std::string(line) != "end_header\n") {
        std::sscanf(line, "element vertex %lu", &fv);
        std::sscanf(line, "element face %lu", &ff);
    }
    std::fclose(in);
    if (fv != nv || ff != nt) {
        std::fprintf(stderr, "mesh_demo: the file holds %lu vertices and %lu faces, the device counted %u and %u\n", fv, ff, nv, nt);
        return 1;
    }
    std::printf("mesh_demo ok %dx%d vertices %u triangles %u (%.3f per pixel) -> %s\n", W, H, nv, nt, (double)nt / (double)px, path);
    return 0;
}
