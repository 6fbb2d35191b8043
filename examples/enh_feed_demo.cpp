// enh_feed_demo.cpp — the reference's "PROPOSED" method (main.cpp:198-202) fed the way a sensor feeds it: uint16 depth
// frames (millimetres, 0 = invalid) and BGR frames in host memory (main.cpp:160-163) through kde::KinectDepthEnhancementFeed,
// the enhanced depth back in the same uint16 format.
// Usage: enh_feed_demo OUT_DIR [FRAMES].  The scene is kde_demo's, moved a little from frame to frame; frames are 640x480,
// 15 x 20 superpixels, fed in chunks of 2.  Writes the inputs as raw little-endian arrays (enh_feed_in_depth.bin uint16
// [FRAMES][H][W], enh_feed_in_bgr.bin uint8 [FRAMES][H][W][3]) so that another binding can repeat the call, and the result
// as enh_feed_depth.bin (uint16 [FRAMES][H][W]); prints the frame count, the number of pixels with a valid enhanced depth and
// the CRC-32 of the result.
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
        std::fprintf(stderr, "usage: %s OUT_DIR [FRAMES]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int N = argc > 2 ? std::atoi(argv[2]) : 5;
    const int W = 640, H = 480, rows = 15, cols = 20, chunk = 2;
    if (N < 1 || N > 64) {
        std::fprintf(stderr, "FRAMES must be in 1..64\n");
        return 2;
    }
    const size_t px = (size_t)W * H;
    std::vector<uint16_t> depth(px * N), enhanced(px * N);
    std::vector<uint8_t> bgr(px * 3 * N);
    for (int f = 0; f < N; ++f)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int bx = x - 8 * f;                                   // the box moves right, the wall comes closer
                int z = 2000 + (3 * x) / 2 - (4 * y) / 5 - 20 * f;
                const bool box = bx > W / 3 && bx < W / 2 && y > H / 4 && y < H / 2;
                if (box) z = 1200;
                if (x > 2 * W / 3 && x < 2 * W / 3 + W / 40 && y > H / 2 && y < H / 2 + H / 30) z = 0;   // a hole
                depth[f * px + (size_t)y * W + x] = (uint16_t)z;
                uint8_t* c = &bgr[(f * px + (size_t)y * W + x) * 3];
                const unsigned n = ((unsigned)x * 2654435761u) ^ ((unsigned)y * 40503u) ^ ((unsigned)f * 69069u);
                c[0] = (uint8_t)((box ? 40 : 150 + 60 * x / W) + (n >> 7) % 5);
                c[1] = (uint8_t)((box ? 170 : 90 + 80 * y / H) + (n >> 11) % 5);
                c[2] = (uint8_t)((box ? 200 : 60) + (n >> 17) % 5);
            }
    if (!save_raw(dir + "/enh_feed_in_depth.bin", depth.data(), depth.size() * sizeof(uint16_t)) ||
        !save_raw(dir + "/enh_feed_in_bgr.bin", bgr.data(), bgr.size()))
        return 1;
    const double fl = 575.8 * W / 640.0;
    const kde::Mat33d K{{fl, 0.0, W / 2.0, 0.0, fl, H / 2.0, 0.0, 0.0, 1.0}};
    kde_feed_stats st{};
    try {
        KinectDepthEnhancement KDE(W, H, chunk);
        KDE.SetParametor(rows, cols, K);
        kde::KinectDepthEnhancementFeed feed(KDE, chunk);
        feed.process(N, depth.data(), bgr.data(), enhanced.data());       // uint16 in, uint16 out
        st = feed.lastStats();
    } catch (const kde::Error& e) {
        std::fprintf(stderr, "kde error: %s\n", e.what());
        return 1;
    }
    size_t valid = 0;
    for (uint16_t v : enhanced) valid += v != 0;
    const uint32_t crc = crc32_of(enhanced.data(), enhanced.size() * sizeof(uint16_t));
    if (!save_raw(dir + "/enh_feed_depth.bin", enhanced.data(), enhanced.size() * sizeof(uint16_t))) return 1;
    if (st.frames != N || st.chunks != (N + chunk - 1) / chunk || valid < px * N / 2) {
        std::fprintf(stderr, "%d frames in %d chunks, %zu valid pixels of %zu\n", st.frames, st.chunks, valid, px * N);
        return 1;
    }
    std::printf("enh_feed_demo ok %dx%d frames %d chunks %d valid %zu crc32 %08x\n", W, H, N, st.chunks, valid, crc);
    return 0;
}
