/* tests/test_nasp_sanitize.py: tools/nasp_ref.c under ASan/UBSan on ragged and smallest-accepted geometries, with holes,
 * bad and NaN normals, and a sigma of 0 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef struct { uint8_t r, g, b, pad_; int32_t x, y, size; } nsp;
typedef struct { float d; int32_t l; } nld;

int nasp_check_geometry(int width, int height, int rows, int cols);
int nasp_segmentation(int width, int height, int rows, int cols, const float* intr9, const uint8_t* bgr, const float* points,
                      const float* normals, float color_sigma, float spatial_sigma, float depth_sigma, float normal_sigma,
                      int iteration, int32_t* labels, nld* ld, nsp* mean, float* centers, float* sp_normals, float* variance);
float nasp_acos_threshold(void);
float nasp_weight(float num, float sigma);

int main(void)
{
    const int geo[][4] = {{64, 64, 8, 8}, {70, 50, 3, 5}, {8, 8, 1, 1}, {333, 97, 5, 13}, {40, 6 + 3, 1, 5}};
    if (nasp_acos_threshold() != 0.5f) return 2;
    if (nasp_weight(0.0f, 10.0f) != 1.0f || nasp_weight(1e9f, 10.0f) != 0.0f) return 2;
    if (!nasp_check_geometry(64, 64, 9, 8) || !nasp_check_geometry(64, 5, 1, 8)) return 2;     /* both rejected */
    for (size_t k = 0; k < sizeof(geo) / sizeof(geo[0]); ++k) {
        const int W = geo[k][0], H = geo[k][1], rows = geo[k][2], cols = geo[k][3];
        if (nasp_check_geometry(W, H, rows, cols)) return 3;
        const size_t px = (size_t)W * H, nc = (size_t)rows * cols;
        uint8_t* bgr = malloc(px * 3);
        float* p = malloc(px * 3 * sizeof(float));
        float* n = malloc(px * 3 * sizeof(float));
        int32_t* labels = malloc(px * sizeof(int32_t));
        nld* ld = malloc(px * sizeof(nld));
        nsp* mean = calloc(nc, sizeof(nsp));
        float* centers = calloc(nc * 3, sizeof(float));
        float* spn = calloc(nc * 3, sizeof(float));
        float* var = calloc(nc, sizeof(float));
        if (!bgr || !p || !n || !labels || !ld || !mean || !centers || !spn || !var) return 1;
        unsigned s = 4321u + (unsigned)k;
        for (size_t i = 0; i < px; ++i) {
            s = s * 1103515245u + 12345u;
            const float z = (s >> 16) % 9 == 0 ? 0.0f : 800.0f + (float)((s >> 8) % 2000);
            p[3 * i + 0] = ((float)(i % W) - W / 2.0f) * z / 575.0f;
            p[3 * i + 1] = (H / 2.0f - (float)(i / W)) * z / 575.0f;
            p[3 * i + 2] = z;
            bgr[3 * i] = (uint8_t)(s >> 5); bgr[3 * i + 1] = (uint8_t)(s >> 11); bgr[3 * i + 2] = (uint8_t)(s >> 19);
            const unsigned q = (s >> 3) % 40;
            n[3 * i] = 0.0f; n[3 * i + 1] = 0.6f; n[3 * i + 2] = -0.8f;
            if (q == 0) n[3 * i] = n[3 * i + 1] = n[3 * i + 2] = -1.0f;
            if (q == 1) n[3 * i] = n[3 * i + 1] = n[3 * i + 2] = NAN;
        }
        const float intr[9] = {575.0f, 0.0f, W / 2.0f, 0.0f, 575.0f, H / 2.0f, 0.0f, 0.0f, 1.0f};
        const float sig[][4] = {{10.0f, 50.0f, 50.0f, 150.0f}, {10.0f, 50.0f, 0.0f, 150.0f}, {0.0f, 50.0f, 50.0f, 0.0f}, {200.0f, 0.5f, 0.0f, 0.0f}};
        for (size_t j = 0; j < sizeof(sig) / sizeof(sig[0]); ++j)
            if (nasp_segmentation(W, H, rows, cols, intr, bgr, p, n, sig[j][0], sig[j][1], sig[j][2], sig[j][3], j == 0 ? 3 : 1,
                                  labels, ld, mean, centers, spn, var) != 0) return 4;
        free(bgr); free(p); free(n); free(labels); free(ld); free(mean); free(centers); free(spn); free(var);
    }
    printf("nasp driver ok\n");
    return 0;
}
