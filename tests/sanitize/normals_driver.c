/* tests/test_normals_ref.py: tools/normals_ref.c under ASan/UBSan on ragged and degenerate frame sizes */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int nref_normals(int W, int H, const float* pts_mm, int method, float f, float s, float* normals, float* fs_out,
                 uint8_t* band);

int main(void)
{
    const int sizes[][2] = {{1, 1}, {1, 37}, {37, 1}, {41, 43}, {2, 2}, {64, 3}};
    for (size_t k = 0; k < sizeof(sizes) / sizeof(sizes[0]); ++k) {
        const int W = sizes[k][0], H = sizes[k][1];
        const size_t px = (size_t)W * H;
        float* p = malloc(px * 3 * sizeof(float));
        float* n = malloc(px * 3 * sizeof(float));
        float* fs = malloc(px * sizeof(float));
        uint8_t* band = malloc(px);
        if (!p || !n || !fs || !band) return 1;
        unsigned s = 12345u + (unsigned)k;
        for (size_t i = 0; i < px; ++i) {
            s = s * 1103515245u + 12345u;
            const float z = (s >> 16) % 7 == 0 ? 0.0f : 800.0f + (float)((s >> 8) % 3000);
            p[3 * i + 0] = ((float)(i % W) - W / 2.0f) * z / 575.0f;
            p[3 * i + 1] = (H / 2.0f - (float)(i / W)) * z / 575.0f;
            p[3 * i + 2] = z;
        }
        /* a small smoothing size so that CM windows fit inside the small frames too */
        if (nref_normals(W, H, p, 1, 0.05f, 3.0f, n, fs, band) != 0) return 1;
        if (nref_normals(W, H, p, 1, 0.05f, 20.0f, n, fs, band) != 0) return 1;
        if (nref_normals(W, H, p, 2, 0.05f, 20.0f, n, NULL, NULL) != 0) return 1;
        free(p);
        free(n);
        free(fs);
        free(band);
    }
    printf("normals driver ok\n");
    return 0;
}
