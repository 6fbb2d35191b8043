/* tests/test_les_sanitize.py: tools/les_ref.c under ASan/UBSan on small and ragged frames (W or H = 1 included) with labels
 * -1 and outside the table, bad, NaN and (-1,-1,z) normals, more superpixels than pixels refused, 0 and many rounds */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef struct { float x, y, z; } lf3;
typedef struct { float x, y, z, w; } lf4;

float les_acos_threshold(float c);
int les_label_image(int width, int height, int n_clusters, const lf3* normals, const int32_t* labels, const lf3* centers,
                    const float* variance_in, int iterations, float max_angle, float max_dist, lf4* input_nd, int32_t* merged,
                    lf4* merged_nd, int32_t* size, float* variance, int32_t* changed);

int main(void)
{
    const int geo[][3] = {{16, 6, 3}, {1, 1, 1}, {1, 37, 6}, {29, 1, 29}, {64, 48, 40}, {7, 5, 35}, {33, 21, 3}};
    if (!(les_acos_threshold(3.141592653f / 8.0f) > 0.92f) || les_acos_threshold(3.141592653f / 3.0f) != 0.5f) return 2;
    if (!(les_acos_threshold(4.0f) < -1.0f) || !isinf(les_acos_threshold(0.0f)) || !isinf(les_acos_threshold(NAN))) return 2;
    for (size_t k = 0; k < sizeof(geo) / sizeof(geo[0]); ++k) {
        const int W = geo[k][0], H = geo[k][1], nc = geo[k][2];
        const size_t px = (size_t)W * H;
        lf3* n = malloc((size_t)nc * sizeof(lf3));
        lf3* c = malloc((size_t)nc * sizeof(lf3));
        int32_t* labels = malloc(px * sizeof(int32_t));
        lf4* ind = malloc(px * sizeof(lf4));
        lf4* mnd = malloc(px * sizeof(lf4));
        int32_t* merged = malloc(px * sizeof(int32_t));
        int32_t* size = malloc((size_t)nc * sizeof(int32_t));
        float* var = malloc((size_t)nc * sizeof(float));
        int32_t changed[20];
        if (!n || !c || !labels || !ind || !mnd || !merged || !size || !var) return 1;
        unsigned s = 977u + (unsigned)k;
        for (int a = 0; a < nc; ++a) {
            s = s * 1103515245u + 12345u;
            const float t = 0.02f * (float)((s >> 8) % 60);
            n[a].x = sinf(t); n[a].y = 0.0f; n[a].z = cosf(t);
            const unsigned q = (s >> 20) % 12;
            if (q == 0) n[a].x = n[a].y = n[a].z = -1.0f;
            if (q == 1) n[a].y = NAN;
            if (q == 2) n[a].x = n[a].y = -1.0f;
            const float d = 1000.0f + (float)((s >> 4) % 300);
            c[a].x = d * n[a].x; c[a].y = d * n[a].y; c[a].z = d * n[a].z;
        }
        for (size_t i = 0; i < px; ++i) {
            s = s * 1103515245u + 12345u;
            const unsigned q = (s >> 16) % 50;
            labels[i] = (int32_t)(((i % (size_t)W) / 3 + (i / (size_t)W) / 2 * 5) % (size_t)nc);
            if (q == 0) labels[i] = -1;
            if (q == 1) labels[i] = nc;
            if (q == 2) labels[i] = INT32_MAX;
            if (q == 3) labels[i] = INT32_MIN;
            if (q > 40) labels[i] = (int32_t)((s >> 3) % (unsigned)nc);
        }
        const int its[] = {10, 0, 1, 20};
        for (size_t j = 0; j < 4; ++j)
            if (les_label_image(W, H, nc, n, labels, c, NULL, its[j], j == 3 ? 4.0f : 3.141592653f / 8.0f, j == 3 ? 1e9f : 150.0f, ind,
                                merged, mnd, size, var, changed) != 0) return 4;
        if (les_label_image(W, H, (int)px + 1, n, labels, c, NULL, 1, 0.4f, 150.0f, ind, merged, mnd, size, var, changed) != 3) return 5;
        free(n); free(c); free(labels); free(ind); free(mnd); free(merged); free(size); free(var);
    }
    printf("les driver ok\n");
    return 0;
}
