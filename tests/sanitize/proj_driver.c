/* tests/test_proj_sanitize.py: tools/proj_ref.c under ASan/UBSan on small and ragged frames (W or H = 1 included) with labels
 * -1, outside the tables and at the ends of int32, planes with a zero denominator, variance 1, > 1 and NaN, holes, every odd
 * window from 1 to 15 (the halo leaves the frame on all sides), bad arguments refused */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

typedef struct { float x, y, z; } pf3;
typedef struct { float x, y, z, w; } pf4;

float proj_acos_threshold(float c);
int proj_plane_projection(int width, int height, int n_clusters, float fx, float fy, int cx, int cy, const pf4* nd,
                          const int32_t* labels, const float* variance, const pf3* points, const int32_t* size, int window,
                          float spatial_sigma, float depth_sigma, float max_angle, int min_size, pf3* plane_fitted, pf3* prefilter,
                          pf3* optimized, double* den64);

int main(void)
{
    const int geo[][3] = {{16, 6, 3}, {1, 1, 1}, {1, 37, 6}, {29, 1, 29}, {70, 50, 20}, {7, 5, 35}, {33, 25, 1}};
    if (!(proj_acos_threshold(3.141592653f / 8.0f) > 0.92f) || proj_acos_threshold(3.141592653f / 3.0f) != 0.5f) return 2;
    if (!(proj_acos_threshold(4.0f) < -1.0f) || !isinf(proj_acos_threshold(0.0f)) || !isinf(proj_acos_threshold(NAN))) return 2;
    for (size_t k = 0; k < sizeof(geo) / sizeof(geo[0]); ++k) {
        const int W = geo[k][0], H = geo[k][1], nc = geo[k][2];
        const size_t px = (size_t)W * H;
        pf4* nd = malloc(px * sizeof(pf4));
        int32_t* labels = malloc(px * sizeof(int32_t));
        float* var = malloc((size_t)nc * sizeof(float));
        int32_t* size = malloc((size_t)nc * sizeof(int32_t));
        pf3* pts = malloc(px * sizeof(pf3));
        pf3* fitted = malloc(px * sizeof(pf3));
        pf3* pre = malloc(px * sizeof(pf3));
        pf3* opt = malloc(px * sizeof(pf3));
        double* den = malloc(px * sizeof(double));
        if (!nd || !labels || !var || !size || !pts || !fitted || !pre || !opt || !den) return 1;
        unsigned s = 4211u + (unsigned)k;
        for (int a = 0; a < nc; ++a) {
            s = s * 1103515245u + 12345u;
            const unsigned q = (s >> 20) % 10;
            var[a] = 0.93f + 0.0006f * (float)((s >> 8) % 100);
            if (q == 0) var[a] = 0.5f;
            if (q == 1) var[a] = 1.0f;
            if (q == 2) var[a] = nextafterf(1.0f, 2.0f);
            if (q == 3) var[a] = NAN;
            size[a] = (int32_t)((s >> 4) % 40);
        }
        for (size_t i = 0; i < px; ++i) {
            s = s * 1103515245u + 12345u;
            const unsigned q = (s >> 16) % 50;
            labels[i] = (int32_t)(((i % (size_t)W) / 3 + (i / (size_t)W) / 2 * 5) % (size_t)nc);
            if (q == 0) labels[i] = -1;
            if (q == 1) labels[i] = nc;
            if (q == 2) labels[i] = INT32_MAX;
            if (q == 3) labels[i] = INT32_MIN;
            const float d = 800.0f + (float)((s >> 3) % 400);
            nd[i].x = 0.05f; nd[i].y = -0.03f; nd[i].z = q == 4 ? 0.0f : 0.99f; nd[i].w = d;
            if (q == 5) nd[i].x = nd[i].y = nd[i].z = nd[i].w = 0.0f;
            const float z = q > 44 ? 0.0f : d * (1.0f + 0.01f * (float)(q % 7));
            pts[i].x = 0.01f * z; pts[i].y = -0.02f * z; pts[i].z = q == 6 ? NAN : z;
        }
        for (int window = 1; window <= 15; window += 2)
            if (proj_plane_projection(W, H, nc, 50.0f, 50.0f, W / 2, H / 2, nd, labels, var, pts, size, window, 20.0f, 100.0f,
                                      window == 15 ? 4.0f : 3.141592653f / 8.0f, 20, fitted, pre, opt, window & 2 ? den : NULL) != 0)
                return 4;
        if (proj_plane_projection(W, H, nc, 50.0f, 50.0f, 0, 0, nd, labels, var, pts, size, 4, 20.0f, 100.0f, 0.4f, 20, fitted, pre, opt, den) != 1)
            return 5;
        if (proj_plane_projection(W, H, 0, 50.0f, 50.0f, 0, 0, nd, labels, var, pts, size, 7, 20.0f, 100.0f, 0.4f, 20, fitted, pre, opt, den) != 1)
            return 5;
        free(nd); free(labels); free(var); free(size); free(pts); free(fitted); free(pre); free(opt); free(den);
    }
    printf("proj driver ok\n");
    return 0;
}
