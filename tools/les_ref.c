/* les_ref.c — CPU restatement of LabelEquivalenceSeg::labelImage (LabelEquivalenceSeg/LabelEquivalenceSeg.cu:228-282), the
 * checker of kinectdepthmapenhancement_amd/csrc/les_kernels.hip.  TEST INFRASTRUCTURE ONLY: the product never links it.
 *
 * Build: tools/Makefile (-O2 -ffp-contract=off -fno-fast-math, the oracle's flags).  Wrapper: tools/les_ref.py.
 * One function per reference kernel, written per pixel and per round from the CUDA text, float32, its operations in its
 * order.  Deliberately NOT in the per-superpixel graph form the GPU uses ("Superpixel merging"): this file is an
 * independent statement of the result.  Deviations L1-L7 are written out in DESIGN.md.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct { float x, y, z; } lf3;
typedef struct { float x, y, z, w; } lf4;

/* L6: acos(d) < c is decided on the argument, d > t: t is the largest float in [-1, 1] whose double acos, rounded to
 * float, is not below c.  No such float (c <= 0): +inf, nothing passes.  Every float in [-1, 1] passes (c > pi): the
 * float just below -1 (a d below -1 has a NaN acos and fails). */
static uint32_t fkey(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static float funkey(uint32_t k)
{
    const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
float les_acos_threshold(float c)
{
    if (c != c) return INFINITY;                                   /* acos(d) < NaN is false */
    if (!((float)acos(-1.0) >= c)) return nextafterf(-1.0f, -INFINITY);
    if ((float)acos(1.0) >= c) return INFINITY;
    uint32_t lo = fkey(-1.0f), hi = fkey(1.0f);                    /* true at lo, false at hi */
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((float)acos((double)funkey(mid)) >= c) lo = mid;
        else hi = mid;
    }
    return funkey(lo);
}

/* compNormal — .cu:37-43 with L6 */
int les_comp_normal(lf4 a, lf4 b, float thr, float max_dist)
{
    const float d = (a.x * b.x + a.y * b.y) + a.z * b.z;
    return d < 1.0f && d > thr && fabsf(a.w - b.w) < max_dist;
}

/* initLabel — .cu:8-35 (L1: a label outside [0, n_clusters) is treated like a bad normal) */
void les_init_label(int width, int height, int n_clusters, const lf3* normals, const int32_t* labels, const lf3* centers,
                    lf4* input_nd, int32_t* merged, int32_t* ref)
{
    const long long npix = (long long)width * height;
    for (long long p = 0; p < npix; p++) {
        const int32_t l = labels[p];
        ref[p] = (int32_t)p;
        if (l >= 0 && l < n_clusters && (normals[l].x != -1.0f || normals[l].y != -1.0f || normals[l].z != -1.0f)) {
            const lf3 n = normals[l], c = centers[l];
            input_nd[p].x = n.x;
            input_nd[p].y = n.y;
            input_nd[p].z = n.z;
            input_nd[p].w = fabsf((n.x * c.x + n.y * c.y) + n.z * c.z);
            merged[p] = l;
        } else {
            input_nd[p].x = input_nd[p].y = input_nd[p].z = input_nd[p].w = 5.0f;
            merged[p] = -1;
        }
    }
}

/* one term of getMin — .cu:63-66; L2: a neighbour index >= W*H contributes nothing */
static int32_t min_term(long long q, long long npix, long long p, const lf4* nd, const int32_t* merged, const int32_t* labels,
                        float thr, float max_dist, int32_t c)
{
    if (q >= npix) return c;
    if (merged[q] > -1 && (labels[q] == labels[p] || les_comp_normal(nd[q], nd[p], thr, max_dist)) && merged[q] < c) return merged[q];
    return c;
}

/* scanKernel — .cu:70-109 (atomicMin on ref is a plain min: order-free) */
void les_scan(int width, int height, const lf4* input_nd, const int32_t* merged, const int32_t* labels, float thr, float max_dist,
              int32_t* ref)
{
    const long long npix = (long long)width * height;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const long long p = x + (long long)y * width;
            const int32_t label1 = merged[p];
            if (!(label1 > -1)) continue;
            const long long up = x + (long long)(y - 1 > 0 ? y - 1 : 0) * width;
            const long long left = (x - 1 > 0 ? x - 1 : 0) + (long long)y * width;
            const long long right = (x + 1 < width ? x + 1 : width) + (long long)y * width;
            const long long down = x + (long long)(y + 1 < height ? y + 1 : height) * width;
            int32_t c = merged[p];
            c = min_term(up, npix, p, input_nd, merged, labels, thr, max_dist, c);
            c = min_term(left, npix, p, input_nd, merged, labels, thr, max_dist, c);
            c = min_term(right, npix, p, input_nd, merged, labels, thr, max_dist, c);
            c = min_term(down, npix, p, input_nd, merged, labels, thr, max_dist, c);
            if (c < label1 && c < ref[label1]) ref[label1] = c;
        }
}

/* analysisKernel — .cu:110-136 as the two phases of L3; scratch holds W*H ints */
void les_analysis(int width, int height, int32_t* merged, int32_t* ref, const int32_t* labels, int32_t* scratch)
{
    const long long npix = (long long)width * height;
    memcpy(scratch, ref, (size_t)npix * sizeof(int32_t));          /* the table as it stood before the phase */
    for (long long p = 0; p < npix; p++)
        if (merged[p] == labels[p]) {
            int32_t current = scratch[p];
            do {
                current = scratch[current];
            } while (current != scratch[current]);
            ref[p] = current;
        }
    for (long long p = 0; p < npix; p++)
        if (merged[p] > -1) merged[p] = ref[merged[p]];
}

/* countKernel + calculate_nd — .cu:162-226 under L4 (sums per member superpixel in ascending label order, count times
 * value) and L5 (everything starts from 0, merged_nd is 0 where the merged label is -1).  size / variance have
 * n_clusters entries.  Returns 1 if two pixels of one superpixel carry different merged labels (the invariant the
 * definition of L4 rests on; it cannot happen). */
int les_count_and_nd(int width, int height, int n_clusters, int32_t* merged, const lf4* input_nd, const int32_t* labels,
                     const lf3* centers, lf4* merged_nd, int32_t* size, float* variance)
{
    const long long npix = (long long)width * height;
    int32_t* cnt = calloc((size_t)n_clusters, sizeof(int32_t));
    int32_t* mof = malloc((size_t)n_clusters * sizeof(int32_t));
    lf4* ndof = malloc((size_t)n_clusters * sizeof(lf4));
    lf3* sn = calloc((size_t)n_clusters, sizeof(lf3));
    lf3* sc = calloc((size_t)n_clusters, sizeof(lf3));
    char* first = calloc((size_t)n_clusters, 1);
    lf4* mnd = calloc((size_t)n_clusters, sizeof(lf4));
    int rc = 0;
    if (!cnt || !mof || !ndof || !sn || !sc || !first || !mnd) { rc = 2; goto done; }
    for (int a = 0; a < n_clusters; a++) { mof[a] = -1; size[a] = 0; variance[a] = 0.0f; }
    /* countKernel's test (.cu:172-174 reads .y twice; kept) */
    for (long long p = 0; p < npix; p++) {
        if (merged[p] > -1 && (input_nd[p].x != -1.0f || input_nd[p].y != -1.0f || input_nd[p].y != -1.0f)) {
            const int32_t a = labels[p];
            if (cnt[a] == 0) { mof[a] = merged[p]; ndof[a] = input_nd[p]; }
            else if (mof[a] != merged[p]) rc = 1;
            cnt[a]++;
            size[merged[p]]++;
        } else {
            merged[p] = -1;
        }
    }
    for (int a = 0; a < n_clusters; a++) {
        if (cnt[a] == 0) continue;
        const int32_t m = mof[a];
        const float c = (float)cnt[a];
        const lf3 pn = {c * ndof[a].x, c * ndof[a].y, c * ndof[a].z};
        const lf3 pc = {c * centers[a].x, c * centers[a].y, c * centers[a].z};
        if (!first[m]) { sn[m] = pn; sc[m] = pc; first[m] = 1; }
        else {
            sn[m].x = sn[m].x + pn.x; sn[m].y = sn[m].y + pn.y; sn[m].z = sn[m].z + pn.z;
            sc[m].x = sc[m].x + pc.x; sc[m].y = sc[m].y + pc.y; sc[m].z = sc[m].z + pc.z;
        }
    }
    for (int m = 0; m < n_clusters; m++) {
        if (!first[m]) continue;
        const float s = (float)size[m];
        mnd[m].x = sn[m].x / s;
        mnd[m].y = sn[m].y / s;
        mnd[m].z = sn[m].z / s;
        const lf3 ctr = {sc[m].x / s, sc[m].y / s, sc[m].z / s};
        mnd[m].w = fabsf((mnd[m].x * ctr.x + mnd[m].y * ctr.y) + mnd[m].z * ctr.z);
        first[m] = 2;
    }
    for (int a = 0; a < n_clusters; a++) {
        if (cnt[a] == 0) continue;
        const int32_t m = mof[a];
        float v = (ndof[a].x * mnd[m].x + ndof[a].y * mnd[m].y) + ndof[a].z * mnd[m].z;
        v /= (float)size[m];
        const float pv = (float)cnt[a] * v;
        if (first[m] == 2) { variance[m] = pv; first[m] = 3; }
        else variance[m] = variance[m] + pv;
    }
    for (long long p = 0; p < npix; p++) {
        if (merged[p] > -1) merged_nd[p] = mnd[merged[p]];
        else merged_nd[p].x = merged_nd[p].y = merged_nd[p].z = merged_nd[p].w = 0.0f;
    }
done:
    free(cnt); free(mof); free(ndof); free(sn); free(sc); free(first); free(mnd);
    return rc;
}

/* labelImage — .cu:228-282.  changed (may be NULL) receives, per round, the number of pixels whose merged label the round
 * changed.  variance_in is the dead fourth argument: never read.  Returns 0, or the error of les_count_and_nd. */
int les_label_image(int width, int height, int n_clusters, const lf3* normals, const int32_t* labels, const lf3* centers,
                    const float* variance_in, int iterations, float max_angle, float max_dist, lf4* input_nd, int32_t* merged,
                    lf4* merged_nd, int32_t* size, float* variance, int32_t* changed)
{
    (void)variance_in;
    const long long npix = (long long)width * height;
    if (width < 1 || height < 1 || n_clusters < 1 || n_clusters > npix || iterations < 0) return 3;
    int32_t* ref = malloc((size_t)npix * sizeof(int32_t));
    int32_t* scratch = malloc((size_t)npix * sizeof(int32_t));
    int32_t* before = malloc((size_t)npix * sizeof(int32_t));
    if (!ref || !scratch || !before) { free(ref); free(scratch); free(before); return 2; }
    const float thr = les_acos_threshold(max_angle);
    les_init_label(width, height, n_clusters, normals, labels, centers, input_nd, merged, ref);
    for (int i = 0; i < iterations; i++) {
        memcpy(before, merged, (size_t)npix * sizeof(int32_t));
        les_scan(width, height, input_nd, merged, labels, thr, max_dist, ref);
        les_analysis(width, height, merged, ref, labels, scratch);
        if (changed) {
            int32_t c = 0;
            for (long long p = 0; p < npix; p++) c += before[p] != merged[p];
            changed[i] = c;
        }
    }
    const int rc = les_count_and_nd(width, height, n_clusters, merged, input_nd, labels, centers, merged_nd, size, variance);
    free(ref); free(scratch); free(before);
    return rc;
}
