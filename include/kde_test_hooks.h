/*
 * include/kde_test_hooks.h — entry points of tools/hooks/libkde_hooks.so and libkde_hip_stage.so.
 *
 * NOT part of the product ABI (include/kde_hip.h / libkde_hip.so export none of these): a measurement helper for
 * bench.py and a probe that lets a test call a device function of the product kernels on chosen arguments.
 */
#ifndef KDE_TEST_HOOKS_H
#define KDE_TEST_HOOKS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* float4 streaming copy (one 16-byte element per thread, the loop shape tools/hbm_microbench found fastest):
 * the empirical HBM ceiling bench.py quotes next to the 8 TB/s datasheet figure.  0 = ok. */
int kde_bench_copy(const void* src_dev, void* dst_dev, size_t bytes, void* stream);

/* packed-BGR copy of npix pixels with K0's access pattern (one unaligned dword load per pixel, 16-bit stores): run under the
 * same PMC passes as K0 it calibrates FETCH_SIZE / WRITE_SIZE for that pattern (exactly 3 bytes read and written per
 * pixel), which the 2 x FETCH_SIZE rule of 16-byte streams does not cover.  0 = ok. */
int kde_bench_bgr3_copy(const void* src_dev, void* dst_dev, size_t npix, void* stream);

/* out_dev[i] = the kernels' square root (csrc/kde_device_math.h, sqrt_int24) of the integer first + i
 * (i < n; first + n <= 2^24), so that the tests can prove it equal to sqrtf() on every argument calculateLD can
 * form (DepthAdaptiveSuperpixel.cu:213).  0 = ok. */
int kde_test_sqrt_int24(uint32_t first, uint32_t n, float* out_dev, void* stream);

/* out_dev[i] = fastdiv24(xs_dev[i], make_fastdiv24(d, max_dividend)) evaluated ON THE DEVICE with the very functions of
 * csrc/kde_device_math.h (the division-by-multiplication of K1's tile map and K7's grid-cell arithmetic), so that a test
 * can compare it with x / d -- including the fallback path (ok == 0: d or max_dividend >= 2^24).  m_sh_ok (host, 3 words,
 * may be NULL) receives the magic number, the shift and the ok flag make_fastdiv24 chose.  0 = ok. */
int kde_test_fastdiv24(uint32_t d, uint64_t max_dividend, uint32_t n, const uint32_t* xs_dev, uint32_t* out_dev,
                       uint32_t* m_sh_ok, void* stream);

/* The 256-way reduction tree of the superpixel cluster kernels (csrc/kde_superpixel_device.h, tree256<2, 2>) run by ONE
 * 256-thread workgroup: thread t contributes iv_rows_dev[r * 256 + t] and fv_rows_dev[r * 256 + t] for r = 0, 1.
 * out_dev (4 words) receives lane 0's results: the two integer sums (modulo 2^32), then the bits of the two float sums,
 * whose value depends on the tree's order of additions.  0 = ok. */
int kde_test_tree256(const int32_t* iv_rows_dev, const float* fv_rows_dev, uint32_t* out_dev, void* stream);

/* ---- tools/hooks/libkde_hip_stage.so ------------------------------------------------------------------------------
 * The product library's own sources compiled with -DKDE_STAGE_HOOKS: every entry point of include/kde_hip.h (same
 * code, same flags) plus the four below.  It exists so that the parity tests can check K1 and K10 STAGE BY STAGE: the
 * composite filters are ill-conditioned only through their first-pass average (and K10's deviation), each stage by
 * itself is well-conditioned, so the tests take the GPU's own average / deviation, re-evaluate the last pass from
 * them in binary64 on the CPU and hold the GPU's final value to 1e-4 against that (oracle/oracle.py: stage_check_*).
 * A test first asserts that this library's final output is bit-identical to the product library's.
 *
 * kde_stage_set(jbf_avg, ers_avg, ers_dev, counters, force_full_rules) — process-wide, applies to later launches:
 *   jbf_avg   device float[n*H*W] or NULL: K1's first-pass average exactly as its second pass uses it
 *             (JointBilateralFilter.cu:38-41; NaN where the sum of weights is 0 and the output is therefore 0)
 *   ers_avg   device float[H*W] or NULL: K10's label-restricted average (EdgeRefinedSuperpixel.cu:139-141)
 *   ers_dev   device float[H*W] or NULL: K10's mean absolute deviation (EdgeRefinedSuperpixel.cu:143-156); only
 *             meaningful where ers_avg is not NaN
 *   counters  device unsigned[8] or NULL: [0..3] K1 packed kernels, once per wavefront that owns at least one pixel, by the
 *             body the wavefront ran (bit 0: colour rule compiled in, bit 1: depth rule); once per tile: [4]/[5] K10 tiles with / without the "adaptive
 *             sigma provably small" shortcut, [6]/[7] K10 tiles without / with the depth rule in the colour-free rows
 *   force_full_rules  != 0: no rule elision — every wavefront runs the body with both Q1 rules (K1) / every tile the per-pixel
 *             deviation pass and the depth rule (K10); the output must not change by a bit                          */
int kde_stage_set(float* jbf_avg_dev, float* ers_avg_dev, float* ers_dev_dev, unsigned* counters_dev, int force_full_rules);

/* kde_stage_spdsr_tail(h, n, labels, points, nd_or_null, sweeps, stream) — the tail of kde_spdsr_process_batch (everything
 * after the back-projection) on the CALLER's labels and cloud instead of the head's, so that a test can feed the plane fit
 * and the mrf sweeps inputs the segmenters never produce:
 *   labels_dev  device int32[n*H*W]; any value is tolerated (< 0 or >= rows*cols: the pixel belongs to no cluster)
 *   points_dev  device kde_float3[n*H*W]
 *   nd_dev_or_null  NULL: the planes are fitted (launch_spdsr_cluster_planes into the handle's tables, as Process does);
 *               else device float[n*rows*cols*4], copied into ClusterND_Device INSTEAD of the fit, which makes the
 *               projection deterministic to the bit
 *   sweeps      >= 0: number of mrf sweeps (Process always runs 20); 0 leaves optimized = points
 * Results through the handle's own getters: kde_spdsr_cluster_nd_device, kde_spdsr_plane_fitted_points_device,
 * kde_spdsr_optimized_points_device / _host (n frames).  h is a kde_spdsr* of THIS library after set_parameters.
 * Refused with KDE_ERR_INVALID before any launch: a null h / labels / points, SetParametor not called, n outside
 * 1..max_batch, sweeps < 0.  0 = ok. */
struct kde_spdsr;
struct kde_float3;
int kde_stage_spdsr_tail(struct kde_spdsr* h, int n, const int32_t* labels_dev, const struct kde_float3* points_dev,
                         const float* nd_dev_or_null, int sweeps, void* stream);

/* ---- the size-selected kernel forms --------------------------------------------------------------------------------
 * Twelve launch sites of the library (csrc/kde_internal.h: CacheSite, past_cache) pick the streaming twin of their kernel
 * -- non-temporal loads and stores, nothing else differs -- when a call moves more than 256 MiB.  The stage build lets a
 * test reach the twin at any shape and proves that it did:
 *
 * kde_stage_set_cache_bytes(bytes) — process-wide, applies to later calls: the sites compare with `bytes` instead of
 *   256 MiB.  0: every call streams (where the site's other conditions, such as 16-byte alignment, hold).
 *   (size_t)256 << 20 restores the product's behaviour.
 * kde_stage_streaming_launches(counts, n) — copies out the first n (0 .. KDE_STAGE_SITES) host counters and zeroes all of
 *   them.  counts[site] = how often that site has launched its streaming form since the last call.  Not thread-safe. */
enum kde_stage_site {
    KDE_STAGE_SITE_P2R_DEPTH = 0,        /* kde_dimconv_projective_to_real_depth / _interp: vector form only */
    KDE_STAGE_SITE_POINTS_MAP,           /* kde_dimconv_projective_to_real_points / real_to_projective: vector form only */
    KDE_STAGE_SITE_POINTS_TO_DEPTH_F32,  /* kde_points_to_depth, float output: vector form only */
    KDE_STAGE_SITE_POINTS_TO_DEPTH_U16,  /* kde_points_to_depth, uint16 output: vector form only */
    KDE_STAGE_SITE_CLOUD,                /* kde_cloud_build_batch, and the vertices of kde_mesh_build_batch */
    KDE_STAGE_SITE_MESH,                 /* kde_mesh_build_batch: classify and emit */
    KDE_STAGE_SITE_ERROR3D,              /* kde_error3d_compare_batch */
    KDE_STAGE_SITE_UNDIST_COLOR,         /* kde_undist_color_batch */
    KDE_STAGE_SITE_UNDIST_DEPTH,         /* kde_undist_depth_batch */
    KDE_STAGE_SITE_REG,                  /* kde_reg_register_batch: scatter and finalise */
    KDE_STAGE_SITE_REG_GATHER,           /* kde_reg_color_to_depth_batch */
    KDE_STAGE_SITE_TEMPORAL,             /* kde_temporal_filter_batch */
    KDE_STAGE_SITES
};
int kde_stage_set_cache_bytes(size_t bytes);
int kde_stage_streaming_launches(uint64_t* counts, int n);

#ifdef __cplusplus
}
#endif
#endif
