/*
 * kde_hip.h — C ABI of libkde_hip.so: the MI355X (gfx950) depth-enhancement filter stage.
 *
 * Drop-in boundary for the hot path of stevesuyao/KinectDepthMapEnhancement
 *   DimensionConvertor / Buffer2D -> JointBilateralFilter::Process -> RegionGrowingBilateralFilter::Process
 * The reference has no FFI; its boundary is the public C++ class surface.  Each entry
 * point below names the reference member (file:line, relative to the reference root) it replaces.
 * include/kde/ holds header-only C++ classes with the reference's names and signatures that
 * forward to this ABI (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - plain C types only: device pointers are raw pointers into HIP device memory owned by the
 *     caller unless a getter says "object-owned"; streams are passed as void* (a hipStream_t,
 *     NULL = the null stream).  Every call is asynchronous on that stream unless stated.
 *   - every function returns KDE_OK (0) or a KDE_ERR_* code and never aborts;
 *     kde_last_error_string() describes the last failure on the calling thread.
 *   - colour images are packed 8UC3 BGR ("CV_8UC3 continuous", cv::gpu::createContinuous,
 *     JointBilateralFilter.cpp:13); depth is float32 millimetres, row-major W x H;
 *     "valid" means depth > 50.0f everywhere (JointBilateralFilter.cu:21).
 *   - a handle is one stream-ordered context (scratch buffers are members, like the reference
 *     objects); handles are independent, a single handle is not thread-safe.
 *   - a handle belongs to the device that was current when it was created (kde_set_device): calls
 *     made while another device is current return KDE_ERR_INVALID instead of launching on it.
 *   - batched entry points take n independent frames laid out back to back
 *     (frame f at base + f * W*H elements) and are the unit that is sharded across GPUs.
 */
#ifndef KDE_HIP_H
#define KDE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KDE_ABI_VERSION 1

enum {
    KDE_OK = 0,
    KDE_ERR_INVALID = 1,      /* bad argument / unsupported geometry            */
    KDE_ERR_HIP = 2,          /* a HIP runtime call failed                      */
    KDE_ERR_NOMEM = 3,        /* host or device allocation failed               */
    KDE_ERR_UNSUPPORTED = 4   /* feature outside the built scope                */
};

/* ---- device-visible record layouts (identical to the reference's) ------------------------- */
typedef struct kde_float3 { float x, y, z; } kde_float3;            /* CUDA float3, 12 B packed          */
typedef struct kde_weighted_d { float d, w; } kde_weighted_d;       /* ArrayBuffer/ArrayBuffer.h:12-15    */
typedef struct kde_superpixel {                                     /* SuperpixelSegmentation.h:17-24     */
    uint8_t r, g, b, pad_;
    int32_t x, y, size;
} kde_superpixel;                                                   /* 16 B                               */
typedef struct kde_label_distance { float d; int32_t l; } kde_label_distance; /* SuperpixelSegmentation.h:26-29 */

/* ---- library ------------------------------------------------------------------------------- */
int kde_abi_version(void);
const char* kde_last_error_string(void);
int kde_device_count(int* count);
int kde_set_device(int device);
/* name/arch of the current device, e.g. "gfx950:sramecc+:xnack-"; buf may be NULL to query cu_count only */
int kde_device_info(char* arch_buf, size_t arch_cap, int* cu_count);
/* PCI address of the current device ("0000:05:00.0", hipDeviceGetPCIBusId): what tells two GPUs of a node apart.
 * The reference is single-device (main.cpp:160-163); the sharding hosts put it in their report so that a run
 * over N devices shows N distinct addresses */
int kde_device_pci_bus_id(char* buf, size_t cap);

/* ============================================================================================
 * JointBilateralFilter — JointBilateralFilter/JointBilateralFilter.{h,cpp,cu}
 * ========================================================================================== */
typedef struct kde_jbf_params {
    int   window_size;              /* WindowSize = 5     JointBilateralFilter.cpp:3  (odd, 1..31) */
    float spatial_sigma;            /* SpatialSigma = 70  :4  (pixels)                              */
    float color_sigma;              /* ColorSigma = 50    :5  (0..255 colour levels; 0 = term off)  */
    float depth_sigma;              /* DepthSigma = 20    :6  (millimetres; 0 = term off)           */
    int   presmooth;                /* 1: guide = cv::gpu::bilateralFilter(colour) (.cu:285); 0: guide = colour */
    int   presmooth_kernel_size;    /* 5    (.cu:285)                                               */
    float presmooth_sigma_color;    /* 30.0 (.cu:285)                                               */
    float presmooth_sigma_spatial;  /* 30.0 (.cu:285)                                               */
} kde_jbf_params;

typedef struct kde_jbf kde_jbf;

/* fills the reference's compile-time constants */
int kde_jbf_default_params(kde_jbf_params* p);
/* JointBilateralFilter::JointBilateralFilter(width, height) + calcSpatialFilter()
 * (JointBilateralFilter.cpp:8-20, 31-40).  params == NULL -> defaults.  max_batch >= 1 sizes the
 * object-owned output / guide buffers for the batched entry points. */
int kde_jbf_create(kde_jbf** out, int width, int height, int max_batch, const kde_jbf_params* params);
/* JointBilateralFilter::~JointBilateralFilter (JointBilateralFilter.cpp:21-30) */
int kde_jbf_destroy(kde_jbf* h);
/* void JointBilateralFilter::Process(float* depth_device, cv::gpu::GpuMat color_image)
 * (JointBilateralFilter.cu:283-290).  bgr_step is GpuMat::step and must equal 3*width.
 * Depth is in millimetres; samples that are NaN, -inf or <= 50 are absent taps, as in the reference.  +inf and samples
 * above 2^64 make every output whose window holds them non-finite garbage in the reference; the tuned kernels keep all
 * other pixels exact to the usual bar but do not reproduce that garbage class for class (kde_jbf_set_variant(h, 0)
 * does).  DESIGN.md section 3, "input domain". */
int kde_jbf_process(kde_jbf* h, const float* depth_dev, const uint8_t* bgr_dev, size_t bgr_step, void* stream);
/* the same over n <= max_batch independent frames; filtered_dev == NULL writes the object-owned buffer */
int kde_jbf_process_batch(kde_jbf* h, int n, const float* depth_dev, const uint8_t* bgr_dev,
                          float* filtered_dev, void* stream);
/* the two kernels of Process individually (K0 = pre-smoothing, K1 = joint_bilateral_filtering):
 * used by the roofline benchmark and the per-kernel parity tests */
int kde_jbf_presmooth_batch(kde_jbf* h, int n, const uint8_t* bgr_dev, uint8_t* smooth_dev, void* stream);
int kde_jbf_filter_batch(kde_jbf* h, int n, const float* depth_dev, const uint8_t* guide_bgr_dev,
                         float* filtered_dev, void* stream);
/* float* getFiltered_Device() const (JointBilateralFilter.cpp:41-43): object-owned, valid until the
 * next Process or destroy */
int kde_jbf_filtered_device(kde_jbf* h, float** out);
/* float* getFiltered_Host() const (:44-46).  Unlike the reference (stale unless visualize() ran) the
 * pinned host copy is refreshed here: synchronises `stream` and copies the frames the last call wrote into the
 * object's own Filtered_Device (at most max_batch).  Results a caller directed into its own buffer
 * (filtered_dev != NULL) are not mirrored -- the object keeps no pointer to caller-owned memory. */
int kde_jbf_filtered_host(kde_jbf* h, void* stream, const float** out);
/* cv::gpu::GpuMat getSmoothImage_Device() (:47-49): object-owned packed BGR, step = 3*width */
int kde_jbf_smooth_device(kde_jbf* h, uint8_t** out);
/* the window_size^2 spatial table as uploaded to the device (calcSpatialFilter) */
int kde_jbf_spatial_table(kde_jbf* h, float* table_host, int capacity);
/* tuning knob for the LDS tile sweep (BASELINE config 3); variant -1 = built-in choice */
int kde_jbf_set_variant(kde_jbf* h, int variant);
/* which kernel kde_jbf_process / kde_jbf_filter_batch will launch for this handle's parameters and variant setting:
 * an index into kde_jbf_variant_name(); 0 = "generic-32x8-1px" (one pixel per thread, any odd window <= 31, zero sigmas).
 * Tuned kernels exist for every odd window from 3 to 31 with non-zero sigmas (23..31 read their log2(S) table from a device
 * copy the handle uploads at creation: it no longer fits the 4 KB kernel-argument block); the reference takes
 * window_size as a run-time argument (JointBilateralFilter.cu:10,18-19) */
int kde_jbf_active_variant(kde_jbf* h, int* variant);
int kde_jbf_variant_count(void);
const char* kde_jbf_variant_name(int variant);

/* ---- host-fed JBF: frames that start and end in host memory --------------------------------------------------------
 * The reference uploads each frame from cudaMallocHost buffers (main.cpp:160-163) after widening the sensor's uint16 depth
 * to float on the host (Buffer2D.cpp:18-32).  A feed takes n frames in host memory, copies them to the device in chunks of
 * chunk_frames, runs K0 + K1 on each chunk (uint16 depth is widened on the device first) and copies the results back,
 * with the copy-in of one chunk, the kernels of the next older and the copy-out of the one before that overlapped on
 * three non-blocking streams of its own over a ring of device slots.
 *
 * A feed BORROWS its kde_jbf: it reads only the handle's parameters and read-only device tables and writes its own
 * buffers, so kde_jbf_filtered_device / _filtered_host / _smooth_device still return what the last kde_jbf_* call
 * wrote.  The handle must outlive the feed, and must not be used (from any thread) while a feed call on it runs.
 * Like a handle, a feed belongs to the device that was current at creation and is not thread-safe; feeds on separate
 * handles may run concurrently from different threads.
 * Host buffers: frame f at base + f * W*H elements (depth, filtered) or base + f * W*H*3 bytes (bgr).  A buffer whose
 * first and last byte are pinned (hipHostMalloc, hipHostRegister, torch pin_memory()) is copied by DMA directly; its
 * whole extent must lie inside ONE pinned allocation.  Any other buffer is pageable and is staged by the calling thread
 * through a pinned ring the feed allocates on first use (inputs before their copy-in, outputs after their copy-out,
 * overlapping the device work on other chunks). */
enum { KDE_DEPTH_F32 = 0, KDE_DEPTH_U16 = 1 };   /* u16: millimetres, 0 = invalid (OpenNI XnDepthPixel); widened exactly */
typedef struct kde_feed_stats {
    int frames, chunks, chunk_frames;          /* of the last call                                                     */
    int inputs_staged, outputs_staged;         /* 1 = that side was pageable and went through the feed's pinned ring   */
    float wall_ms;                             /* host clock, entry to return                                          */
    float h2d_ms, compute_ms, d2h_ms;          /* sums of the per-chunk HIP-event spans on the feed's three streams   */
    size_t h2d_bytes, d2h_bytes;
} kde_feed_stats;
typedef struct kde_jbf_feed kde_jbf_feed;
/* chunk_frames in 1..65535 (the bound of kde_jbf_filter_batch); device buffers are sized on the first call */
int kde_jbf_feed_create(kde_jbf_feed** out, kde_jbf* jbf, int chunk_frames);
int kde_jbf_feed_destroy(kde_jbf_feed* f);
/* JointBilateralFilter::Process over n >= 1 frames in host memory (n is not bounded by max_batch): bit-identical to
 * kde_jbf_process_batch on the same frames.  depth_format = KDE_DEPTH_F32 (float) or KDE_DEPTH_U16 (uint16_t).
 * BLOCKING: returns once all n outputs are in filtered_host; the inputs may be reused at once.  It synchronises only the
 * feed's own streams and events, never the device or another stream.  It takes no stream and cannot be captured into a
 * graph: with kde_enh_feed_process, the only entry points of this header that are not capture-safe. */
int kde_jbf_feed_process(kde_jbf_feed* f, int n, const void* depth_host, int depth_format, const uint8_t* bgr_host,
                         float* filtered_host);
/* what the last kde_jbf_feed_process did (zeros before the first call) */
int kde_jbf_feed_last_stats(kde_jbf_feed* f, kde_feed_stats* out);

/* ============================================================================================
 * MarkovRandomField — MarkovRandomField/MarkovRandomField.{cpp,cu} (sibling filter)
 * ========================================================================================== */
typedef struct kde_mrf kde_mrf;
/* MarkovRandomField(width,height); constants MarkovRandomField.cpp:3-6 (window 5, ColorSigma 50, SmoothSigma 150);
 * pass window<=0 / negative sigmas for the defaults */
int kde_mrf_create(kde_mrf** out, int width, int height, int max_batch, int window, float color_sigma, float smooth_sigma);
int kde_mrf_destroy(kde_mrf* h);
/* void MarkovRandomField::Process(float* depth_device, cv::gpu::GpuMat color_image) (MarkovRandomField.cu:42-49) */
int kde_mrf_process_batch(kde_mrf* h, int n, const float* depth_dev, const uint8_t* bgr_dev, float* filtered_dev, void* stream);
int kde_mrf_filtered_device(kde_mrf* h, float** out);
/* float* getFiltered_Host() (MarkovRandomField.h:16; refreshed after every Process in the reference,
 * MarkovRandomField.cu:48): object-owned pinned memory, lazily copied from the object's own Filtered_Device here;
 * synchronises the stream.  Holds the frames of the last call that wrote Filtered_Device. */
int kde_mrf_filtered_host(kde_mrf* h, void* stream, const float** out);

/* ============================================================================================
 * DimensionConvertor — DimensionConvertor/DimensionConvertor.{h,cpp,cu}
 * ========================================================================================== */
typedef struct kde_dimconv kde_dimconv;
int kde_dimconv_create(kde_dimconv** out);
int kde_dimconv_destroy(kde_dimconv* h);
/* void setCameraParameters(const cv::Mat_<double> intrinsic, int width, int height) (DimensionConvertor.cpp:3-13):
 * K is the row-major 3x3 intrinsic matrix; Fx,Fy = (float)K00,K11; Cx,Cy = (int)K02,K12 (truncated) */
int kde_dimconv_set_camera(kde_dimconv* h, const double* K9, int width, int height);
/* void projectiveToReal(float* data, float3* out) (DimensionConvertor.cu:3-23); n frames */
int kde_dimconv_projective_to_real_depth(kde_dimconv* h, int n, const float* depth_dev, kde_float3* out_dev, void* stream);
/* void projectiveToReal(float3* data, float3* out) (DimensionConvertor.cu:25-33) */
int kde_dimconv_projective_to_real_points(kde_dimconv* h, int n, const kde_float3* in_dev, kde_float3* out_dev, void* stream);
/* void projectiveToRealInterp(float* data, float3* out) (DimensionConvertor.cu:44-77) */
int kde_dimconv_projective_to_real_interp(kde_dimconv* h, int n, const float* depth_dev, kde_float3* out_dev, void* stream);
/* void realToProjective(float3* data, float3* out) (DimensionConvertor.cu:35-43) */
int kde_dimconv_real_to_projective(kde_dimconv* h, int n, const kde_float3* in_dev, kde_float3* out_dev, void* stream);

/* ============================================================================================
 * Buffer2D / ArrayBuffer — ArrayBuffer/{ArrayBuffer,Buffer2D}.{h,cpp,cu}
 * ========================================================================================== */
typedef struct kde_buffer2d kde_buffer2d;
/* Buffer2D(width,height): allocates weighted_d[W*H] and zero-initialises it (Buffer2D.cpp:4-11, ArrayBuffer.cu:9-30) */
int kde_buffer2d_create(kde_buffer2d** out, int width, int height);
int kde_buffer2d_destroy(kde_buffer2d* h);
/* void insertData(float* data) (Buffer2D.cu:33-56): d = data, w = 1 */
int kde_buffer2d_insert_depth(kde_buffer2d* h, const float* depth_dev, void* stream);
/* void insertData(float2* data) (Buffer2D.cu:123-147): d = data.x, w = (float)row  [sic, :137] */
int kde_buffer2d_insert_float2(kde_buffer2d* h, const float* xy_dev, void* stream);
/* void insertData(weighted_d* data) (Buffer2D.cpp:13-15): device-to-device copy */
int kde_buffer2d_insert_weighted(kde_buffer2d* h, const kde_weighted_d* data_dev, void* stream);
/* void getDepthMap(float* out) (Buffer2D.cu:59-77) / getWeightMap (:79-94) */
int kde_buffer2d_get_depth_map(kde_buffer2d* h, float* out_dev, void* stream);
int kde_buffer2d_get_weight_map(kde_buffer2d* h, float* out_dev, void* stream);
/* void updateData(float* data) (Buffer2D.cu:97-120 -> updateWaitedDepth :13-30) */
int kde_buffer2d_update(kde_buffer2d* h, const float* depth_dev, void* stream);
/* the same for a sequence of n_frames frames (frame f at depth_dev + f*W*H), fused into one pass
 * over the buffer: the streaming temporal-fusion front end (main.cpp:86-116) */
int kde_buffer2d_update_sequence(kde_buffer2d* h, int n_frames, const float* depth_dev, void* stream);
/* weighted_d* getRawPointer() (ArrayBuffer.cpp:19-21): object-owned */
int kde_buffer2d_raw_pointer(kde_buffer2d* h, kde_weighted_d** out);

/* ============================================================================================
 * DepthAdaptiveSuperpixel — SuperpixelSegmentation/DepthAdaptiveSuperpixel.{h,cpp,cu}
 * (+ base SuperpixelSegmentation.{h,cpp}); DASP path only
 * ========================================================================================== */
typedef struct kde_dasp kde_dasp;
/* DepthAdaptiveSuperpixel(width,height) (DepthAdaptiveSuperpixel.cpp:4-8) */
int kde_dasp_create(kde_dasp** out, int width, int height);
int kde_dasp_destroy(kde_dasp* h);
/* void SetParametor(int rows, int cols, cv::Mat_<double> intrinsic) (DepthAdaptiveSuperpixel.cpp:15-39).
 * Rejects geometries the reference would index out of bounds with (KDE_ERR_INVALID):
 * width/cols >= 4, height/rows >= 4, width/(width/cols) == cols, height >= 6.
 * Zero-fills the cluster tables, the labels and the (distance, label) records (the reference leaves them uninitialised). */
int kde_dasp_set_parameters(kde_dasp* h, int rows, int cols, const double* K9);
/* void Segmentation(GpuMat color, float3* points3d, float color_sigma, float spatial_sigma,
 *                   float depth_sigma, int iteration) (DepthAdaptiveSuperpixel.cu:570-588)
 * Domain.  The sigmas are finite and do not sum to 0; iteration >= 0.  The cloud is ANY float3 image: 0 (a hole), negative,
 * +-inf, NaN and up to FLT_MAX depths, and x / y that project a centre anywhere, give what the reference's arithmetic gives,
 * bit for bit -- also where a candidate distance is +inf or NaN (the 16-way tree is then evaluated literally: a NaN neither
 * replaces nor is replaced).  iteration = 0 samples the clusters and leaves init_LD's grid (own cell, 999999.9) in the
 * records; the labels stay what the call before left, 0 after SetParametor. */
int kde_dasp_segmentation(kde_dasp* h, const uint8_t* bgr_dev, const kde_float3* points_dev,
                          float color_sigma, float spatial_sigma, float depth_sigma, int iteration, void* stream);
/* int* getLabelDevice() / superpixel* getMeanDataDevice() (SuperpixelSegmentation.cpp) + DASP members */
int kde_dasp_labels_device(kde_dasp* h, int32_t** out);
int kde_dasp_mean_device(kde_dasp* h, kde_superpixel** out);
int kde_dasp_centers_device(kde_dasp* h, kde_float3** out);
int kde_dasp_ld_device(kde_dasp* h, kde_label_distance** out);
/* Labels_Host: refreshed by a blocking copy like DepthAdaptiveSuperpixel.cu:587, but lazily */
int kde_dasp_labels_host(kde_dasp* h, void* stream, const int32_t** out);
/* meanData_Host: rows*cols records, refreshed by a blocking copy as the viewers do it (SuperpixelSegmentation.cpp:97) */
int kde_dasp_mean_host(kde_dasp* h, void* stream, const kde_superpixel** out, int* count);

/* ============================================================================================
 * EdgeRefinedSuperpixel — EdgeRefinedSuperpixel/EdgeRefinedSuperpixel.{h,cpp,cu}
 * ========================================================================================== */
typedef struct kde_ers kde_ers;
/* EdgeRefinedSuperpixel(width,height) + calcSpatialFilter (EdgeRefinedSuperpixel.cpp:9-55);
 * constants WindowSize 7, SpatialSigma 30, ColorSigma 50, DepthSigma 70 (:4-7) */
int kde_ers_create(kde_ers** out, int width, int height);
int kde_ers_destroy(kde_ers* h);
/* void EdgeRefining(int* color_label_device, int* depth_label_device, float* depth_device,
 *                   cv::gpu::GpuMat color_image) (EdgeRefinedSuperpixel.cu:208-223).
 * Labels are what the segmenters write: -1 (unassigned) or a superpixel index in [0, width * height).
 * Depth domain as for kde_jbf_process (+inf / > 2^64 samples: kde_ers_set_variant(h, 3) reproduces the reference). */
int kde_ers_edge_refining(kde_ers* h, const int32_t* color_labels_dev, const int32_t* depth_labels_dev,
                          const float* depth_dev, const uint8_t* bgr_dev, void* stream);
/* (no reference counterpart) which depthmap_enhancement kernel serves the handle: 0 = built-in choice,
 * 1 = packed-pair kernel (labels are superpixel indices, exact as floats for frames of <= 2^24 pixels),
 * 2 = scalar tuned kernel, 3 = generic kernels (any-window depthmap_enhancement, and edge_refining as two
 * launches on global memory instead of the fused LDS kernel).  For A/B measurements and the per-kernel parity tests. */
int kde_ers_set_variant(kde_ers* h, int variant);
/* the two kernels individually, for per-kernel parity tests:
 * edge_refining (.cu:4-102; snapshot semantics) on the object-owned label/depth copies,
 * leaving its result readable through kde_ers_stage_* ; depthmap_enhancement (.cu:104-205; D3) */
int kde_ers_stage_edge_depth_device(kde_ers* h, float** out);
int kde_ers_refined_labels_device(kde_ers* h, int32_t** out);    /* getRefinedLabels_Device (EdgeRefinedSuperpixel.cpp:56-58) */
int kde_ers_refined_depth_device(kde_ers* h, float** out);       /* getRefinedDepth_Device  (:63-65)                         */
int kde_ers_refined_labels_host(kde_ers* h, void* stream, const int32_t** out); /* getRefinedLabels_Host (:59-62) */
int kde_ers_refined_depth_host(kde_ers* h, void* stream, const float** out);    /* getRefinedDepth_Host  (:66-69) */

/* ============================================================================================
 * RegionGrowingBilateralFilter — RegionGrowingBilateralFilter.{h,cpp}
 * ========================================================================================== */
typedef struct kde_rgbf kde_rgbf;
int kde_rgbf_create(kde_rgbf** out, int width, int height);                       /* .cpp:5-11  */
int kde_rgbf_destroy(kde_rgbf* h);                                                /* .cpp:12-20 */
int kde_rgbf_set_parameters(kde_rgbf* h, int rows, int cols, const double* K9);   /* SetParametor, .cpp:21-26 */
/* void Process(float* depth_device, float3* points_device, cv::gpu::GpuMat color_device) (.cpp:27-38):
 * SP->Segmentation(200,40,0,1); DASP->Segmentation(100,20,200,1); ERS->EdgeRefining(SP labels, DASP labels, ...) */
int kde_rgbf_process(kde_rgbf* h, const float* depth_dev, const kde_float3* points_dev,
                     const uint8_t* bgr_dev, void* stream);
/* A batch of independent frames (the unit north_star shards across GPUs; the reference has only the single-frame call):
 * kde_rgbf_create_batch sizes the object's buffers for max_batch frames, kde_rgbf_process_batch runs Process on n <=
 * max_batch frames laid out back to back -- every kernel of the chain takes the whole batch in one launch, and each
 * frame's labels and refined depth are bit-identical to its single-frame kde_rgbf_process.  The getters then return
 * n frames back to back (frame f at + f * W*H). */
int kde_rgbf_create_batch(kde_rgbf** out, int width, int height, int max_batch);
int kde_rgbf_process_batch(kde_rgbf* h, int n, const float* depth_dev, const kde_float3* points_dev,
                           const uint8_t* bgr_dev, void* stream);
int kde_rgbf_refined_depth_device(kde_rgbf* h, float** out);                       /* .cpp:39-41 */
int kde_rgbf_refined_depth_host(kde_rgbf* h, void* stream, const float** out);     /* .cpp:42-44 */
int kde_rgbf_refined_labels_device(kde_rgbf* h, int32_t** out);
int kde_rgbf_sp_labels_device(kde_rgbf* h, int32_t** out);
int kde_rgbf_dasp_labels_device(kde_rgbf* h, int32_t** out);

/* ============================================================================================
 * SPDepthSuperResolution — SPDepthSuperResolution.{h,cpp}: class surface named by the north star.
 * Process = .cpp:57-191: SP(200,10,0,5), DASP(0,10,200,5), ERS, projectiveToReal, per-superpixel plane fit
 * (the reference's host cv::PCA loop, here on the device) and Projection_GPU::PlaneProjection(nd, labels,
 * points) (Projection_GPU/Projection_GPU.cu:55-81, 148-187, 274-294; 20 sweeps, snapshot semantics D5).
 * ========================================================================================== */
typedef struct kde_spdsr kde_spdsr;
int kde_spdsr_create(kde_spdsr** out, int width, int height);
int kde_spdsr_destroy(kde_spdsr* h);
int kde_spdsr_set_parameters(kde_spdsr* h, int rows, int cols, const double* K9);
int kde_spdsr_process(kde_spdsr* h, const float* depth_dev, const kde_float3* points_dev,
                      const uint8_t* bgr_dev, void* stream);
/* batched form, as kde_rgbf_process_batch: head (labels, refined depth, edge-enhanced points) bit-identical per frame;
 * the plane fit accumulates double-precision moments with atomics, so the tail agrees with the single-frame call to
 * the same 1e-4 it agrees with itself from run to run.  ClusterND: n tables of rows*cols float4 back to back. */
int kde_spdsr_create_batch(kde_spdsr** out, int width, int height, int max_batch);
int kde_spdsr_process_batch(kde_spdsr* h, int n, const float* depth_dev, const kde_float3* points_dev,
                            const uint8_t* bgr_dev, void* stream);
int kde_spdsr_refined_depth_device(kde_spdsr* h, float** out);
int kde_spdsr_refined_depth_host(kde_spdsr* h, void* stream, const float** out);
int kde_spdsr_refined_labels_device(kde_spdsr* h, int32_t** out);
int kde_spdsr_edge_enhanced_points_device(kde_spdsr* h, kde_float3** out);         /* EdgeEnhanced3DPoints_Device */
int kde_spdsr_optimized_points_device(kde_spdsr* h, kde_float3** out);             /* getOptimizedPoints_Device (Projection_GPU.cpp:62-64) */
int kde_spdsr_optimized_points_host(kde_spdsr* h, void* stream, const kde_float3** out); /* getOptimizedPoints_Host (:59-61) */
int kde_spdsr_plane_fitted_points_device(kde_spdsr* h, kde_float3** out);         /* Projection_GPU::GetPlaneFitted3D_Device (:56-58) */
int kde_spdsr_cluster_nd_device(kde_spdsr* h, float** out);                       /* ClusterND_Device: float4 {normal, distance} per cluster */

/* ============================================================================================
 * NormalMapGenerator — NormalEstimation/NormalMapGenerator.{h,cpp,cu} with SmoothingAreaMapGenerator and
 * IntegralImageGenerator: per-pixel surface normals of packed kde_float3 points in millimetres (as
 * kde_dimconv_projective_to_real_depth writes them).  A bad point is (-1,-1,-1).  Any W x H, batched, asynchronous on the
 * caller's stream with no host synchronisation and no allocation, so kde_normals_generate_batch can be captured into a
 * graph.  Definitions N1 / N2 (neighbours by linear index, windows that leave the frame) are in DESIGN.md.
 * ========================================================================================== */
typedef struct kde_normals kde_normals;
enum { KDE_NORMALS_SDC = 0, KDE_NORMALS_CM = 1, KDE_NORMALS_BILATERAL = 2 };   /* NormalMapGenerator.h:28 */
typedef struct kde_normals_params {
    int method;                     /* normal_estimation_method_ = BILATERAL  NormalMapGenerator.cpp:15 */
    float max_depth_change_factor;  /* max_depth_change_factor_ = 0.05f       SmoothingAreaMapGenerator.cpp:15 */
    float normal_smoothing_size;    /* normal_smoothing_size_ = 20.0f         SmoothingAreaMapGenerator.cpp:16 */
} kde_normals_params;
/* fills the reference's defaults: BILATERAL, 0.05f, 20.0f */
int kde_normals_default_params(kde_normals_params* p);
/* NormalMapGenerator(int w, int h) (NormalMapGenerator.cpp:11-17).  p == NULL -> defaults.  max_batch >= 1 sizes the
 * object-owned maps.  method SDC -> KDE_ERR_UNSUPPORTED; max_depth_change_factor must be finite and
 * normal_smoothing_size finite in [-1e6, 1e6] */
int kde_normals_create(kde_normals** out, int width, int height, int max_batch, const kde_normals_params* p);
/* NormalMapGenerator::~NormalMapGenerator (NormalMapGenerator.cpp:19-23) */
int kde_normals_destroy(kde_normals* h);
/* void setNormalEstimationMethods(int method) (NormalMapGenerator.cpp:35-37): CM or BILATERAL; SDC -> KDE_ERR_UNSUPPORTED */
int kde_normals_set_method(kde_normals* h, int method);
/* void generateNormalMap(float3* vertices_device) (NormalMapGenerator.cu:513-524) over n <= max_batch frames;
 * normals_dev == NULL writes the object-owned normal map */
int kde_normals_generate_batch(kde_normals* h, int n, const kde_float3* points_dev,
                               kde_float3* normals_dev /* NULL: object-owned */, void* stream);
/* float3* getNormalMap() (NormalMapGenerator.cpp:47-49): object-owned, n frames of the last call that wrote it */
int kde_normals_normal_map_device(kde_normals* h, kde_float3** out);
/* host copy of the object-owned normal map (what getNormalImg copies down, NormalMapGenerator.cu:423-426): pinned,
 * lazily copied on `stream`, which is synchronised */
int kde_normals_normal_map_host(kde_normals* h, void* stream, const kde_float3** out);
/* SmoothingAreaMapGenerator::getFinalSmoothingMap (SmoothingAreaMapGenerator.cpp:51-53): object-owned, the frames of the
 * last call if it ran CM, else KDE_ERR_INVALID (BILATERAL builds no smoothing map) */
int kde_normals_smoothing_map_device(kde_normals* h, float** out);

/* ============================================================================================
 * NormalAdaptiveSuperpixel — SuperpixelSegmentation/NormalAdaptiveSuperpixel.{h,cpp,cu} (+ the DepthAdaptiveSuperpixel
 * base): superpixels on colour, position, depth and surface normal; the consumer of NormalMapGenerator's output in
 * KinectDepthEnhancement.cpp:65-67.  Points are packed kde_float3 in millimetres, a bad normal is (-1,-1,-1).  Batched,
 * asynchronous on the caller's stream, no allocation after kde_nasp_set_parameters.  Definition and the deviations
 * NA1-NA5 are in DESIGN.md ("Normal-adaptive superpixels"); every output is bit-identical to tools/nasp_ref.c.
 * ========================================================================================== */
typedef struct kde_nasp kde_nasp;
/* NormalAdaptiveSuperpixel(width,height) (NormalAdaptiveSuperpixel.cpp:4-8); max_batch >= 1 sizes the object's buffers */
int kde_nasp_create(kde_nasp** out, int width, int height, int max_batch);
int kde_nasp_destroy(kde_nasp* h);                                                 /* ~NormalAdaptiveSuperpixel (.cpp:9-17) */
/* void SetParametor(int rows, int cols, cv::Mat_<double> intrinsic) (inherited, DepthAdaptiveSuperpixel.cpp:15-39; initMemory
 * NormalAdaptiveSuperpixel.cpp:19-37).  Zero-fills mean, centres, normals, variance and LD (NA5).  KDE_ERR_INVALID for
 * geometries the reference would index out of bounds: width/cols >= 8, height/rows >= 8 (the 8 x 8 candidates),
 * width/(width/cols) == cols, height >= 6. */
int kde_nasp_set_parameters(kde_nasp* h, int rows, int cols, const double* K9);
/* void Segmentation(GpuMat color, float3* points3d, float3* normals, float color_sigma, float spatial_sigma,
 *                   float depth_sigma, float normal_sigma, int iteration) (NormalAdaptiveSuperpixel.cu:1070-1103).
 * The weights of the weighted-average pass are host-built tables keyed by (color_sigma, spatial_sigma): a call whose two
 * sigmas differ from the previous call's rebuilds and uploads them on `stream`; such a call is refused with
 * KDE_ERR_UNSUPPORTED while `stream` is capturing (call once with the same sigmas first), as is a spatial_sigma whose
 * table would not fit (weight still non-zero after 2^20 entries on a window larger than that).  iteration >= 0; with
 * iteration = 0 the cluster tables hold the sampled clusters, LD the initial grid (own cell, 999999.9) and the labels are not
 * written, as in the reference. */
int kde_nasp_segmentation(kde_nasp* h, const uint8_t* bgr_dev, const kde_float3* points_dev, const kde_float3* normals_dev,
                          float color_sigma, float spatial_sigma, float depth_sigma, float normal_sigma, int iteration,
                          void* stream);
/* the same over n <= max_batch frames back to back; frame f's result is bit-identical to its single-frame call */
int kde_nasp_segmentation_batch(kde_nasp* h, int n, const uint8_t* bgr_dev, const kde_float3* points_dev,
                                const kde_float3* normals_dev, float color_sigma, float spatial_sigma, float depth_sigma,
                                float normal_sigma, int iteration, void* stream);
/* object-owned device buffers, the frames of the last call back to back */
int kde_nasp_labels_device(kde_nasp* h, int32_t** out);                 /* getLabelDevice (SuperpixelSegmentation.cpp)       */
int kde_nasp_mean_device(kde_nasp* h, kde_superpixel** out);            /* getMeanDataDevice                                 */
int kde_nasp_centers_device(kde_nasp* h, kde_float3** out);             /* getCentersDevice (NormalAdaptiveSuperpixel.h:23)  */
int kde_nasp_normals_device(kde_nasp* h, kde_float3** out);             /* getNormalsDevice (:25)                            */
int kde_nasp_normals_variance_device(kde_nasp* h, float** out);         /* getNormalsVarianceDevice (:27)                    */
int kde_nasp_ld_device(kde_nasp* h, kde_label_distance** out);          /* LD_Device                                         */
/* pinned host copies, refreshed lazily by a blocking copy on `stream` (the reference copies after every Segmentation,
 * .cu:1097-1101): the only calls that synchronise.  count = records returned (rows*cols per frame of the last call) */
int kde_nasp_labels_host(kde_nasp* h, void* stream, const int32_t** out);                              /* Labels_Host */
int kde_nasp_mean_host(kde_nasp* h, void* stream, const kde_superpixel** out, int* count);             /* meanData_Host */
int kde_nasp_centers_host(kde_nasp* h, void* stream, const kde_float3** out, int* count);              /* getCentersHost (:22) */
int kde_nasp_normals_host(kde_nasp* h, void* stream, const kde_float3** out, int* count);              /* getNormalsHost (:24) */
int kde_nasp_normals_variance_host(kde_nasp* h, void* stream, const float** out, int* count);          /* getNormalsVarianceHost (:26) */

/* ============================================================================================
 * LabelEquivalenceSeg — LabelEquivalenceSeg/LabelEquivalenceSeg.{h,cpp,cu}: merges 4-adjacent superpixels whose plane
 * parameters are similar (angle between normals below max_angle, plane distances within max_plane_distance) by label
 * equivalence, then gives every merged region an averaged plane (n, d), a size and a normal-agreement "variance"; the
 * consumer of NormalAdaptiveSuperpixel's four cluster outputs in KinectDepthEnhancement.cpp:76.  Batched, asynchronous on
 * the caller's stream, capturable, no allocation and no host synchronisation after kde_les_create.  Definition and the
 * deviations L1-L7 are in DESIGN.md ("Superpixel merging"); every output is bit-identical to tools/les_ref.c.
 * n_clusters is the length of the per-superpixel tables (the reference class sizes everything W*H and cannot know it):
 * 1 <= n_clusters <= min(W*H, 2048); a larger count is refused with KDE_ERR_INVALID (the graph step keeps its tables in
 * LDS and the adjacency takes n_clusters^2 bits per frame).  A label outside [0, n_clusters) is a pixel without superpixel.
 * ========================================================================================== */
typedef struct kde_les kde_les;
typedef struct kde_float4 { float x, y, z, w; } kde_float4;         /* CUDA float4, 16 B                  */
typedef struct kde_les_params {
    int   iterations;               /* 10 rounds of scan + analysis      LabelEquivalenceSeg.cu:235 (>= 0)            */
    float max_angle;                /* 3.141592653f / 8.0f radians       :40                                          */
    float max_plane_distance;       /* 150.0f millimetres                :42                                          */
} kde_les_params;
/* fills the reference's constants: 10, 3.141592653f / 8.0f, 150.0f */
int kde_les_default_params(kde_les_params* p);
/* LabelEquivalenceSeg(int width, int height) (LabelEquivalenceSeg.cpp:7-38).  p == NULL -> defaults; max_batch >= 1
 * sizes the object-owned buffers.  iterations >= 0; max_angle and max_plane_distance must not be NaN */
int kde_les_create(kde_les** out, int width, int height, int max_batch, const kde_les_params* p);
int kde_les_destroy(kde_les* h);                                    /* ~LabelEquivalenceSeg (.cpp:41-59) */
/* void labelImage(float3* cluster_normals_device, int* cluster_label_device, float3* cluster_centers_device,
 *                 float* variance_device) (LabelEquivalenceSeg.cu:228-282).  variance_dev is dead in the reference (its only
 * use is commented out, :82): kept for the signature, may be NULL, never read */
int kde_les_label_image(kde_les* h, const kde_float3* normals_dev, const int32_t* labels_dev, const kde_float3* centers_dev,
                        const float* variance_dev, int n_clusters, void* stream);
/* the same over n <= max_batch frames back to back: labels [n][H][W], per-superpixel inputs [n][n_clusters] (as
 * NormalAdaptiveSuperpixel lays its outputs out); frame f's result is bit-identical to its single-frame call */
int kde_les_label_image_batch(kde_les* h, int n, const kde_float3* normals_dev, const int32_t* labels_dev,
                              const kde_float3* centers_dev, const float* variance_dev, int n_clusters, void* stream);
/* object-owned device buffers, the frames of the last call back to back */
int kde_les_merged_label_device(kde_les* h, int32_t** out);         /* getMergedClusterLabel_Device (.cpp:128): [n][H][W], -1 = none */
int kde_les_merged_nd_device(kde_les* h, kde_float4** out);         /* getMergedClusterND_Device (.cpp:125): [n][H][W], 0 where label -1 */
/* indexed by merged label, n_clusters entries per frame of the last call, 0 for labels that are nobody's merged label */
int kde_les_merged_variance_device(kde_les* h, float** out);        /* getMergedClusterVariance_Device (.cpp:137) */
int kde_les_merged_size_device(kde_les* h, int32_t** out);          /* getMergedClusterSize_Device (.cpp:143)     */
/* pinned host copies, refreshed lazily by a blocking copy on `stream` (the reference copies the labels after every
 * labelImage, .cu:278): the only calls that synchronise */
int kde_les_merged_label_host(kde_les* h, void* stream, const int32_t** out);       /* getMergedClusterLabel_Host (.cpp:134) */
int kde_les_merged_nd_host(kde_les* h, void* stream, const kde_float4** out);       /* getMergedClusterND_Host (.cpp:131)    */

/* ============================================================================================
 * Projection_GPU — Projection_GPU/Projection_GPU.{h,cpp,cu}, the five-argument PlaneProjection (.cu:248-272): every pixel
 * of a region whose normals agree (acos(variance) < max_angle) is projected along its ray onto the region's plane; where
 * the region is also larger than min_size and the projected depth is within 3 % of the measured one, the depth is replaced
 * by (within 1 %) or blended with (by the variance) the projected one; a window_size^2 depth-bilateral filter smooths the
 * result.  The consumer of LabelEquivalenceSeg's four outputs in KinectDepthEnhancement.cpp:79-80.  Batched, asynchronous
 * on the caller's stream, capturable, no allocation and no host synchronisation after kde_proj_create.  Definition and the
 * deviations P1-P5 are in DESIGN.md ("Plane projection (five-argument)"); the checker is tools/proj_ref.c.
 * (kde_spdsr_* holds the three-argument overload, which runs inside SPDepthSuperResolution::Process.)
 * ========================================================================================== */
typedef struct kde_proj kde_proj;
typedef struct kde_proj_params {
    int   window_size;              /* WindowSize = 7      Projection_GPU.cpp:4  (odd, 1..15)                          */
    float spatial_sigma;            /* SpatialSigma = 20   :3  (pixels, not 0 and not NaN)                             */
    float depth_sigma;              /* DepthSigma = 100    :5  (millimetres, > 0)                                      */
    float max_angle;                /* 3.141592653f / 8.0f radians   Projection_GPU.cu:38, :203                        */
    int   min_size;                 /* 1300 pixels: a region counts as large when size > min_size   .cu:203            */
} kde_proj_params;
/* fills the reference's constants: 7, 20, 100, 3.141592653f / 8.0f, 1300 */
int kde_proj_default_params(kde_proj_params* p);
/* Projection_GPU(int width, int height, const cv::Mat intrinsic) (Projection_GPU.cpp:7-21): K9 is the row-major 3x3
 * intrinsic matrix, Fx,Fy = (float)K00,K11; Cx,Cy = (int)K02,K12 (truncated).  Builds the unit-depth rays (initTemp,
 * .cu:3-19) and the spatial table (calcSpatialFilter, .cpp:35-44) once.  params == NULL -> defaults; max_batch >= 1 sizes
 * the object-owned buffers. */
int kde_proj_create(kde_proj** out, int width, int height, int max_batch, const double* K9, const kde_proj_params* params);
int kde_proj_destroy(kde_proj* h);                                  /* ~Projection_GPU (.cpp:23-33) */
/* void PlaneProjection(const float4* nd_device, const int* labels_device, const float* variance_device,
 *                      const float3* points3d_device, int* size_device) (.cu:248-272).  nd and labels are per pixel,
 * variance and size are tables of n_clusters >= 1 entries indexed by label: what the four kde_les_merged_*_device getters
 * return.  A label outside [0, n_clusters) is a pixel without region. */
int kde_proj_plane_projection(kde_proj* h, const kde_float4* nd_dev, const int32_t* labels_dev, const float* variance_dev,
                              const kde_float3* points_dev, const int32_t* size_dev, int n_clusters, void* stream);
/* the same over n <= max_batch frames back to back: per-pixel inputs [n][H][W], tables [n][n_clusters]; frame f's result is
 * bit-identical to its single-frame call */
int kde_proj_plane_projection_batch(kde_proj* h, int n, const kde_float4* nd_dev, const int32_t* labels_dev,
                                    const float* variance_dev, const kde_float3* points_dev, const int32_t* size_dev,
                                    int n_clusters, void* stream);
/* object-owned, the frames of the last call back to back; the host copies are pinned and refreshed lazily by a blocking
 * copy on `stream` (the reference's copies are commented out, .cu:269-270): the only calls that synchronise */
int kde_proj_optimized_points_device(kde_proj* h, kde_float3** out);                        /* GetOptimized3D_Device (.cpp:62-64)   */
int kde_proj_optimized_points_host(kde_proj* h, void* stream, const kde_float3** out);      /* GetOptimized3D_Host (:59-61)         */
int kde_proj_plane_fitted_points_device(kde_proj* h, kde_float3** out);                     /* GetPlaneFitted3D_Device (:56-58)     */
int kde_proj_plane_fitted_points_host(kde_proj* h, void* stream, const kde_float3** out);   /* GetPlaneFitted3D_Host (:52-54)       */

/* ============================================================================================
 * KinectDepthEnhancement — KinectDepthEnhancement.{h,cpp}: the reference's "PROPOSED" method (main.cpp:198-202).
 * Process = .cpp:56-81: JointBilateralFilter (defaults), projectiveToReal(float*), NormalMapGenerator (CM),
 * NormalAdaptiveSuperpixel::Segmentation(10, 50, 50, 150, 1), LabelEquivalenceSeg::labelImage with rows*cols superpixels
 * and the five-argument PlaneProjection (defaults).  Composition only: every stage is the object above, and each output
 * is bit-identical to the six stage objects called by hand.  Not built: the two cv::imwrite calls (:69, :77), and
 * getRefinedDepth_Device / _Host (:82-87), which return a buffer of the EdgeRefinedSuperpixel member that Process never
 * writes.
 * ========================================================================================== */
typedef struct kde_enh kde_enh;
/* KinectDepthEnhancement(int width, int height) (.cpp:11-24); max_batch >= 1 sizes every stage */
int kde_enh_create(kde_enh** out, int width, int height, int max_batch);
int kde_enh_destroy(kde_enh* h);                                    /* ~KinectDepthEnhancement (.cpp:25-45) */
/* void SetParametor(int rows, int cols, cv::Mat_<double> intrinsic) (.cpp:46-55).  Refuses what kde_nasp_set_parameters
 * refuses, and rows*cols > min(W*H, 2048), the kde_les_label_image bound.  Builds NormalAdaptiveSuperpixel's weight tables
 * for Process's sigmas, so kde_enh_process_batch can be captured from the first call. */
int kde_enh_set_parameters(kde_enh* h, int rows, int cols, const double* K9);
/* void Process(float* depth_device, cv::gpu::GpuMat color_device) (.cpp:56-81) over n <= max_batch frames back to back */
int kde_enh_process_batch(kde_enh* h, int n, const float* depth_dev, const uint8_t* bgr_dev, void* stream);
/* object-owned, the frames of the last call back to back */
int kde_enh_optimized_points_device(kde_enh* h, kde_float3** out);                          /* getOptimizedPoints_Device (.cpp:88-90) */
int kde_enh_optimized_points_host(kde_enh* h, void* stream, const kde_float3** out);        /* getOptimizedPoints_Host (:91-93)       */
int kde_enh_nasp_labels_device(kde_enh* h, int32_t** out);          /* NASP->getLabelDevice()                       */
int kde_enh_merged_labels_device(kde_enh* h, int32_t** out);        /* spMerging->getMergedClusterLabel_Device()    */
int kde_enh_edge_enhanced_points_device(kde_enh* h, kde_float3** out);   /* EdgeEnhanced3DPoints_Device             */

/* ---- depth output: the enhanced cloud as a depth map --------------------------------------------------------------
 * The reference's result is a point cloud (getOptimizedPoints_Host, main.cpp:198-202) although its input is the sensor's
 * depth map (uint16 millimetres, 0 = invalid, widened on the host and uploaded, main.cpp:160-163).  kde_points_to_depth writes the z of
 * n_points packed points as a depth map.  Stateless, on the current device, asynchronous on `stream`, capture-safe.
 *   KDE_DEPTH_F32  out[i] = points[i].z, the bits unchanged (NaNs included)
 *   KDE_DEPTH_U16  r = rintf(z) (round half to even); out[i] = (r >= 1 && r <= 65535) ? (uint16_t)r : 0.  NaN, +-inf,
 *                  z < 0.5 and z >= 65535.5 give 0, the sensor's "invalid"; every integer z in 1..65535 is returned as it
 *                  is, so this is the exact inverse of the widening a feed applies to uint16 depth.
 * n_points == 0 is KDE_OK and launches nothing.  KDE_ERR_INVALID: a null pointer with n_points > 0, an unknown format,
 * points_dev or a float output not 4-byte aligned, a uint16 output not 2-byte aligned.  Pointers that are both 16-byte
 * aligned take the vector kernels; any other alignment is served by scalar ones. */
enum { KDE_OUT_POINTS_F32 = 0, KDE_OUT_DEPTH_F32 = 1, KDE_OUT_DEPTH_U16 = 2 };   /* out_format of kde_enh_feed_process */
int kde_points_to_depth(size_t n_points, const kde_float3* points_dev, int depth_format /* KDE_DEPTH_F32 | KDE_DEPTH_U16 */,
                        void* depth_dev, void* stream);

/* ---- host-fed KinectDepthEnhancement: frames that start and end in host memory --------------------------------------
 * Process (main.cpp:198-202) on n frames in host memory, the upload of main.cpp:160-163 and the uint16 widening
 * included: the contract of kde_jbf_feed_* above (n >= 1 not bounded by max_batch; pinned or pageable buffers, detected
 * per call, pageable ones staged through a pinned ring; BLOCKING; synchronises only the feed's own three streams and
 * events; not capture-safe; one device, not thread-safe), with these differences:
 *   - chunk_frames must lie in 1..max_batch of the kde_enh: each chunk is one kde_enh_process_batch.
 *   - the feed borrows the kde_enh and RUNS it: per chunk, on the feed's compute stream, the uint16 widening (if any),
 *     kde_enh_process_batch on the slot's buffers, then the output step into the slot.  The kde_enh_* getters afterwards
 *     show the LAST CHUNK of the last call.  The kde_enh must outlive the feed and must not be used while a call runs;
 *     a kde_enh whose SetParametor was not called makes kde_enh_feed_process return that object's own refusal.
 *   - out_format selects what comes back, frame f at out_host + f * W*H elements:
 *       KDE_OUT_POINTS_F32  kde_float3 (12 B): the optimized points (getOptimizedPoints_Host of every frame)
 *       KDE_OUT_DEPTH_F32   float (4 B), KDE_OUT_DEPTH_U16  uint16_t (2 B): kde_points_to_depth of them
 *     The copy-out reads only the slot, so the next chunk's kernels may overwrite the object's buffers meanwhile.
 *   - stats: d2h_bytes = W*H*n * {12, 4, 2}, h2d_bytes = W*H*n * (depth element size + 3).
 * Every result is bit-identical to kde_enh_process_batch on the same frames followed by kde_points_to_depth.  On failure
 * the three streams are synchronised before the call returns: nothing stays in flight into the caller's memory. */
typedef struct kde_enh_feed kde_enh_feed;
int kde_enh_feed_create(kde_enh_feed** out, kde_enh* enh, int chunk_frames);
int kde_enh_feed_destroy(kde_enh_feed* f);
int kde_enh_feed_process(kde_enh_feed* f, int n, const void* depth_host, int depth_format, const uint8_t* bgr_host,
                         int out_format, void* out_host);
/* what the last kde_enh_feed_process did (zeros before the first call) */
int kde_enh_feed_last_stats(kde_enh_feed* f, kde_feed_stats* out);

/* ============================================================================================
 * MeanError3D — the reference's quality figure (main.cpp:220-308): the mean 3-D distance of each method's cloud from the
 * cloud of the temporally averaged depth, over the pixels where both are valid.  One call compares m <= 8 candidate
 * results with one ground truth for n frames on the device and leaves a table of (sum, count, mean) per frame and
 * candidate.  For a candidate point p and the truth point t of the same pixel:
 *   valid  iff p.z > z_min && p.z < z_max && t.z > z_min && t.z < z_max (both ends exclusive; NaN and +-inf are invalid;
 *          defaults 50 and 15000, main.cpp:227-238)
 *   term   dz = p.z - t.z, dy = p.y - t.y, dx = p.x - t.x; e = sqrtf((dz*dz + dy*dy) + dx*dx) in float32, no fused
 *          multiply-add, correctly rounded sqrtf (main.cpp:240-242).  Nothing else is special: a valid z with a NaN x gives
 *          a NaN term, which reaches the sum as it would in the reference.
 *   count  the number of valid pixels; sum = the sum of their terms in BINARY64 in a fixed order;
 *          mean = (float)(sum / (double)count), NaN when count == 0 like the reference's 0.0f / 0 (main.cpp:304-308).
 * The reference accumulates in float32 in raster order (exact only to about count * 2^-24, and no parallel order can
 * reproduce it); the binary64 sum here is within count * 2^-53 of the exact sum, and the table is deterministic to the bit:
 * it does not depend on n, m, a frame's position in the batch, a candidate's position among the m, or pointer alignment.
 * A source is a cloud or a depth map; a depth map (float, or uint16 widened by (float)u) stands for the cloud that
 * projectiveToReal(float*) makes of it with the object's camera, and gives the bits the float3 source of that cloud gives.
 * ========================================================================================== */
enum { KDE_SRC_POINTS_F32 = 0, KDE_SRC_DEPTH_F32 = 1, KDE_SRC_DEPTH_U16 = 2 };
typedef struct kde_error3d_source { const void* data_dev; int format; } kde_error3d_source;   /* [frames][H][W] of float3 / float / uint16 */
typedef struct kde_error3d_result { double sum; uint32_t count; float mean; } kde_error3d_result;   /* 16 bytes */
typedef struct kde_error3d kde_error3d;
/* the accumulators of the loop main.cpp:220-308 (declared at :217-218) for max_batch frames x max_candidates (1..8)
 * methods, on the current device.  On a
 * host without a device the object is created without buffers: every call validates as usual and
 * kde_error3d_compare_batch then returns KDE_ERR_HIP. */
int kde_error3d_create(kde_error3d** out, int width, int height, int max_batch, int max_candidates);
int kde_error3d_destroy(kde_error3d* h);   /* main.cpp:220-308 keeps its accumulators on the stack; NULL is a no-op */
/* the camera a depth-map source is projected with (main.cpp:220-308 reads clouds made by convertor.projectiveToReal, :168):
 * fx, fy as float, cx, cy truncated to int, like kde_dimconv_set_camera.  Needed only when a source is a depth map. */
int kde_error3d_set_camera(kde_error3d* h, const double* K9);
/* the validity range of main.cpp:220-308 (its literals 50.0f and 15000.0f): finite, z_min < z_max */
int kde_error3d_set_range(kde_error3d* h, float z_min, float z_max);
/* the loop of main.cpp:220-308 for n <= max_batch frames and m <= max_candidates candidates against one truth:
 * `candidates` is a HOST array of m descriptors, read at call time (they travel as kernel arguments); truth_frames == 1
 * compares every frame with the same truth frame, truth_frames == n frame f with truth frame f.  Pointers need the
 * alignment of their element only (4 bytes for float3 and float, 2 for uint16); frames that start on 16-byte boundaries
 * are read with 16-byte loads.  A depth-map source before kde_error3d_set_camera is KDE_ERR_INVALID.  Two launches, no
 * allocation, no host synchronisation, no upload: capturable like kde_enh_process_batch. */
int kde_error3d_compare_batch(kde_error3d* h, int n, int m, const kde_error3d_source* candidates,
                              const kde_error3d_source* truth, int truth_frames, void* stream);
/* the five averages of main.cpp:220-308 and what they were divided from: object-owned, [n][m] of the last call, valid until
 * the next call or destroy.  KDE_ERR_INVALID before the first call. */
int kde_error3d_results_device(kde_error3d* h, kde_error3d_result** out);
/* the same in pinned host memory after a blocking copy on `stream` (main.cpp:220-308 computes on the host): synchronises,
 * like the other *_host getters */
int kde_error3d_results_host(kde_error3d* h, void* stream, const kde_error3d_result** out);

/* ==========================================================================================
 * PointCloudXYZRGB: the output step of main.cpp:211-300 on the device -- a method's organised float3 grid (millimetres) and
 * the colour image become the coloured cloud the reference pushes into a pcl::PointCloud<pcl::PointXYZRGB>, for a batch of
 * frames.  For pixel i in raster order with point p and colour bytes (b, g, r):
 *   valid   iff p.z > z_min && p.z < z_max (both ends exclusive; NaN and +-inf are invalid)
 *   record  x = p.x / divisor, y = p.y / divisor, z = negate_z ? -(p.z / divisor) : p.z / divisor (correctly rounded float
 *           divisions), rgb = (r << 16) | (g << 8) | b: PCL's packed rgb, and the payload of a binary PCD file with
 *           FIELDS x y z rgb
 *   dense mode (organized == 0, what the reference does): the valid records of frame f, in raster order, are the first
 *           count[f] records of the frame's slot, which starts at record f * W * H; the rest of the slot is NOT written
 *   organised mode: W * H records per frame; an invalid pixel has x = y = z = NaN (0x7fc00000) and keeps its colour
 * A source is what kde_error3d_source describes; a depth map gives the bytes the float3 source of its cloud gives.
 * ========================================================================================== */
typedef struct kde_cloud_point { float x, y, z; uint32_t rgb; } kde_cloud_point;             /* 16 bytes */
typedef struct kde_cloud_params { float z_min, z_max, divisor; int negate_z; int organized; } kde_cloud_params;
typedef struct kde_cloud kde_cloud;
/* the literals of main.cpp:211-300: z_min 50, z_max 15000, divisor 1000, negate_z 1; organized 0 */
int kde_cloud_default_params(kde_cloud_params* p);
/* the clouds of main.cpp:211-300 (declared at :211-216) for max_batch frames on the current device; p == NULL: the defaults.
 * z_min, z_max finite with z_min < z_max, divisor finite and > 0.  The object owns max_batch * W * H records for calls with
 * out_dev == NULL.  On a host without a device the object is created without buffers: every call validates as usual and
 * kde_cloud_build_batch then returns KDE_ERR_HIP. */
int kde_cloud_create(kde_cloud** out, int width, int height, int max_batch, const kde_cloud_params* p);
int kde_cloud_destroy(kde_cloud* h);   /* main.cpp:211-300 holds its clouds in shared pointers; NULL is a no-op */
/* the camera a depth-map source is projected with (main.cpp:211-300 reads clouds made by convertor.projectiveToReal, :168),
 * as kde_error3d_set_camera.  Needed only when the source is a depth map. */
int kde_cloud_set_camera(kde_cloud* h, const double* K9);
/* the loop of main.cpp:211-300 for n <= max_batch frames of one method: `src` is a HOST descriptor read at call time;
 * bgr_dev is [bgr_frames][H][W][3] with bgr_frames == 1 (one image for every frame) or n; out_dev is [n][W * H] records on a
 * 16-byte boundary, or NULL for the object-owned buffer.  The source needs the alignment of its element only; frames that
 * start on 16-byte boundaries are read with 16-byte loads, with the same result.  Dense mode: three launches (count per
 * segment, scan per frame, scatter); organised mode: a 4 * n-byte memset and one launch.  No allocation, no host
 * synchronisation, no spinning between workgroups: capturable like kde_error3d_compare_batch. */
int kde_cloud_build_batch(kde_cloud* h, int n, const kde_error3d_source* src, const uint8_t* bgr_dev, int bgr_frames,
                          kde_cloud_point* out_dev, void* stream);
/* the records of the last call of main.cpp:211-300's loop (out_dev of that call, or the object-owned buffer) and the number of
 * valid pixels per frame, count[n]; valid until the next call or destroy.  KDE_ERR_INVALID before the first call. */
int kde_cloud_points_device(kde_cloud* h, kde_cloud_point** out);
int kde_cloud_counts_device(kde_cloud* h, uint32_t** out);   /* main.cpp:211-300: the sizes of its clouds, on the device */
/* count[n] in pinned host memory after a blocking copy on `stream` (main.cpp:211-300: cloud->size()): synchronises */
int kde_cloud_counts_host(kde_cloud* h, void* stream, const uint32_t** out);
/* the clouds of main.cpp:211-300 in pinned host memory (allocated on first use), frames packed tightly: frame f is the
 * records offsets[f] .. offsets[f + 1] - 1, offsets[n] the total.  Dense mode copies only the used records.  The buffer
 * out_dev of the last call must still be alive.  Synchronises. */
int kde_cloud_points_host(kde_cloud* h, void* stream, const kde_cloud_point** out, const uint64_t** offsets);

/* ==========================================================================================
 * OrganizedMesh: the surface main.cpp:211-300 hands to its viewer as points, as a triangle mesh of the organised grid, for a
 * batch of frames (the reference has no mesh; it stands in for pcl::OrganizedFastMesh on the cloud of main.cpp:211-300).
 * One frame has W x H pixels, W, H >= 2; a source is what kde_error3d_source describes, projected as kde_cloud_* projects it.
 *   vertices   exactly the dense cloud: pixel i is a vertex iff p.z > z_min && p.z < z_max; its record is the kde_cloud_point
 *              of kde_cloud_build_batch (same divisor, negate_z), stored in raster order in the frame's slot, which starts
 *              at record f * W * H; count[f] of them, nothing written behind.  The index of a vertex is its rank.
 *   edges      two pixels are linked iff both are valid and |za - zb| <= max_diff + rel_diff * min(za, zb), z the source's z
 *              in millimetres; one subtraction, one product, one sum in binary32 (the link of kde_speckle_*)
 *   triangles  pixel (x, y), x < W - 1, y < H - 1, owns the quad a = (x, y), b = (x + 1, y), c = (x, y + 1), d = (x + 1, y + 1).
 *              A triangle is emitted iff its three corners are valid and its three edges linked.  Four valid corners:
 *              KDE_MESH_DIAG_AD gives (a, c, d) then (a, d, b); KDE_MESH_DIAG_BC (a, c, b) then (b, c, d);
 *              KDE_MESH_DIAG_ADAPTIVE cuts along b-c iff |zb - zc| < |za - zd| (a tie goes to a-d).  Each of the two is
 *              tested on its own; the other cut is not tried.  Exactly three valid corners: a missing (b, c, d), b missing
 *              (a, c, d), c missing (a, d, b), d missing (a, c, b).  All turn the same way in the image; flip_winding swaps
 *              v1 and v2 of every triangle.
 *   records    kde_mesh_triangle, 12 bytes, frame-local indices, ordered by owning pixel in raster order, within a quad the
 *              first before the second: the first tri_count[f] records of the slot that starts at record
 *              f * 2 (W - 1) (H - 1); nothing written behind.
 * The result is a function of the frame alone: the same bytes for any batch, place in it and pointer alignment.
 * ========================================================================================== */
enum { KDE_MESH_DIAG_AD = 0, KDE_MESH_DIAG_BC = 1, KDE_MESH_DIAG_ADAPTIVE = 2 };
typedef struct kde_mesh_triangle { uint32_t v0, v1, v2; } kde_mesh_triangle;                 /* 12 bytes */
typedef struct kde_mesh_params {
    float z_min, z_max, divisor; int negate_z; float max_diff, rel_diff; int diagonal; int flip_winding;
} kde_mesh_params;
typedef struct kde_mesh kde_mesh;
/* the literals of main.cpp:211-300 (50, 15000, 1000, negate_z 1), the link of kde_speckle_default_params (10, 0.02),
 * KDE_MESH_DIAG_ADAPTIVE, flip_winding 0 */
int kde_mesh_default_params(kde_mesh_params* p);
/* the surface of main.cpp:211-300 for max_batch frames on the current device; p == NULL: the defaults.  width, height >= 2;
 * z_min, z_max, divisor as kde_cloud_create; max_diff, rel_diff finite and >= 0; diagonal in 0..2.  The object owns
 * max_batch * W * H vertex records and max_batch * 2 (W - 1) (H - 1) triangle records for calls with NULL outputs.  On a host
 * without a device the object is created without buffers and kde_mesh_build_batch returns KDE_ERR_HIP, like kde_cloud_create. */
int kde_mesh_create(kde_mesh** out, int width, int height, int max_batch, const kde_mesh_params* p);
int kde_mesh_destroy(kde_mesh* h);   /* main.cpp:211-300 holds its clouds in shared pointers; NULL is a no-op */
/* the camera a depth-map source is projected with (main.cpp:211-300 reads clouds made by convertor.projectiveToReal, :168),
 * as kde_cloud_set_camera.  Needed only when the source is a depth map. */
int kde_mesh_set_camera(kde_mesh* h, const double* K9);
/* the loop of main.cpp:211-300 for n <= max_batch frames, with the triangles: src, bgr_dev and bgr_frames as
 * kde_cloud_build_batch; vertices_out_dev is [n][W * H] records on a 16-byte boundary, triangles_out_dev
 * [n][2 (W - 1) (H - 1)] records on a 4-byte boundary, either NULL for the object-owned buffer.  Six launches (the three of the
 * dense cloud, classify, scan, emit), no memset, no allocation, no upload, no host synchronisation, no spinning between
 * workgroups: capturable from the first call. */
int kde_mesh_build_batch(kde_mesh* h, int n, const kde_error3d_source* src, const uint8_t* bgr_dev, int bgr_frames,
                         kde_cloud_point* vertices_out_dev, kde_mesh_triangle* triangles_out_dev, void* stream);
/* the records of the last call of main.cpp:211-300's loop (the outputs of that call, or the object-owned buffers), count[n]
 * and tri_count[n]; valid until the next call or destroy.  KDE_ERR_INVALID before the first call. */
int kde_mesh_vertices_device(kde_mesh* h, kde_cloud_point** out);
int kde_mesh_triangles_device(kde_mesh* h, kde_mesh_triangle** out);   /* main.cpp:211-300 has no faces: the triangles of the last call */
int kde_mesh_counts_device(kde_mesh* h, uint32_t** out);       /* main.cpp:211-300: the sizes of its clouds, on the device */
int kde_mesh_tri_counts_device(kde_mesh* h, uint32_t** out);   /* main.cpp:211-300 has no faces: their number per frame, on the device */
/* count[n] / tri_count[n] in pinned host memory after a blocking copy on `stream` (main.cpp:211-300: cloud->size()): synchronise */
int kde_mesh_counts_host(kde_mesh* h, void* stream, const uint32_t** out);
int kde_mesh_tri_counts_host(kde_mesh* h, void* stream, const uint32_t** out);   /* main.cpp:211-300: the number of faces, as cloud->size() */
/* the vertices / triangles of main.cpp:211-300's surface in pinned host memory (allocated on first use), frames packed
 * tightly: frame f is the records offsets[f] .. offsets[f + 1] - 1, offsets[n] the total; only the used records are copied.
 * The output buffers of the last call must still be alive.  Synchronise, like kde_cloud_points_host. */
int kde_mesh_vertices_host(kde_mesh* h, void* stream, const kde_cloud_point** out, const uint64_t** offsets);
int kde_mesh_triangles_host(kde_mesh* h, void* stream, const kde_mesh_triangle** out, const uint64_t** offsets);   /* main.cpp:211-300 */

/* ==========================================================================================
 * DepthRegistration: depth warped into the colour camera's view.  Every class of this library assumes that depth pixel
 * (x, y) and colour pixel (x, y) look along the same ray; the reference gets that from outside its own code:
 * Kinect::InitAllData (Kinect.cpp:71-75) asks OpenNI to register the depth stream to the image stream before any frame
 * reaches main.cpp.  Frames from any other source (the host feeds take "the sensor's uint16 depth") are registered here, for
 * a batch on the device, by a scatter through a z-buffer.
 *
 * Calibration: the depth camera (fxd, fyd, cxd, cyd) and the colour camera (fxc, fyc, cxc, cyc), each from a row-major 3 x 3
 * double matrix converted to float, and P_colour = R * P_depth + t (R 9 doubles row-major, t 3 doubles in millimetres, both
 * converted to float).  Axes: x right, y down, z forward; pixel centres at integer coordinates.  cx AND cy ARE KEPT AS
 * FLOATS HERE, not truncated to int as DimensionConvertor does (DimensionConvertor.cpp:3-13): calibrated principal points
 * are no integers, and truncating two cameras independently would move the result by up to a pixel.  No lens distortion
 * here: frames of a camera with distortion coefficients go through LensUndistortion (kde_undist_*, below) first.
 *
 * The rule.  Every operation is one IEEE binary32 operation in the order written, no fused multiply-add, divisions
 * correctly rounded.  For source pixel (u, v) of frame f with depth z (float, or (float)u16):
 *   valid     iff z > z_min && z < z_max (defaults 0 and FLT_MAX: NaN, +-inf, 0 and negatives are invalid)
 *   project(a, b):  xn = (a - cxd) / fxd;  yn = (b - cyd) / fyd;  X = xn * z;  Y = yn * z
 *             Xc = ((r00 * X + r01 * Y) + r02 * z) + tx, Yc and Zc likewise from rows 1 and 2
 *             fails unless Zc > z_min && Zc < z_max
 *             uc = fxc * (Xc / Zc) + cxc;  vc = fyc * (Yc / Zc) + cyc
 *   centre    project((float)u, (float)v); a failed centre drops the pixel.  The value written is the centre's Zc, its key
 *             the bit pattern of Zc as uint32 (Zc is positive, so unsigned order is numeric order).
 *   point mode (max_splat == 0): iu = rintf(uc), iv = rintf(vc) (ties to even); kept iff iu >= 0 && iu <= Wc - 1 &&
 *             iv >= 0 && iv <= Hc - 1, tested on the floats (a NaN fails); zbuf[f][iv][iu] = min(zbuf, key)
 *   splat mode (max_splat in 1..16), which closes the cracks a one-pixel scatter leaves when the target is finer:
 *             (ua, va) = project(u - 0.5f, v - 0.5f), (ub, vb) = project(u + 0.5f, v + 0.5f) at the same z; either failing
 *             or a NaN coordinate drops the pixel.  Columns i0 = max(ceilf(min(ua, ub)), 0) .. i1 = min(ceilf(max(ua, ub))
 *             - 1, Wc - 1): the integers of a half-open interval, so abutting footprints tile the line; a span longer than
 *             max_splat is cut to i0 .. i0 + max_splat - 1; rows likewise; an empty span writes nothing.  Every covered
 *             target pixel takes the min with the centre's key.
 *   finalise  a target pixel no source pixel reached is 0 (the sensor's "invalid"); any other is Zc unchanged
 *             (KDE_DEPTH_F32) or depth_to_u16(Zc) as kde_points_to_depth rounds (KDE_DEPTH_U16).  filled[f] = the number of
 *             target pixels reached, counted on the keys, not on the rounded uint16.
 * The min of keys does not depend on arrival order and the count is an integer sum: the result is deterministic to the bit
 * and does not depend on n, a frame's position in the batch or pointer alignment.
 * ========================================================================================== */
typedef struct kde_reg_params { float z_min, z_max; int max_splat; } kde_reg_params;
typedef struct kde_reg kde_reg;
/* Kinect.cpp:71-75 takes no parameter: z_min 0, z_max FLT_MAX, max_splat 0 */
int kde_reg_default_params(kde_reg_params* p);
/* the two viewpoints of Kinect.cpp:71-75 -- depth frames of depth_w x depth_h, colour frames of color_w x color_h -- for
 * max_batch frames on the current device; p == NULL: the defaults.  Sizes >= 1 (a side at most 2^24); z_min finite and >= 0
 * (the key order needs positive z), z_min < z_max, max_splat in 0..16.  The object owns the z-buffer (4 bytes per target
 * pixel), filled[max_batch] and max_batch * color_w * color_h floats for calls with out_dev == NULL.  On a host without a
 * device the object is created without buffers: every call validates as usual and the launches then return KDE_ERR_HIP. */
int kde_reg_create(kde_reg** out, int depth_w, int depth_h, int color_w, int color_h, int max_batch, const kde_reg_params* p);
int kde_reg_destroy(kde_reg* h);   /* Kinect.cpp:71-75 keeps its generators while the Kinect lives; NULL is a no-op */
/* the calibration Kinect.cpp:71-75 leaves to the device's factory data: Kd9, Kc9, R9 row-major, t3 in millimetres, as above.
 * KDE_ERR_INVALID: a null pointer, a non-finite value (as double or as float), fx or fy of either camera not > 0. */
int kde_reg_set_calibration(kde_reg* h, const double* Kd9, const double* Kc9, const double* R9, const double* t3);
/* Kinect.cpp:71-75 for n <= max_batch frames: depth_dev is [n][depth_h][depth_w] of depth_format (KDE_DEPTH_F32 |
 * KDE_DEPTH_U16), out_dev is [n][color_h][color_w] of out_format or NULL for the object-owned buffer.  Pointers need the
 * alignment of their element only; source frames on a 16-byte (float) or 8-byte (uint16) boundary are read with vector
 * loads, with the same result.  KDE_ERR_INVALID before kde_reg_set_calibration.  Three launches (the z-buffer reset to
 * 0xFF, the scatter, the finalise); no allocation, no host synchronisation, no communication between workgroups: capturable
 * like kde_cloud_build_batch.  The reset is a kernel and not a memset node, because the replay of a captured graph did not
 * keep a memset node in front of the kernel behind it. */
int kde_reg_register_batch(kde_reg* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev, void* stream);
/* Kinect.cpp:71-75 the other way round, for users who would rather work at the depth camera's resolution: for each depth
 * pixel (u, v) of frame f with the point-mode target (iu, iv) of its centre, out_bgr[f][v][u] = bgr[iv][iu] when the pixel
 * is valid and its target inside the colour frame, else (0, 0, 0).  bgr_dev is [bgr_frames][color_h][color_w][3] with
 * bgr_frames == 1 (one image for every frame) or n; out_bgr_dev is [n][depth_h][depth_w][3].  THERE IS NO OCCLUSION TEST: a
 * depth pixel the colour camera cannot see takes the colour of whatever hides it.  One launch; does not touch the z-buffer
 * or the results of kde_reg_register_batch. */
int kde_reg_color_to_depth_batch(kde_reg* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev, int bgr_frames,
                                 uint8_t* out_bgr_dev, void* stream);
/* the registered frames of the last kde_reg_register_batch (Kinect.cpp:71-75): out_dev of that call or the object-owned
 * buffer, in that call's out_format; valid until the next call or destroy.  KDE_ERR_INVALID before the first call. */
int kde_reg_depth_device(kde_reg* h, void** out);
/* the same in pinned host memory after a blocking copy on `stream` (Kinect.cpp:71-75 hands its frames to the host):
 * synchronises; out_dev of the last call must still be alive */
int kde_reg_depth_host(kde_reg* h, void* stream, const void** out);
int kde_reg_filled_device(kde_reg* h, uint32_t** out);   /* Kinect.cpp:71-75: filled[n] of the last call, on the device */
/* filled[n] in pinned host memory after a blocking copy on `stream` (Kinect.cpp:71-75): synchronises */
int kde_reg_filled_host(kde_reg* h, void* stream, const uint32_t** out);

/* ==========================================================================================
 * LensUndistortion: frames of a camera with lens distortion resampled into a pinhole view.  Every class of this library
 * assumes a pinhole camera (DimensionConvertor.cpp:3-13 back-projects with fx, fy, cx, cy only); the reference never had to
 * care, because its frames come through OpenNI from a Kinect v1.  Sensors calibrated with OpenCV ship distortion
 * coefficients, and their frames, taken as they are, bend every plane the pipeline fits.  This is a gather, for a batch on
 * the device: colour and depth go through the same map with different sampling rules.  No reference counterpart.
 *
 * Calibration: the source (distorted) camera (fx, fy, cx, cy) from a row-major 3 x 3 double matrix K converted to float (cx,
 * cy stay floats, as in kde_reg_*); eight coefficients k1, k2, p1, p2, k3, k4, k5, k6 in OpenCV's order, doubles converted to
 * float: the rational model, of which k4 = k5 = k6 = 0 is the five-coefficient Brown-Conrady model; the target (pinhole)
 * camera (fxn, fyn, cxn, cyn) from K_new, or K when K_new is NULL.  Source frames are src_w x src_h, output frames out_w x
 * out_h.  There is no rectifying rotation: it would change z, which is kde_reg_*'s job.  No fisheye model.
 *
 * The rule.  Every operation is one IEEE binary32 operation in the order written, no fused multiply-add, divisions
 * correctly rounded.  For output pixel (i, j):
 *   x  = ((float)i - cxn) / fxn;  y = ((float)j - cyn) / fyn
 *   xx = x * x;  yy = y * y;  xy = x * y;  r2 = xx + yy
 *   num = ((k3 * r2 + k2) * r2 + k1) * r2 + 1;  den = ((k6 * r2 + k5) * r2 + k4) * r2 + 1;  rad = num / den
 *   xd = (x * rad + p1 * (xy + xy)) + p2 * (r2 + (xx + xx))
 *   yd = (y * rad + p1 * (r2 + (yy + yy))) + p2 * (xy + xy)
 *   us = fx * xd + cx;  vs = fy * yd + cy                      the point of the source frame the pixel shows
 *   bilinear(p)  x0 = floorf(us), ax = us - x0, y0 = floorf(vs), ay = vs - y0; the taps p00 = p(x0, y0), p01 = p(x0 + 1, y0),
 *             p10 = p(x0, y0 + 1), p11 = p(x0 + 1, y0 + 1); top = p00 + ax * (p01 - p00), bot = p10 + ax * (p11 - p10),
 *             value = top + ay * (bot - top)
 *   colour    BGR uint8.  The pixel is (0, 0, 0) unless us > -1 && us < src_w && vs > -1 && vs < src_h, tested on the floats
 *             before any conversion to an integer (a NaN fails).  A tap outside the source frame is (0, 0, 0).  Per channel
 *             the byte stored is rintf(bilinear) (ties to even) clamped to 0 .. 255.
 *   depth     KDE_DEPTH_F32 or KDE_DEPTH_U16 on either side, uint16 widened by (float)u.  A depth is valid iff z > z_min && z <
 *             z_max (defaults 0 and FLT_MAX: NaN, +-inf, 0 and negatives are invalid).
 *             depth_interp == 0 (default), and the fall-back of the other mode: fu = rintf(us), fv = rintf(vs) (ties to
 *             even); the sample (fu, fv) is kept iff fu >= 0 && fu <= src_w - 1 && fv >= 0 && fv <= src_h - 1, tested on the
 *             floats, and it is valid; otherwise the pixel is 0 (the sensor's "invalid").
 *             depth_interp == 1: the pixel is bilinear(z) iff x0 >= 0 && x0 + 1 <= src_w - 1 && y0 >= 0 && y0 + 1 <= src_h - 1
 *             (all four taps inside, on the floats), all four taps are valid, and max - min of the four <= max_gap
 *             (millimetres; no default).  In every other case the nearest rule above: a depth is never blended across a hole
 *             or an edge.
 *             The output is the float itself (KDE_DEPTH_F32) or depth_to_u16 of it as kde_points_to_depth rounds
 *             (KDE_DEPTH_U16).  filled[f] = the number of output pixels of frame f that were kept (by either rule), counted
 *             before the uint16 rounding, as kde_reg_* counts its keys.
 * Every output pixel is a function of the source frame and its own coordinates, and the count is an integer sum: the result
 * is deterministic to the bit and does not depend on n, a frame's position in the batch or pointer alignment.
 * ========================================================================================== */
typedef struct kde_undist_params { float z_min, z_max; int depth_interp; float max_gap; } kde_undist_params;
typedef struct kde_undist kde_undist;
/* z_min 0, z_max FLT_MAX, depth_interp 0 (nearest), max_gap 0 (unused in that mode; depth_interp 1 needs one) */
int kde_undist_default_params(kde_undist_params* p);
/* source frames of src_w x src_h, output frames of out_w x out_h, max_batch frames on the current device; p == NULL: the
 * defaults.  Sizes >= 1 (a side at most 2^24, so that W - 1 is an exact float); z_min finite and >= 0, z_min < z_max,
 * depth_interp 0 or 1, and with depth_interp 1 a finite max_gap > 0.  The object owns filled[max_batch], max_batch * out_w *
 * out_h floats for calls with out_dev == NULL and the out_w * out_h float2 of kde_undist_map_device.  On a host without a
 * device the object is created without buffers: every call validates as usual and the launches then return KDE_ERR_HIP. */
int kde_undist_create(kde_undist** out, int src_w, int src_h, int out_w, int out_h, int max_batch, const kde_undist_params* p);
int kde_undist_destroy(kde_undist* h);   /* NULL is a no-op */
/* K9 and Knew9 row-major 3 x 3 (Knew9 == NULL: the pinhole view keeps K), dist8 = k1, k2, p1, p2, k3, k4, k5, k6, as above.
 * KDE_ERR_INVALID: a null K9 or dist8, a non-finite value (as double or as float), fx or fy of either camera not > 0.  A
 * refused call leaves the calibration in force as it was. */
int kde_undist_set_calibration(kde_undist* h, const double* K9, const double* dist8, const double* Knew9);
/* n <= max_batch colour frames: bgr_dev is [bgr_frames][src_h][src_w][3] with bgr_frames == 1 (one image for every frame) or
 * n, out_bgr_dev is [n][out_h][out_w][3].  No alignment is asked of either pointer; output frames on a 4-byte boundary are
 * written 256 consecutive bytes per store instruction, with the same result.  KDE_ERR_INVALID before
 * kde_undist_set_calibration.  One launch; no allocation, no host synchronisation, no communication between workgroups:
 * capturable like kde_reg_register_batch. */
int kde_undist_color_batch(kde_undist* h, int n, const uint8_t* bgr_dev, int bgr_frames, uint8_t* out_bgr_dev, void* stream);
/* n <= max_batch depth frames: depth_dev is [n][src_h][src_w] of depth_format (KDE_DEPTH_F32 | KDE_DEPTH_U16), out_dev is
 * [n][out_h][out_w] of out_format or NULL for the object-owned buffer.  Pointers need the alignment of their element only;
 * output frames on a 16-byte (float) or 8-byte (uint16) boundary are written with vector stores, with the same result.
 * KDE_ERR_INVALID before kde_undist_set_calibration.  Two launches (filled = 0, the remap: kernel nodes keep their order in a
 * replayed graph, a memset node did not); no allocation, no host synchronisation: capturable. */
int kde_undist_depth_batch(kde_undist* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev, void* stream);
/* the frames of the last kde_undist_depth_batch: out_dev of that call or the object-owned buffer, in that call's
 * out_format; valid until the next call or destroy.  KDE_ERR_INVALID before the first call. */
int kde_undist_depth_device(kde_undist* h, void** out);
/* the same in pinned host memory after a blocking copy on `stream`: synchronises; out_dev of the last call must still be alive */
int kde_undist_depth_host(kde_undist* h, void* stream, const void** out);
int kde_undist_filled_device(kde_undist* h, uint32_t** out);   /* filled[n] of the last kde_undist_depth_batch, on the device */
/* filled[n] in pinned host memory after a blocking copy on `stream`: synchronises */
int kde_undist_filled_host(kde_undist* h, void* stream, const uint32_t** out);
/* [out_h][out_w] of (us, vs) as float2 on the device, what OpenCV's initUndistortRectifyMap gives (CV_32FC2) for this
 * calibration with R = identity: computed by its own launch on `stream` at the first request after
 * kde_undist_set_calibration, returned as it is later (work on another stream must be ordered behind that first request by
 * the caller).  The remap calls above compute the map per pixel and do not read it.  No allocation, no synchronisation. */
int kde_undist_map_device(kde_undist* h, void* stream, const float** out);

/* ==========================================================================================
 * GuidedDepthUpsampling: a low-resolution depth frame brought to the size of its colour image.  Every class of this library
 * takes depth and colour of one size; sensors other than a Kinect v1 deliver 512 x 424 or 320 x 240 depth beside 1080p or VGA
 * colour.  This is joint bilateral upsampling (Kopf et al. 2007): low-resolution samples weighted by their distance to the
 * output pixel and by how much the full-resolution colour at the output pixel resembles the colour at the sample -- the idea
 * of JointBilateralFilter on two grids.  A gather, for a batch on the device.  No reference counterpart.
 *
 * Frames: depth src_w x src_h (KDE_DEPTH_F32 or KDE_DEPTH_U16, uint16 widened by (float)u), the guide BGR uint8 out_w x out_h,
 * the output out_w x out_h (either format); out_w >= src_w and out_h >= src_h.  Both images show the same view: pixel centres
 * at (i + 0.5) / out_w of the width and (qx + 0.5) / src_w of it.
 *
 * The rule.  Every operation is one IEEE binary32 operation in the order written, no fused multiply-add, divisions
 * correctly rounded.  Tables, made once at create on the host:
 *   sx = (float)src_w / (float)out_w;  sy = (float)src_h / (float)out_h
 *   gx_of[qx] = clamp((int)rintf(((float)qx + 0.5f) / sx - 0.5f), 0, out_w - 1) for qx = 0 .. src_w - 1, gy_of[qy] likewise:
 *             the output pixel that "is" low-resolution sample q
 *   range[k] = (float)exp(-(double)(k * k) / (2.0 * (double)sigma_color * (double)sigma_color)) for k = 0 .. 765
 * For output pixel (i, j) with guide colour c = bgr(i, j):
 *   1. u = ((float)i + 0.5f) * sx - 0.5f;  v = ((float)j + 0.5f) * sy - 0.5f;  x0 = floorf(u);  y0 = floorf(v)
 *   2. taps qy = y0 - r + 1 .. y0 + r (outer loop), qx = x0 - r + 1 .. x0 + r (inner loop), in that order.  A tap outside the
 *      source frame is absent.  A tap whose depth is not z > z_min && z < z_max is absent (NaN and +-inf fail).
 *   3. wx = max(1 - fabsf((float)qx - u) / (float)r, 0), wy likewise;  k = |db| + |dg| + |dr| between c and
 *      bgr(gx_of[qx], gy_of[qy]);  w = (wx * wy) * range[k].  A tap with w == 0 is absent: w > 0 is the test.
 *   4. max_gap > 0, the guard: zref = the depth of the tap with the largest w, the first such tap in tap order winning a tie;
 *      taps with fabsf(z - zref) > max_gap are absent.
 *   5. num = den = 0; per remaining tap in tap order num = num + w * z, den = den + w.  The pixel is num / den, or 0 (the
 *      sensor's "invalid") if no tap remains.
 *   6. The output is the float itself (KDE_DEPTH_F32) or depth_to_u16 of it as kde_points_to_depth rounds (KDE_DEPTH_U16).
 *      filled[f] = the number of pixels of frame f with a remaining tap, counted before the uint16 rounding.
 * No transcendental is evaluated at run time.  Every output pixel is a function of the source frame, the guide and its own
 * coordinates, and the count is an integer sum: the result is deterministic to the bit and does not depend on n, a frame's
 * position in the batch or pointer alignment.
 * ========================================================================================== */
typedef struct kde_upsample_params { int radius; float sigma_color; float max_gap; float z_min, z_max; } kde_upsample_params;
typedef struct kde_upsample kde_upsample;
/* radius 2, sigma_color 30 (the colour constant of K0, cv_bilateral's, in the same form: an L1 distance, squared), max_gap 0
 * (no guard), z_min 0, z_max FLT_MAX */
int kde_upsample_default_params(kde_upsample_params* p);
/* depth frames of src_w x src_h, guide and output frames of out_w x out_h, max_batch frames on the current device; p == NULL:
 * the defaults.  KDE_ERR_INVALID: sizes below 1 or a side above 2^24, out_w < src_w or out_h < src_h (this is an upsampler,
 * and it bounds the taps a tile of output pixels reads), radius outside 1..4, sigma_color not finite or not > 0, max_gap not
 * finite or < 0, z_min not finite or < 0, z_min >= z_max.  The object owns the tables, filled[max_batch], a count per
 * workgroup and max_batch * out_w * out_h floats for calls with out_dev == NULL.  On a host without a device the object is
 * created without buffers: every call validates as usual and the launch then returns KDE_ERR_HIP. */
int kde_upsample_create(kde_upsample** out, int src_w, int src_h, int out_w, int out_h, int max_batch, const kde_upsample_params* p);
int kde_upsample_destroy(kde_upsample* h);   /* NULL is a no-op */
/* n <= max_batch frames: depth_dev is [n][src_h][src_w] of depth_format (KDE_DEPTH_F32 | KDE_DEPTH_U16), bgr_dev is
 * [bgr_frames][out_h][out_w][3] with bgr_frames == 1 (one guide for every frame) or n, out_dev is [n][out_h][out_w] of
 * out_format or NULL for the object-owned buffer.  Pointers need the alignment of their element only; output frames on a
 * 16-byte (float) or 8-byte (uint16) boundary whose width is a multiple of four are written with vector stores, with the same
 * result.  Two launches: the upsampling, whose workgroups each write their count of filled pixels, and the sum of those
 * counts into filled[f] -- no atomic, no memset node (kernel nodes keep their order in a replayed graph, a memset node did
 * not) and nothing to reset; no allocation, no host synchronisation: capturable from the first call. */
int kde_upsample_depth_batch(kde_upsample* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev, int bgr_frames,
                             int out_format, void* out_dev, void* stream);
/* the frames of the last kde_upsample_depth_batch: out_dev of that call or the object-owned buffer, in that call's
 * out_format; valid until the next call or destroy.  KDE_ERR_INVALID before the first call. */
int kde_upsample_depth_device(kde_upsample* h, void** out);
/* the same in pinned host memory after a blocking copy on `stream`: synchronises; out_dev of the last call must still be alive */
int kde_upsample_depth_host(kde_upsample* h, void* stream, const void** out);
int kde_upsample_filled_device(kde_upsample* h, uint32_t** out);   /* filled[n] of the last kde_upsample_depth_batch, on the device */
/* filled[n] in pinned host memory after a blocking copy on `stream`: synchronises */
int kde_upsample_filled_host(kde_upsample* h, void* stream, const uint32_t** out);
/* range[0 .. 765] of the object as the kernel reads it, copied to table_host[capacity]; KDE_ERR_INVALID for capacity < 766.
 * Host memory only: works without a device. */
int kde_upsample_range_table(kde_upsample* h, float* table_host, int capacity);

/* ==========================================================================================
 * DepthHoleFilling: the holes of a depth frame filled from their valid neighbours under the guide of its colour image.  The
 * registration's z-buffer leaves occlusion bands and cracks, the undistortion an invalid rim, a Kinect a shadow band beside
 * every foreground object, a time-of-flight sensor drops dark surfaces; the filters behind reach two or three pixels into a
 * hole.  This stage closes a hole front by front: each pass fills the hole pixels that have enough valid neighbours within
 * `radius`, from those neighbours, weighted by distance and by how much the guide colour at the neighbour resembles the
 * colour at the pixel; the next pass builds on the result.  iterations * radius bounds how far a fill reaches.  For a batch on
 * the device.  No reference counterpart.
 *
 * Frames: depth width x height (KDE_DEPTH_F32 or KDE_DEPTH_U16, uint16 widened by (float)u), the guide BGR uint8 and the
 * output (either format) of the same size.
 *
 * The rule.  Every operation is one IEEE binary32 operation in the order written, no fused multiply-add, divisions
 * correctly rounded.  With r = radius and N = iterations.  Tables, made once at create on the host:
 *   space[dy + r][dx + r] = (float)exp(-(double)(dx * dx + dy * dy) / (2.0 * (double)sigma_space * (double)sigma_space))
 *   range[k] = (float)exp(-(double)(k * k) / (2.0 * (double)sigma_color * (double)sigma_color)) for k = 0 .. 765
 * The state of a frame is a float image z in which 0 means "hole".
 *   Pass 0 sanitises the input: z = (d > z_min && d < z_max) ? (float)d : 0 (NaN and +-inf become holes); pass_of = 0 where
 *   z > 0 and 255 elsewhere.
 *   Pass p = 1 .. N reads the state of pass p - 1 as a snapshot and writes a new state.  For each pixel with z == 0:
 *   1. its taps are dy = -r .. r (outer loop), dx = -r .. r (inner loop), without the centre, in that order.
 *   2. A tap is absent if it lies outside the frame or has z == 0.
 *   3. k = |db| + |dg| + |dr| between the guide at the pixel and the guide at the tap.
 *   4. w = space[dy + r][dx + r] * range[k].  A tap with w == 0 is absent: w > 0 is the test.
 *   5. support = the number of taps that remain.
 *   6. max_gap > 0, the guard: zref = the depth of the heaviest remaining tap, the first such tap in tap order winning a tie
 *      (gap_rule 0), or the largest depth among the remaining taps -- the background, where a shadow band belongs (gap_rule
 *      1); taps with fabsf(z - zref) > max_gap become absent.  support is not recounted.
 *   7. num = den = 0; per remaining tap in tap order num = num + w * z, den = den + w;  v = num / den.
 *   8. The pixel becomes v with pass_of = p iff support >= min_taps and v > 0; otherwise it stays 0.
 *   Pixels with z > 0 never change, in any pass.
 * After pass N, per frame: the output is the state itself (KDE_DEPTH_F32) or depth_to_u16 of it as kde_points_to_depth rounds
 * (KDE_DEPTH_U16); filled[f] = the number of pixels with 1 <= pass_of <= N, remaining[f] = the number still 0, both counted
 * before the uint16 rounding; pass_of is 0 for an original pixel, p for one filled in pass p, 255 for one that is still a hole.
 * N passes and then M more on the float result equal N + M passes (at the default z_min and z_max): validity is z > 0 on the
 * state and nothing else.  A fill from equal depths need not be that depth to the bit: num / den rounds.
 * No transcendental is evaluated at run time.  Every pixel of a pass is a function of the snapshot before it, the guide and
 * the tables, and the counts are integer sums: the result is deterministic to the bit and does not depend on n, a frame's
 * position in the batch, pointer alignment or passes_per_launch.
 * ========================================================================================== */
typedef struct kde_holefill_params { int radius; int iterations; int min_taps; float sigma_space; float sigma_color;
                                     float max_gap; int gap_rule; float z_min, z_max; int passes_per_launch; } kde_holefill_params;
typedef struct kde_holefill kde_holefill;
/* radius 2, iterations 8, min_taps 3, sigma_space 2, sigma_color 30 (the colour constant of K0, in the same form: an L1
 * distance, squared), max_gap 0 (no guard), gap_rule 0 (heaviest; 1: farthest), z_min 0, z_max FLT_MAX, passes_per_launch 0
 * (the library's choice for the radius and the guard; 1 .. 4: forced) */
int kde_holefill_default_params(kde_holefill_params* p);
/* frames of width x height, max_batch of them on the current device; p == NULL: the defaults.  KDE_ERR_INVALID: sizes below 1
 * or a side above 2^24, radius outside 1..3, iterations outside 1..64, min_taps outside 1..(2 radius + 1)^2 - 1, sigma_space or
 * sigma_color not finite or not > 0, max_gap not finite or < 0, gap_rule neither 0 nor 1, z_min not finite or < 0, z_min >=
 * z_max, passes_per_launch outside 0..4.  The object owns the tables, the two counts per frame and per workgroup, pass_of for
 * calls without pass_of_dev, max_batch * width * height floats for calls with out_dev == NULL and up to two more such images
 * for the state between launches.  On a host without a device the object is created without buffers: every call validates as
 * usual and the launch then returns KDE_ERR_HIP. */
int kde_holefill_create(kde_holefill** out, int width, int height, int max_batch, const kde_holefill_params* p);
int kde_holefill_destroy(kde_holefill* h);   /* NULL is a no-op */
/* n <= max_batch frames: depth_dev is [n][height][width] of depth_format (KDE_DEPTH_F32 | KDE_DEPTH_U16), bgr_dev is
 * [bgr_frames][height][width][3] with bgr_frames == 1 (one guide for every frame) or n, out_dev is [n][height][width] of
 * out_format or NULL for the object-owned buffer, pass_of_dev is [n][height][width] uint8 or NULL where it is not wanted.
 * Pointers need the alignment of their element only.  In place is refused: KDE_ERR_INVALID where the frames that are written
 * -- out_dev's, or with out_dev == NULL the object-owned buffer's, which kde_holefill_depth_device hands out -- overlap those
 * of depth_dev (a workgroup reads the neighbourhood of its tile while its neighbours write theirs).  To run more passes on a
 * result, pass a buffer for the new result.
 * One launch performs k = passes_per_launch passes in on-chip memory, on a tile and a halo of k * radius pixels around it, so
 * the N passes take ceil(N / k) launches between two object-owned state images, the last of which converts to out_format and
 * writes each workgroup's two counts; one more launch sums them into filled[f] and remaining[f] -- no atomic, no memset node
 * (kernel nodes keep their order in a replayed graph, a memset node did not) and nothing to reset; no allocation, no host
 * synchronisation: capturable from the first call.  A tile without a hole does no pass and only moves its bytes. */
int kde_holefill_fill_batch(kde_holefill* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev, int bgr_frames,
                            int out_format, void* out_dev, uint8_t* pass_of_dev /* NULL: not wanted */, void* stream);
/* the frames of the last kde_holefill_fill_batch: out_dev of that call or the object-owned buffer, in that call's out_format;
 * valid until the next call or destroy.  KDE_ERR_INVALID before the first call (this and the five getters below). */
int kde_holefill_depth_device(kde_holefill* h, void** out);
/* the same in pinned host memory after a blocking copy on `stream`: synchronises; out_dev of the last call must still be alive */
int kde_holefill_depth_host(kde_holefill* h, void* stream, const void** out);
int kde_holefill_filled_device(kde_holefill* h, uint32_t** out);   /* filled[n] of the last kde_holefill_fill_batch, on the device */
/* filled[n] in pinned host memory after a blocking copy on `stream`: synchronises */
int kde_holefill_filled_host(kde_holefill* h, void* stream, const uint32_t** out);
int kde_holefill_remaining_device(kde_holefill* h, uint32_t** out);   /* remaining[n] of the last call, on the device */
int kde_holefill_remaining_host(kde_holefill* h, void* stream, const uint32_t** out);   /* synchronises */
/* the k the object runs with: passes_per_launch where it was given, the library's choice where it was 0 (4, 2, 2 for radius
 * 1, 2, 3; 1 for radius 3 with the guard) */
int kde_holefill_passes_per_launch(kde_holefill* h, int* out);
/* space[(2 radius + 1)^2] (row dy + r, column dx + r) and range[0 .. 765] of the object as the kernel reads them, copied to
 * table_host[capacity]; KDE_ERR_INVALID for a capacity below the table's size.  Host memory only: work without a device. */
int kde_holefill_space_table(kde_holefill* h, float* table_host, int capacity);
int kde_holefill_range_table(kde_holefill* h, float* table_host, int capacity);

/* ==========================================================================================
 * DepthSpeckleFilter: wrong depth taken away.  The registration's point mode lets background samples show through the cracks
 * of an upscaled foreground, a time-of-flight sensor delivers flying pixels along every silhouette, a Kinect speckles inside
 * its shadow bands; the stages behind treat such pixels as data (the hole filler fills the hole around a speckle from the
 * speckle).  This stage labels the connected components of a frame under a depth-difference link and sets the components
 * smaller than min_size to 0, as OpenCV's filterSpeckles does: the complement of DepthHoleFilling -- invalidate first, then
 * fill.  For a batch on the device.  No reference counterpart, no colour guide.
 *
 * Frames: depth width x height (KDE_DEPTH_F32 or KDE_DEPTH_U16, uint16 widened by (float)u), the output (either format) and
 * the optional labels (int32) of the same size.
 *
 * The rule.  Every operation is one IEEE binary32 operation in the order written, no fused multiply-add.
 *   1. State.  z = (d > z_min && d < z_max) ? (float)d : 0 (NaN and +-inf become 0).
 *   2. Link.  Two neighbouring pixels a, b are linked iff both have z > 0 and
 *        fabsf(za - zb) <= max_diff + rel_diff * fminf(za, zb)
 *      with the product and the sum rounded separately.  Neighbours are horizontal or vertical for connectivity 4, plus the
 *      two diagonals for 8.
 *   3. Component.  A component is a class of the transitive closure of the links.  Its label is the smallest raster index
 *      y * width + x among its pixels, within its frame; its size is its pixel count.
 *   4. Output.  z where the component's size is >= min_size, 0 elsewhere; for KDE_DEPTH_U16 depth_to_u16 of that, as
 *      kde_points_to_depth rounds.  labels is the label of a kept pixel and -1 where the output is 0.  Per frame, counted before
 *      the uint16 rounding: removed[f] = the number of pixels with z > 0 whose output is 0, components[f] = the number of kept
 *      components, capped[f] = the number of threads that ran into the hard iteration cap of a loop: 0; anything else is a
 *      defect of the library and the frame is not to be trusted.  min_size 1 removes nothing and is plain labelling.
 * The result is a function of the input frame alone: labels are component minima and the counts integer sums, both order-free,
 * so the bytes do not depend on n, a frame's position in the batch, pointer alignment, the tile shape or the order in which
 * atomics land.
 * ========================================================================================== */
typedef struct kde_speckle_params { int min_size; float max_diff; float rel_diff; int connectivity; float z_min, z_max; } kde_speckle_params;
typedef struct kde_speckle kde_speckle;
/* min_size 64, max_diff 10 (millimetres), rel_diff 0.02, connectivity 4, z_min 0, z_max FLT_MAX */
int kde_speckle_default_params(kde_speckle_params* p);
/* frames of width x height, max_batch of them on the current device; p == NULL: the defaults.  KDE_ERR_INVALID: sizes below 1,
 * a side above 2^24 or width * height above 2^30, min_size outside 1..2^24, max_diff or rel_diff not finite or < 0,
 * connectivity neither 4 nor 8, z_min not finite or < 0, z_min >= z_max.  The object owns the union-find table and the sizes
 * (two 4-byte words per pixel of max_batch frames), three counts per frame and per workgroup, and max_batch * width * height
 * floats for calls with out_dev == NULL.  On a host without a device the object is created without buffers: every call
 * validates as usual and the launch then returns KDE_ERR_HIP. */
int kde_speckle_create(kde_speckle** out, int width, int height, int max_batch, const kde_speckle_params* p);
int kde_speckle_destroy(kde_speckle* h);   /* NULL is a no-op */
/* n <= max_batch frames: depth_dev is [n][height][width] of depth_format (KDE_DEPTH_F32 | KDE_DEPTH_U16), out_dev is
 * [n][height][width] of out_format or NULL for the object-owned buffer, labels_dev is [n][height][width] int32 or NULL where
 * it is not wanted.  Pointers need the alignment of their element only.  In place is allowed exactly when out_dev == depth_dev
 * and out_format == depth_format (the last step reads a pixel and then writes it, every step before it only reads the input);
 * any other overlap of the frames that are written -- out_dev's, or with out_dev == NULL the object-owned buffer's, which
 * kde_speckle_depth_device hands out -- with those of depth_dev is KDE_ERR_INVALID, and so is labels_dev overlapping either.
 * Five launches (three for a frame of one 32 x 16 tile): the tiles labelled in on-chip memory, the components united across
 * the tile seams with atomic minima, the sizes summed at the roots, the output, the sums of the counts.  No workgroup waits
 * for another and every loop is bounded; no memset node and nothing to reset (the words a call accumulates into are
 * initialised by its own first kernel); no allocation, no host synchronisation: capturable from the first call. */
int kde_speckle_filter_batch(kde_speckle* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev,
                             int32_t* labels_dev /* NULL: not wanted */, void* stream);
/* the frames of the last kde_speckle_filter_batch: out_dev of that call or the object-owned buffer, in that call's out_format;
 * valid until the next call or destroy.  KDE_ERR_INVALID before the first call (this and the seven getters below). */
int kde_speckle_depth_device(kde_speckle* h, void** out);
/* the same in pinned host memory after a blocking copy on `stream`: synchronises; out_dev of the last call must still be alive */
int kde_speckle_depth_host(kde_speckle* h, void* stream, const void** out);
int kde_speckle_removed_device(kde_speckle* h, uint32_t** out);   /* removed[n] of the last kde_speckle_filter_batch, on the device */
int kde_speckle_removed_host(kde_speckle* h, void* stream, const uint32_t** out);   /* in pinned host memory: synchronises */
int kde_speckle_components_device(kde_speckle* h, uint32_t** out);   /* components[n] of the last call, on the device */
int kde_speckle_components_host(kde_speckle* h, void* stream, const uint32_t** out);   /* synchronises */
int kde_speckle_capped_device(kde_speckle* h, uint32_t** out);   /* capped[n] of the last call, on the device: 0 in a correct library */
int kde_speckle_capped_host(kde_speckle* h, void* stream, const uint32_t** out);   /* synchronises */

/* ==========================================================================================
 * DepthTemporalFilter: motion-aware smoothing of a depth sequence.  Every stage above looks at one frame; a camera delivers a
 * sequence, and frame-to-frame noise survives the spatial filters while holes blink open and shut.  This stage blends each
 * sample into a per-pixel running value while the sample stays on the same surface, starts again where it jumps, holds the
 * value over short dropouts and forgets it where the colour guide says the scene changed.  It sits beside DepthSpeckleFilter
 * and in front of DepthHoleFilling.  No reference counterpart (kde_buffer2d_update_sequence folds n frames into ONE plain
 * average and has no notion of motion).
 *
 * The frames of a call are consecutive in time, and the object carries state from one call to the next.
 *
 * Frames: depth width x height (KDE_DEPTH_F32 or KDE_DEPTH_U16, uint16 widened by (float)u), the optional guide
 * width x height x 3 (b, g, r bytes) and the output (either format) of the same size.
 *
 * State per pixel, object-owned: value (float32, 0 means none) and hist (uint32): bits 0-7 hold the raw validity of the last
 * eight frames, bit 0 the newest; bits 8-31 hold the guide colour b | g << 8 | r << 16 of the previous frame, or 0 when no
 * guide was ever given.  kde_temporal_create and kde_temporal_reset set both words to 0.
 *
 * The rule.  Every operation is one IEEE binary32 operation in the order written, no fused multiply-add.  For frame t of the
 * call, in order, for a pixel with raw sample d and, if a guide is given, colour (b, g, r):
 *   1. Sample.  z = (d > z_min && d < z_max) ? (float)d : 0 (NaN and +-inf become 0).
 *   2. Scene change, only with a guide and color_thresh < 765.  If |b - b'| + |g - g'| + |r - r'| > color_thresh against the
 *      stored colour (b', g', r'): value = 0 and hist &= ~0xFF.  On the first frame after a reset the stored colour is (0, 0, 0)
 *      and the state is already empty, so no flag is needed.
 *   3. Valid sample (z > 0).  prev = value.  If prev > 0 && fabsf(z - prev) <= max_diff + rel_diff * fminf(z, prev), then
 *      out = prev + alpha * (z - prev), with the difference, the product and the sum each rounded on its own; otherwise
 *      out = z.  hist[7:0] = (hist[7:0] << 1 | 1) & 0xFF.
 *   4. Hole (z == 0).  prev = value.  If prev > 0 && persist_min >= 1 && popcount(hist[7:0]) >= persist_min, then out = prev
 *      (the history before this frame's shift); otherwise out = 0.  hist[7:0] = (hist[7:0] << 1) & 0xFF.  A value is therefore
 *      held for at most eight frames after the last valid sample.
 *   5. Store.  value = out (the float, never the uint16 rounding); the colour bits become this frame's colour, or are left
 *      unchanged without a guide.  The output is out; for KDE_DEPTH_U16 depth_to_u16(out), as kde_points_to_depth rounds.
 * Per frame, integer sums taken before the uint16 rounding: smoothed[f] = the linked branch of step 3; jumped[f] = z > 0 &&
 * prev > 0 and not linked; held[f] = step 4 with out > 0; changed[f] = step 2 fired on a pixel whose value was > 0.
 * The result is a function of the sequence since the last reset and nothing else: the bytes do not depend on how the sequence
 * is cut into calls, on n, pointer alignment, the pixels a thread owns or the frames it loads ahead.
 *
 * Several sensors are served by several objects; because the rule is per pixel they can also share one object on frames of
 * height S * H.  A sequence does not shard across GPUs: frame t needs the state frame t - 1 left.
 * ========================================================================================== */
typedef struct kde_temporal_params { float alpha; float max_diff; float rel_diff; int persist_min; int color_thresh; float z_min, z_max; } kde_temporal_params;
typedef struct kde_temporal kde_temporal;
/* alpha 0.4, max_diff 10 (millimetres), rel_diff 0.02 (DepthSpeckleFilter's link: the two stages agree on what one surface is),
 * persist_min 3, color_thresh 48, z_min 0, z_max FLT_MAX */
int kde_temporal_default_params(kde_temporal_params* p);
/* frames of width x height, at most max_batch of them per call, on the current device; p == NULL: the defaults.
 * KDE_ERR_INVALID: sizes below 1, width * height above 2^30, alpha outside (0, 1] (1: pass-through plus hold), max_diff or
 * rel_diff not finite or < 0, persist_min outside 0..8 (0: never hold), color_thresh outside 0..765 (765: the guide is never
 * consulted), z_min not finite or < 0, z_min >= z_max.  The object owns the state (two 4-byte words per pixel, zeroed here),
 * four counts per frame and per wavefront, and max_batch * width * height floats for calls with out_dev == NULL.  On a host
 * without a device the object is created without buffers: every call validates as usual and the launch then returns
 * KDE_ERR_HIP. */
int kde_temporal_create(kde_temporal** out, int width, int height, int max_batch, const kde_temporal_params* p);
int kde_temporal_destroy(kde_temporal* h);   /* NULL is a no-op */
/* The next n <= max_batch frames of the sequence: depth_dev is [n][height][width] of depth_format (KDE_DEPTH_F32 |
 * KDE_DEPTH_U16), bgr_dev is [n][height][width][3] bytes or NULL (no guide: step 2 does not run and the stored colour stays),
 * out_dev is [n][height][width] of out_format or NULL for the object-owned buffer.  Pointers need the alignment of their
 * element only.  In place is allowed exactly when out_dev == depth_dev and out_format == depth_format (each thread reads its
 * pixel of frame t before it writes it); any other overlap of the frames that are written -- out_dev's, or with out_dev == NULL
 * the object-owned buffer's, which kde_temporal_depth_device hands out -- with those of depth_dev is KDE_ERR_INVALID, and so is
 * their overlap with bgr_dev.  Two launches: the filter, in which a thread reads the state of its pixels once, walks the n
 * frames in time order with the state in registers and writes it once, and the sums of the counts.  No allocation, no host
 * synchronisation and no memset node: capturable from the first call.  Replaying a captured graph advances the stream by n
 * frames: a replay filters what the captured pointers hold then as the NEXT n frames of the sequence. */
int kde_temporal_filter_batch(kde_temporal* h, int n, const void* depth_dev, int depth_format, const uint8_t* bgr_dev /* NULL: no guide */,
                              int out_format, void* out_dev /* NULL: object-owned */, void* stream);
/* Both state words of every pixel become 0, as after create: the next frame starts a sequence.  A launch on `stream`, not a
 * memset node; capturable.  The getters below answer "kde_temporal_filter_batch was not called" again until the next call. */
int kde_temporal_reset(kde_temporal* h, void* stream);
/* The object-owned state in the layout above: value[height][width] float32 and hist[height][width] uint32, on the device
 * (both NULL for an object created without a device).  Reading it between calls checkpoints a stream; writing to it between
 * calls is allowed and is the way to restore a checkpoint, or to move a stream to another object with two copies.  The caller
 * orders its copies with the calls (the same stream, or an event). */
int kde_temporal_state_device(kde_temporal* h, float** value, uint32_t** hist);
/* A measurement knob, not a parameter: the pixels a thread owns (1, 2, 4, 8) and the frames whose loads it issues ahead of the
 * arithmetic (1, 2, 4); 0, 0: the library's choice, a function of the frame size and n (kde_temporal_shape reports it).  The
 * bytes of every result are the same for every shape.  KDE_ERR_INVALID for anything else. */
int kde_temporal_set_shape(kde_temporal* h, int pixels_per_thread, int unroll);
int kde_temporal_shape(kde_temporal* h, int n, int* pixels_per_thread, int* unroll);   /* what a call of n frames would run */
/* the frames of the last kde_temporal_filter_batch: out_dev of that call or the object-owned buffer, in that call's out_format;
 * valid until the next call or destroy.  KDE_ERR_INVALID before the first call and after kde_temporal_reset (this and the nine
 * getters below). */
int kde_temporal_depth_device(kde_temporal* h, void** out);
/* the same in pinned host memory after a blocking copy on `stream`: synchronises; out_dev of the last call must still be alive */
int kde_temporal_depth_host(kde_temporal* h, void* stream, const void** out);
int kde_temporal_smoothed_device(kde_temporal* h, uint32_t** out);   /* smoothed[n] of the last kde_temporal_filter_batch, on the device */
int kde_temporal_smoothed_host(kde_temporal* h, void* stream, const uint32_t** out);   /* in pinned host memory: synchronises */
int kde_temporal_jumped_device(kde_temporal* h, uint32_t** out);
int kde_temporal_jumped_host(kde_temporal* h, void* stream, const uint32_t** out);   /* synchronises */
int kde_temporal_held_device(kde_temporal* h, uint32_t** out);
int kde_temporal_held_host(kde_temporal* h, void* stream, const uint32_t** out);   /* synchronises */
int kde_temporal_changed_device(kde_temporal* h, uint32_t** out);
int kde_temporal_changed_host(kde_temporal* h, void* stream, const uint32_t** out);   /* synchronises */

/* ==========================================================================================
 * DepthDecimation: depth frames, and their colour guides, made `factor` times smaller each way.  Every stage above, and every
 * class of the reference, runs at the size of the frame it is given; this is the step down of a multi-resolution chain --
 * decimate, enhance at the small size, GuidedDepthUpsampling back under the full-resolution guide -- and the cheapest
 * denoiser there is.  An average pool mixes the sensor's 0 into valid depths and invents depths between two surfaces; strided
 * indexing throws k^2 - 1 of k^2 samples away.  This stage is hole-aware and edge-aware.  No reference counterpart.
 *
 * Frames: depth src_w x src_h (KDE_DEPTH_F32 or KDE_DEPTH_U16, uint16 widened by (float)u); k = factor, an integer in 2..8; the
 * output out_w = ceil(src_w / k) by out_h = ceil(src_h / k), in either format.  Output pixel (i, j) stands for the block of
 * source pixels qy = j * k .. min(j * k + k, src_h) - 1 (outer loop), qx = i * k .. min(i * k + k, src_w) - 1 (inner loop):
 * this loop order is the tap order.  Blocks on the right and bottom edge may be partial: they use only the samples that exist,
 * and nothing is scaled for them.
 *
 * The rule.  Every operation is one IEEE binary32 operation in the order written, the division correctly rounded; nothing
 * transcendental is evaluated.  Per output pixel:
 *   1. A sample is valid iff z > z_min && z < z_max (NaN and +-inf fail).
 *   2. m = the number of valid samples of the block.
 *   3. If m < min_valid the pixel is 0 (the sensor's "invalid").  A partial block with fewer existing samples than min_valid is
 *      therefore a hole.
 *   4. zmed = the lower median of the valid samples: sorted ascending to v[0 .. m - 1], v[(m - 1) / 2].  It is always one of the
 *      samples.
 *   5. mode KDE_DECIMATE_MEDIAN: the pixel is zmed.  It never lies between two surfaces; uint16 in to uint16 out is exact.
 *   6. mode KDE_DECIMATE_MEAN: num = 0, cnt = 0; for each valid sample in tap order with max_gap == 0 || fabsf(z - zmed) <=
 *      max_gap: num = num + z, cnt = cnt + 1.  The pixel is num / (float)cnt; cnt >= 1 because zmed passes its own test.
 *   7. The output is the float itself (KDE_DEPTH_F32) or depth_to_u16 of it as kde_points_to_depth rounds (KDE_DEPTH_U16).
 *   8. filled[f] = the number of non-hole output pixels of frame f, counted before the uint16 rounding.
 *   9. mixed[f] = the number of output pixels with m >= 1 whose largest valid sample minus smallest valid sample exceeds
 *      max_gap: the blocks that straddle a depth edge.  It is 0 for every frame when max_gap == 0.
 * The guide (kde_decimate_color_batch): per channel, s = the integer sum over the block's existing pixels and c their count;
 * the output is (2 * s + c) / (2 * c) in integer division, the area mean rounded half up.  It is exact; it does not claim to
 * equal OpenCV's INTER_AREA, which rounds half to even.
 * The camera (kde_decimate_intrinsics): fx' = fx / k, fy' = fy / k, cx' = (cx + 0.5) / k - 0.5, cy' likewise, in doubles on the
 * host: the pixel-centre rule, under which the centre of block (i, j) is pixel (i, j).  One limit: GuidedDepthUpsampling back to
 * src_w x src_h assumes both images cover the same view, which holds exactly only when both sides are multiples of k.
 * Every output pixel is a function of its own block and the counts are integer sums: the result is deterministic to the bit and
 * does not depend on n, a frame's position in the batch or pointer alignment.
 * ========================================================================================== */
enum { KDE_DECIMATE_MEDIAN = 0, KDE_DECIMATE_MEAN = 1 };
typedef struct kde_decimate_params { int factor; int mode; int min_valid; float max_gap; float z_min, z_max; } kde_decimate_params;
typedef struct kde_decimate kde_decimate;
/* factor 2, KDE_DECIMATE_MEDIAN, min_valid 1, max_gap 0 (no guard), z_min 0, z_max FLT_MAX */
int kde_decimate_default_params(kde_decimate_params* p);
/* source frames of src_w x src_h, at most max_batch of them per call, on the current device; p == NULL: the defaults.
 * KDE_ERR_INVALID: sizes below 1 or a side above 2^24, factor outside 2..8, mode neither 0 nor 1, min_valid outside
 * 1..factor^2, max_gap not finite or < 0, z_min not finite or < 0, z_min >= z_max.  The object owns filled[max_batch],
 * mixed[max_batch], a count pair per workgroup and max_batch * out_w * out_h floats for calls with out_dev == NULL.  On a host
 * without a device the object is created without buffers: every call validates as usual and the launch then returns
 * KDE_ERR_HIP. */
int kde_decimate_create(kde_decimate** out, int src_w, int src_h, int max_batch, const kde_decimate_params* p);
int kde_decimate_destroy(kde_decimate* h);   /* NULL is a no-op */
int kde_decimate_out_size(kde_decimate* h, int* out_w, int* out_h);   /* ceil(src_w / factor), ceil(src_h / factor); needs no device */
/* n <= max_batch frames: depth_dev is [n][src_h][src_w] of depth_format (KDE_DEPTH_F32 | KDE_DEPTH_U16), out_dev is
 * [n][out_h][out_w] of out_format or NULL for the object-owned buffer.  Pointers need the alignment of their element only:
 * whatever the alignment, a source row is read as the aligned 16-byte pieces inside it and as elements at its two ends, with
 * the same result.  In place is refused: the frames that are written -- out_dev's, or with out_dev == NULL the object-owned
 * buffer's, which kde_decimate_depth_device hands out -- must not overlap those of depth_dev (KDE_ERR_INVALID).  Two launches:
 * the decimation, whose workgroups each write their count pair, and the sum of those into filled[f] and mixed[f] -- no atomic,
 * no memset node and nothing to reset; no allocation, no host synchronisation: capturable from the first call. */
int kde_decimate_depth_batch(kde_decimate* h, int n, const void* depth_dev, int depth_format, int out_format, void* out_dev /* NULL: object-owned */,
                             void* stream);
/* the guides of n <= max_batch frames: bgr_dev is [n][src_h][src_w][3] bytes, out_bgr_dev [n][out_h][out_w][3]; any alignment;
 * the two must not overlap (KDE_ERR_INVALID).  One launch; it leaves the results of the last kde_decimate_depth_batch alone. */
int kde_decimate_color_batch(kde_decimate* h, int n, const uint8_t* bgr_dev, uint8_t* out_bgr_dev, void* stream);
/* K_out[9] = the row-major 3 x 3 camera matrix of the small image for K_in[9] of the source image (K_out may be K_in): the
 * rule above, the skew entries divided by k, the last row copied.  Doubles, on the host only: works without a device. */
int kde_decimate_intrinsics(kde_decimate* h, const double* K_in, double* K_out);
/* the frames of the last kde_decimate_depth_batch: out_dev of that call or the object-owned buffer, in that call's out_format;
 * valid until the next call or destroy.  KDE_ERR_INVALID before the first call (this and the five getters below). */
int kde_decimate_depth_device(kde_decimate* h, void** out);
/* the same in pinned host memory after a blocking copy on `stream`: synchronises; out_dev of the last call must still be alive */
int kde_decimate_depth_host(kde_decimate* h, void* stream, const void** out);
int kde_decimate_filled_device(kde_decimate* h, uint32_t** out);   /* filled[n] of the last kde_decimate_depth_batch, on the device */
int kde_decimate_filled_host(kde_decimate* h, void* stream, const uint32_t** out);   /* in pinned host memory: synchronises */
int kde_decimate_mixed_device(kde_decimate* h, uint32_t** out);
int kde_decimate_mixed_host(kde_decimate* h, void* stream, const uint32_t** out);   /* synchronises */

#ifdef __cplusplus
}
#endif
#endif /* KDE_HIP_H */
