// kde/kde.hpp — header-only C++ classes with the reference's names and member signatures for the hot
// path, forwarding to the C ABI of libkde_hip.so (include/kde_hip.h).
//
//   reference class (file)                                        -> class below
//   JointBilateralFilter        (JointBilateralFilter/JointBilateralFilter.h:9-36)
//   MarkovRandomField           (MarkovRandomField/MarkovRandomField.h)
//   DimensionConvertor          (DimensionConvertor/DimensionConvertor.h:152-171)
//   Buffer2D / ArrayBuffer      (ArrayBuffer/Buffer2D.h:9-37, ArrayBuffer.h:9-45)
//   DepthAdaptiveSuperpixel     (SuperpixelSegmentation/DepthAdaptiveSuperpixel.h:15-28)
//   EdgeRefinedSuperpixel       (EdgeRefinedSuperpixel/EdgeRefinedSuperpixel.h:14-45)
//   RegionGrowingBilateralFilter(RegionGrowingBilateralFilter.h:11-27)
//   SPDepthSuperResolution      (SPDepthSuperResolution.h:17-46)
//   LabelEquivalenceSeg         (LabelEquivalenceSeg/LabelEquivalenceSeg.h:7-49)
//   Projection_GPU              (Projection_GPU/Projection_GPU.h:8-42; the five-argument PlaneProjection)
//   KinectDepthEnhancement      (KinectDepthEnhancement.h:19-44)
//   kde::JointBilateralFilterFeed (extension: JointBilateralFilter on frames in host memory, main.cpp:160-163)
//   kde::KinectDepthEnhancementFeed, kde::pointsToDepth (extension: KinectDepthEnhancement on frames in host memory,
//                                 main.cpp:160-163, 198-202, with the result as a point cloud or a depth map)
//   kde::MeanError3D              (extension: the quality figure of main.cpp:220-308 for a batch, on the device)
//   kde::PointCloudXYZRGB         (extension: the coloured clouds of main.cpp:211-300 for a batch, compacted on the device)
//   kde::DepthRegistration        (extension: what Kinect.cpp:71-75 asks OpenNI for -- depth warped into the colour camera's view)
//   kde::LensUndistortion         (extension: frames of a camera with lens distortion resampled into the pinhole view assumed above)
//   kde::GuidedDepthUpsampling    (extension: low-resolution depth brought to the size of its colour image, guided by that image)
//
// What differs from the reference headers, and why:
//   * cv::gpu::GpuMat parameters are templates over "anything with .data/.rows/.cols/.step" — a real
//     cv::gpu::GpuMat binds unchanged, and builds without OpenCV can pass kde::GpuImage8UC3;
//   * cv::Mat_<double> intrinsic parameters are templates over "anything callable as K(row, col)"
//     (cv::Mat_<double> is) with an overload for a row-major double[9];
//   * failures throw kde::Error (std::runtime_error) instead of being ignored (the reference checks no
//     CUDA return code); nothing aborts;
//   * every object owns one stream-ordered context; an optional stream (void* = hipStream_t) can be set
//     with setStream(), default is the null stream like the reference;
//   * the viewer members (visualize, getSegmentedImage, getRandomColorImage) render into object-owned host images
//     (kde::HostImage8UC3, viewers.hpp) instead of cv::Mat_ / cv::imshow windows; releaseVideo() is a no-op;
//   * classes live in the global namespace like the reference's unless KDE_NO_GLOBAL_NAMES is defined
//     (then they are only reachable as kde::ref::Name).
#ifndef KDE_KDE_HPP
#define KDE_KDE_HPP

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../kde_hip.h"
#include "viewers.hpp"   // host-side renderers behind visualize() / getSegmentedImage() / getRandomColorImage()

#if defined(__has_include)
#if __has_include(<hip/hip_vector_types.h>)
#include <hip/hip_vector_types.h>   // float2 / float3 as the reference's CUDA headers provide them
#define KDE_HAVE_VECTOR_TYPES 1
#endif
#endif
#ifndef KDE_HAVE_VECTOR_TYPES
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
#endif

namespace kde {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& what) : std::runtime_error(what), code_(code) {}
    int code() const { return code_; }
private:
    int code_;
};

inline void check(int rc)
{
    if (rc != KDE_OK) throw Error(rc, std::string("libkde_hip: ") + kde_last_error_string());
}

// stand-in for a continuous CV_8UC3 cv::gpu::GpuMat (packed BGR on the device)
struct GpuImage8UC3 {
    uint8_t* data;
    int rows, cols;
    size_t step;
};

struct Mat33d {   // stand-in for cv::Mat_<double>(3,3)
    double v[9];
    double operator()(int r, int c) const { return v[r * 3 + c]; }
};

template <class MatLike>
inline void intrinsic_to_array(const MatLike& K, double out[9])
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) out[r * 3 + c] = static_cast<double>(K(r, c));
}
inline void intrinsic_to_array(const double* K, double out[9])
{
    for (int i = 0; i < 9; i++) out[i] = K[i];
}

static_assert(sizeof(float3) == sizeof(kde_float3), "float3 must be 12 bytes packed");

// every class takes a colour image as "continuous CV_8UC3 of the object's size" (cv::gpu::createContinuous,
// JointBilateralFilter.cpp:13, main.cpp:62): a padded or wrongly sized GpuMat is rejected, not silently misread
template <class GpuMatLike>
inline void require_continuous_8uc3(const GpuMatLike& img, int width, int height, const char* who)
{
    if (img.rows != height || img.cols != width || static_cast<size_t>(img.step) != static_cast<size_t>(width) * 3)
        throw Error(KDE_ERR_INVALID, std::string(who) + ": colour image must be a continuous " + std::to_string(width) + "x" +
                                         std::to_string(height) + " 8UC3 (step == 3 * width)");
}

namespace ref {

// ------------------------------------------------------------------------------------------------
class JointBilateralFilter {
public:
    JointBilateralFilter(int width, int height) : Width(width), Height(height)
    {
        check(kde_jbf_create(&h_, width, height, 1, nullptr));   // reference constants (JointBilateralFilter.cpp:3-6)
    }
    // extension: explicit parameters / batch capacity (the reference hard-codes them)
    JointBilateralFilter(int width, int height, const kde_jbf_params& params, int max_batch = 1)
        : Width(width), Height(height)
    {
        check(kde_jbf_create(&h_, width, height, max_batch, &params));
    }
    ~JointBilateralFilter() { kde_jbf_destroy(h_); }
    JointBilateralFilter(const JointBilateralFilter&) = delete;
    JointBilateralFilter& operator=(const JointBilateralFilter&) = delete;

    template <class GpuMatLike>
    void Process(float* depth_device, const GpuMatLike& color_image)
    {
        if (color_image.rows != Height || color_image.cols != Width)
            throw Error(KDE_ERR_INVALID, "JointBilateralFilter::Process: colour image size mismatch");
        check(kde_jbf_process(h_, depth_device, color_image.data, color_image.step, stream_));
    }
    void ProcessBatch(int n, const float* depth_device, const uint8_t* bgr_device, float* filtered_device = nullptr)
    {
        check(kde_jbf_process_batch(h_, n, depth_device, bgr_device, filtered_device, stream_));
    }
    float* getFiltered_Device() const
    {
        float* p = nullptr;
        check(kde_jbf_filtered_device(h_, &p));
        return p;
    }
    float* getFiltered_Host() const
    {
        const float* p = nullptr;
        check(kde_jbf_filtered_host(h_, stream_, &p));
        return const_cast<float*>(p);
    }
    GpuImage8UC3 getSmoothImage_Device()
    {
        uint8_t* p = nullptr;
        check(kde_jbf_smooth_device(h_, &p));
        return GpuImage8UC3{p, Height, Width, static_cast<size_t>(Width) * 3};
    }
    // void visualize(float* depth_host) (JointBilateralFilter.h:18, .cpp:50-79): refreshes Filtered_Host (in the reference this
    // member is the ONLY thing that does) and renders the caller's input depth and the filtered depth with the reference's
    // ramp over 5000 mm, pixels <= 50 mm black.  The reference then shows both with cv::imshow + cv::waitKey(1); windows are
    // outside the scope, the pictures are kept in the object instead (getInputDepthImage / getOutputDepthImage).
    void visualize(float* depth_host)
    {
        if (InputDepth.rows != Height) InputDepth = HostImage8UC3(Height, Width), OutputDepth = HostImage8UC3(Height, Width);
        viewers::render_depth(depth_host, 5000.0f, true, 50.0f, InputDepth);
        viewers::render_depth(getFiltered_Host(), 5000.0f, true, 50.0f, OutputDepth);
    }
    HostImage8UC3& getInputDepthImage() { return InputDepth; }       // extension: what "depth_input" would have shown
    HostImage8UC3& getOutputDepthImage() { return OutputDepth; }     // extension: what "depth_filtered" would have shown
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_jbf* handle() const { return h_; }
    // extension: the name of the kernel this object's parameters select ("generic-32x8-1px" when no tuned one applies:
    // window 1, a zero sigma, or a colour sigma outside the tuned range); kde_jbf_active_variant
    const char* activeKernel() const
    {
        int v = 0;
        check(kde_jbf_active_variant(h_, &v));
        return kde_jbf_variant_name(v);
    }

private:
    int Width, Height;
    kde_jbf* h_ = nullptr;
    void* stream_ = nullptr;
    HostImage8UC3 InputDepth, OutputDepth;
};

// ------------------------------------------------------------------------------------------------
class MarkovRandomField {
public:
    MarkovRandomField(int width, int height) : Width(width), Height(height)
    {
        check(kde_mrf_create(&h_, width, height, 1, 0, -1.0f, -1.0f));   // MarkovRandomField.cpp:3-6
    }
    ~MarkovRandomField() { kde_mrf_destroy(h_); }
    MarkovRandomField(const MarkovRandomField&) = delete;
    MarkovRandomField& operator=(const MarkovRandomField&) = delete;
    template <class GpuMatLike>
    void Process(float* depth_device, const GpuMatLike& color_image)
    {
        if (color_image.rows != Height || color_image.cols != Width || color_image.step != static_cast<size_t>(Width) * 3)
            throw Error(KDE_ERR_INVALID, "MarkovRandomField::Process: colour image must be continuous WxH 8UC3");
        check(kde_mrf_process_batch(h_, 1, depth_device, color_image.data, nullptr, stream_));
    }
    float* getFiltered_Device() const
    {
        float* p = nullptr;
        check(kde_mrf_filtered_device(h_, &p));
        return p;
    }
    float* getFiltered_Host() const      // MarkovRandomField.h:16
    {
        const float* p = nullptr;
        check(kde_mrf_filtered_host(h_, stream_, &p));
        return const_cast<float*>(p);
    }
    // cv::gpu::GpuMat getSmoothImage_Device() (MarkovRandomField.h:17): the reference allocates smooth_Device and never
    // writes it (MarkovRandomField.cpp:13, no kernel takes it) -- there is nothing to return but an empty image
    GpuImage8UC3 getSmoothImage_Device() { return GpuImage8UC3{nullptr, 0, 0, 0}; }
    // void visualize(float* depth_host) (MarkovRandomField.h:18, .cpp:50-79): as JointBilateralFilter::visualize
    void visualize(float* depth_host)
    {
        if (InputDepth.rows != Height) InputDepth = HostImage8UC3(Height, Width), OutputDepth = HostImage8UC3(Height, Width);
        viewers::render_depth(depth_host, 5000.0f, true, 50.0f, InputDepth);
        viewers::render_depth(getFiltered_Host(), 5000.0f, true, 50.0f, OutputDepth);
    }
    HostImage8UC3& getInputDepthImage() { return InputDepth; }
    HostImage8UC3& getOutputDepthImage() { return OutputDepth; }
    void setStream(void* hip_stream) { stream_ = hip_stream; }

private:
    int Width, Height;
    kde_mrf* h_ = nullptr;
    void* stream_ = nullptr;
    HostImage8UC3 InputDepth, OutputDepth;
};

// ------------------------------------------------------------------------------------------------
class DimensionConvertor {
public:
    DimensionConvertor() { check(kde_dimconv_create(&h_)); }
    ~DimensionConvertor() { kde_dimconv_destroy(h_); }
    DimensionConvertor(const DimensionConvertor&) = delete;
    DimensionConvertor& operator=(const DimensionConvertor&) = delete;

    template <class MatLike>
    void setCameraParameters(const MatLike& intrinsic, int width, int height)
    {
        double K[9];
        intrinsic_to_array(intrinsic, K);
        check(kde_dimconv_set_camera(h_, K, width, height));
    }
    void projectiveToReal(float* data, float3* out)
    {
        check(kde_dimconv_projective_to_real_depth(h_, 1, data, reinterpret_cast<kde_float3*>(out), stream_));
    }
    void projectiveToReal(float3* data, float3* out)
    {
        check(kde_dimconv_projective_to_real_points(h_, 1, reinterpret_cast<const kde_float3*>(data),
                                                    reinterpret_cast<kde_float3*>(out), stream_));
    }
    void projectiveToRealInterp(float* data, float3* out)
    {
        check(kde_dimconv_projective_to_real_interp(h_, 1, data, reinterpret_cast<kde_float3*>(out), stream_));
    }
    void realToProjective(float3* data, float3* out)
    {
        check(kde_dimconv_real_to_projective(h_, 1, reinterpret_cast<const kde_float3*>(data),
                                             reinterpret_cast<kde_float3*>(out), stream_));
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }

private:
    kde_dimconv* h_ = nullptr;
    void* stream_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
class ArrayBuffer {
public:
    typedef kde_weighted_d weighted_d;   // ArrayBuffer.h:12-15
    virtual ~ArrayBuffer() {}
    virtual void insertData(float* data) = 0;
    virtual void insertData(weighted_d* data) = 0;
    virtual void getDepthMap(float* out) = 0;
    virtual void getWeightMap(float* out) = 0;
    virtual void updateData(float* data) = 0;
};

class Buffer2D : public ArrayBuffer {
public:
    explicit Buffer2D(int width, int height) { check(kde_buffer2d_create(&h_, width, height)); }
    ~Buffer2D() override { kde_buffer2d_destroy(h_); }
    Buffer2D(const Buffer2D&) = delete;
    Buffer2D& operator=(const Buffer2D&) = delete;

    void insertData(float* data) override { check(kde_buffer2d_insert_depth(h_, data, stream_)); }
    void insertData(weighted_d* data) override { check(kde_buffer2d_insert_weighted(h_, data, stream_)); }
    void insertData(float2* data) { check(kde_buffer2d_insert_float2(h_, reinterpret_cast<const float*>(data), stream_)); }
    void getDepthMap(float* out) override { check(kde_buffer2d_get_depth_map(h_, out, stream_)); }
    void getWeightMap(float* out) override { check(kde_buffer2d_get_weight_map(h_, out, stream_)); }
    void updateData(float* data) override { check(kde_buffer2d_update(h_, data, stream_)); }
    // extension: n_frames consecutive frames fused into one pass over the buffer
    void updateData(float* data, int n_frames) { check(kde_buffer2d_update_sequence(h_, n_frames, data, stream_)); }
    weighted_d* getRawPointer()
    {
        weighted_d* p = nullptr;
        check(kde_buffer2d_raw_pointer(h_, &p));
        return p;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }

private:
    kde_buffer2d* h_ = nullptr;
    void* stream_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
class DepthAdaptiveSuperpixel {
public:
    typedef kde_superpixel superpixel;             // SuperpixelSegmentation.h:17-24
    typedef kde_label_distance label_distance;     // :26-29
    DepthAdaptiveSuperpixel(int width, int height) : Width(width), Height(height) { check(kde_dasp_create(&h_, width, height)); }
    virtual ~DepthAdaptiveSuperpixel() { kde_dasp_destroy(h_); }
    DepthAdaptiveSuperpixel(const DepthAdaptiveSuperpixel&) = delete;
    DepthAdaptiveSuperpixel& operator=(const DepthAdaptiveSuperpixel&) = delete;

    template <class MatLike>
    void SetParametor(int rows, int cols, const MatLike& intrinsic)   // [sic]
    {
        double K[9];
        intrinsic_to_array(intrinsic, K);
        check(kde_dasp_set_parameters(h_, rows, cols, K));
    }
    template <class GpuMatLike>
    void Segmentation(const GpuMatLike& color_image, float3* points3d_device, float color_sigma,
                      float spatial_sigma, float depth_sigma, int iteration)
    {
        require_continuous_8uc3(color_image, Width, Height, "DepthAdaptiveSuperpixel::Segmentation");
        check(kde_dasp_segmentation(h_, color_image.data, reinterpret_cast<const kde_float3*>(points3d_device),
                                    color_sigma, spatial_sigma, depth_sigma, iteration, stream_));
    }
    int* getLabelDevice()
    {
        int32_t* p = nullptr;
        check(kde_dasp_labels_device(h_, &p));
        return p;
    }
    superpixel* getMeanDataDevice()
    {
        superpixel* p = nullptr;
        check(kde_dasp_mean_device(h_, &p));
        return p;
    }
    // ---- viewer members of the base class (SuperpixelSegmentation.h:36-41, .cpp:50-200); host side, no window, no video ----
    static const int Line = 0, Average = 1;
    // options == Line: the input with segment borders in white; otherwise every pixel in its cluster's mean colour
    // (.r,.g,.b into channels 0,1,2 as the reference writes them), label -1 black
    template <class ImageLike>
    HostImage8UC3& getSegmentedImage(const ImageLike& input_host, int options)
    {
        const int32_t* labels = nullptr;
        check(kde_dasp_labels_host(h_, stream_, &labels));
        if (SegmentedColor.rows != Height) SegmentedColor = HostImage8UC3(Height, Width);
        if (options == Line) {
            viewers::copy_from(input_host, SegmentedColor);
            viewers::mark_label_borders(labels, SegmentedColor);
        } else {
            const superpixel* mean = nullptr;
            int count = 0;
            check(kde_dasp_mean_host(h_, stream_, &mean, &count));
            for (int y = 0; y < Height; y++)
                for (int x = 0; x < Width; x++) {
                    const int32_t id = labels[static_cast<size_t>(y) * Width + x];
                    if (id >= 0 && id < count) SegmentedColor.set(y, x, mean[id].r, mean[id].g, mean[id].b);
                    else SegmentedColor.set(y, x, 0, 0, 0);
                }
        }
        return SegmentedColor;
    }
    HostImage8UC3& getRandomColorImage()
    {
        const int32_t* labels = nullptr;
        check(kde_dasp_labels_host(h_, stream_, &labels));
        if (SegmentedRandomColor.rows != Height) SegmentedRandomColor = HostImage8UC3(Height, Width);
        viewers::render_random_colours(labels, SegmentedRandomColor);
        return SegmentedRandomColor;
    }
    void releaseVideo() {}      // the reference's constructor opens an .avi writer (SuperpixelSegmentation.cpp:9); this one does not
    void setStream(void* hip_stream) { stream_ = hip_stream; }

private:
    int Width, Height;
    kde_dasp* h_ = nullptr;
    void* stream_ = nullptr;
    HostImage8UC3 SegmentedColor, SegmentedRandomColor;
};

// ------------------------------------------------------------------------------------------------
class EdgeRefinedSuperpixel {
public:
    EdgeRefinedSuperpixel(int width, int height) : Width(width), Height(height) { check(kde_ers_create(&h_, width, height)); }
    ~EdgeRefinedSuperpixel() { kde_ers_destroy(h_); }
    EdgeRefinedSuperpixel(const EdgeRefinedSuperpixel&) = delete;
    EdgeRefinedSuperpixel& operator=(const EdgeRefinedSuperpixel&) = delete;

    template <class GpuMatLike>
    void EdgeRefining(int* color_label_device, int* depth_label_device, float* depth_device, const GpuMatLike& color_image)
    {
        require_continuous_8uc3(color_image, Width, Height, "EdgeRefinedSuperpixel::EdgeRefining");
        check(kde_ers_edge_refining(h_, color_label_device, depth_label_device, depth_device, color_image.data, stream_));
    }
    int* getRefinedLabels_Device()
    {
        int32_t* p = nullptr;
        check(kde_ers_refined_labels_device(h_, &p));
        return p;
    }
    int* getRefinedLabels_Host()
    {
        const int32_t* p = nullptr;
        check(kde_ers_refined_labels_host(h_, stream_, &p));
        return const_cast<int*>(p);
    }
    float* getRefinedDepth_Device()
    {
        float* p = nullptr;
        check(kde_ers_refined_depth_device(h_, &p));
        return p;
    }
    float* getRefinedDepth_Host()
    {
        const float* p = nullptr;
        check(kde_ers_refined_depth_host(h_, stream_, &p));
        return const_cast<float*>(p);
    }
    // ---- viewer members (EdgeRefinedSuperpixel.h:27-29, .cpp:70-147); host side ----
    // refined depth on the reference's ramp over 3000 mm (`max_depth` is ignored there too, .cpp:79-80); then, except in the
    // last row / column: depth == 0 black, segment borders and label -100 white
    HostImage8UC3& getSegmentedImage(const int max_depth)
    {
        (void)max_depth;
        const float* depth = getRefinedDepth_Host();
        const int32_t* labels = getRefinedLabels_Host();
        if (segmentedImage.rows != Height) segmentedImage = HostImage8UC3(Height, Width);
        viewers::render_depth(depth, 3000.0f, false, 0.0f, segmentedImage);
        for (int y = 0; y + 1 < Height; y++)
            for (int x = 0; x + 1 < Width; x++) {
                const size_t q = static_cast<size_t>(y) * Width + x;
                if (depth[q] == 0.0f) segmentedImage.set(y, x, 0, 0, 0);
                if (labels[q] != labels[q + Width] || labels[q] != labels[q + 1] || labels[q] == -100) segmentedImage.set(y, x, 255, 255, 255);
            }
        return segmentedImage;
    }
    template <class ImageLike>
    HostImage8UC3& getSegmentedImage(const ImageLike& input_host)
    {
        if (SegmentedColor.rows != Height) SegmentedColor = HostImage8UC3(Height, Width);
        viewers::copy_from(input_host, SegmentedColor);
        viewers::mark_label_borders(getRefinedLabels_Host(), SegmentedColor);
        return SegmentedColor;
    }
    HostImage8UC3& getRandomColorImage()
    {
        if (SegmentedRandomColor.rows != Height) SegmentedRandomColor = HostImage8UC3(Height, Width);
        viewers::render_random_colours(getRefinedLabels_Host(), SegmentedRandomColor);
        return SegmentedRandomColor;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }

private:
    int Width, Height;
    kde_ers* h_ = nullptr;
    void* stream_ = nullptr;
    HostImage8UC3 segmentedImage, SegmentedColor, SegmentedRandomColor;
};

// ------------------------------------------------------------------------------------------------
class RegionGrowingBilateralFilter {
public:
    RegionGrowingBilateralFilter(int width, int height) : Width(width), Height(height) { check(kde_rgbf_create(&h_, width, height)); }
    // extension: buffers for max_batch independent frames per ProcessBatch (the reference processes one frame per call)
    RegionGrowingBilateralFilter(int width, int height, int max_batch) : Width(width), Height(height)
    {
        check(kde_rgbf_create_batch(&h_, width, height, max_batch));
    }
    ~RegionGrowingBilateralFilter() { kde_rgbf_destroy(h_); }
    RegionGrowingBilateralFilter(const RegionGrowingBilateralFilter&) = delete;
    RegionGrowingBilateralFilter& operator=(const RegionGrowingBilateralFilter&) = delete;

    template <class MatLike>
    void SetParametor(int rows, int cols, const MatLike& intrinsic)   // [sic]
    {
        double K[9];
        intrinsic_to_array(intrinsic, K);
        check(kde_rgbf_set_parameters(h_, rows, cols, K));
    }
    template <class GpuMatLike>
    void Process(float* depth_device, float3* points_device, const GpuMatLike& color_device)
    {
        require_continuous_8uc3(color_device, Width, Height, "RegionGrowingBilateralFilter::Process");
        check(kde_rgbf_process(h_, depth_device, reinterpret_cast<const kde_float3*>(points_device), color_device.data, stream_));
    }
    // n frames back to back in every argument; the getters then return n frames back to back, each bit-identical to Process
    void ProcessBatch(int n, const float* depth_device, const float3* points_device, const uint8_t* bgr_device)
    {
        check(kde_rgbf_process_batch(h_, n, depth_device, reinterpret_cast<const kde_float3*>(points_device), bgr_device, stream_));
    }
    float* getRefinedDepth_Device()
    {
        float* p = nullptr;
        check(kde_rgbf_refined_depth_device(h_, &p));
        return p;
    }
    float* getRefinedDepth_Host()
    {
        const float* p = nullptr;
        check(kde_rgbf_refined_depth_host(h_, stream_, &p));
        return const_cast<float*>(p);
    }
    int* getRefinedLabels_Device()
    {
        int32_t* p = nullptr;
        check(kde_rgbf_refined_labels_device(h_, &p));
        return p;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }

private:
    int Width, Height;
    kde_rgbf* h_ = nullptr;
    void* stream_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
class SPDepthSuperResolution {
public:
    SPDepthSuperResolution(int width, int height) : Width(width), Height(height) { check(kde_spdsr_create(&h_, width, height)); }
    SPDepthSuperResolution(int width, int height, int max_batch) : Width(width), Height(height)      // extension, as RGBF's
    {
        check(kde_spdsr_create_batch(&h_, width, height, max_batch));
    }
    ~SPDepthSuperResolution() { kde_spdsr_destroy(h_); }
    SPDepthSuperResolution(const SPDepthSuperResolution&) = delete;
    SPDepthSuperResolution& operator=(const SPDepthSuperResolution&) = delete;

    template <class MatLike>
    void SetParametor(int rows, int cols, const MatLike& intrinsic)   // [sic]
    {
        double K[9];
        intrinsic_to_array(intrinsic, K);
        check(kde_spdsr_set_parameters(h_, rows, cols, K));
    }
    template <class GpuMatLike>
    void Process(float* depth_device, float3* points_device, const GpuMatLike& color_device)
    {
        require_continuous_8uc3(color_device, Width, Height, "SPDepthSuperResolution::Process");
        check(kde_spdsr_process(h_, depth_device, reinterpret_cast<const kde_float3*>(points_device), color_device.data, stream_));
    }
    void ProcessBatch(int n, const float* depth_device, const float3* points_device, const uint8_t* bgr_device)
    {
        check(kde_spdsr_process_batch(h_, n, depth_device, reinterpret_cast<const kde_float3*>(points_device), bgr_device, stream_));
    }
    float* getRefinedDepth_Device()
    {
        float* p = nullptr;
        check(kde_spdsr_refined_depth_device(h_, &p));
        return p;
    }
    float* getRefinedDepth_Host()
    {
        const float* p = nullptr;
        check(kde_spdsr_refined_depth_host(h_, stream_, &p));
        return const_cast<float*>(p);
    }
    float3* getEdgeEnhanced3DPoints_Device()
    {
        kde_float3* p = nullptr;
        check(kde_spdsr_edge_enhanced_points_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    float3* getOptimizedPoints_Device()
    {
        kde_float3* p = nullptr;
        check(kde_spdsr_optimized_points_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    float3* getOptimizedPoints_Host()
    {
        const kde_float3* p = nullptr;
        check(kde_spdsr_optimized_points_host(h_, stream_, &p));
        return reinterpret_cast<float3*>(const_cast<kde_float3*>(p));
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }

private:
    int Width, Height;
    kde_spdsr* h_ = nullptr;
    void* stream_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
// NormalEstimation/NormalMapGenerator.h: per-pixel normals of points in millimetres (projectiveToReal's output)
class NormalMapGenerator {
public:
    static const int SDC = KDE_NORMALS_SDC, CM = KDE_NORMALS_CM, BILATERAL = KDE_NORMALS_BILATERAL;   // NormalMapGenerator.h:28
    NormalMapGenerator(int w, int h) : Width(w), Height(h) { check(kde_normals_create(&h_, w, h, 1, nullptr)); }
    ~NormalMapGenerator() { kde_normals_destroy(h_); }
    NormalMapGenerator(const NormalMapGenerator&) = delete;
    NormalMapGenerator& operator=(const NormalMapGenerator&) = delete;
    void setNormalEstimationMethods(int method) { check(kde_normals_set_method(h_, method)); }   // SDC throws UNSUPPORTED
    void generateNormalMap(float3* vertices_device)
    {
        check(kde_normals_generate_batch(h_, 1, reinterpret_cast<const kde_float3*>(vertices_device), nullptr, stream_));
    }
    float3* getNormalMap()
    {
        kde_float3* p = nullptr;
        check(kde_normals_normal_map_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    // cv::Mat getNormalImg() (NormalMapGenerator.cu:423-439): (int)(255*(n+1.0)/2) per component, host-side
    HostImage8UC3& getNormalImg()
    {
        const kde_float3* p = nullptr;
        check(kde_normals_normal_map_host(h_, stream_, &p));
        if (NormalImg.rows != Height) NormalImg = HostImage8UC3(Height, Width);
        viewers::render_normals(reinterpret_cast<const float*>(p), NormalImg);
        return NormalImg;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_normals* handle() const { return h_; }

private:
    int Width, Height;
    kde_normals* h_ = nullptr;
    void* stream_ = nullptr;
    HostImage8UC3 NormalImg;
};

// ------------------------------------------------------------------------------------------------
// SuperpixelSegmentation/NormalAdaptiveSuperpixel.h:15-38 (derived from DepthAdaptiveSuperpixel there; here a class of
// its own over kde_nasp_* with the inherited members it is used through): superpixels on colour, position, depth and
// surface normal, the consumer of NormalMapGenerator::getNormalMap() in KinectDepthEnhancement.cpp:65-67
class NormalAdaptiveSuperpixel {
public:
    typedef kde_superpixel superpixel;             // SuperpixelSegmentation.h:17-24
    typedef kde_label_distance label_distance;     // :26-29
    NormalAdaptiveSuperpixel(int width, int height) : Width(width), Height(height) { check(kde_nasp_create(&h_, width, height, 1)); }
    virtual ~NormalAdaptiveSuperpixel() { kde_nasp_destroy(h_); }
    NormalAdaptiveSuperpixel(const NormalAdaptiveSuperpixel&) = delete;
    NormalAdaptiveSuperpixel& operator=(const NormalAdaptiveSuperpixel&) = delete;

    template <class MatLike>
    void SetParametor(int rows, int cols, const MatLike& intrinsic)   // [sic], inherited (DepthAdaptiveSuperpixel.cpp:15-39)
    {
        double K[9];
        intrinsic_to_array(intrinsic, K);
        check(kde_nasp_set_parameters(h_, rows, cols, K));
    }
    template <class GpuMatLike>
    void Segmentation(const GpuMatLike& color_image, float3* points3d_device, float3* normals_device, float color_sigma,
                      float spatial_sigma, float depth_sigma, float normal_sigma, int iteration)
    {
        require_continuous_8uc3(color_image, Width, Height, "NormalAdaptiveSuperpixel::Segmentation");
        check(kde_nasp_segmentation(h_, color_image.data, reinterpret_cast<const kde_float3*>(points3d_device),
                                    reinterpret_cast<const kde_float3*>(normals_device), color_sigma, spatial_sigma, depth_sigma,
                                    normal_sigma, iteration, stream_));
    }
    int* getLabelDevice()
    {
        int32_t* p = nullptr;
        check(kde_nasp_labels_device(h_, &p));
        return p;
    }
    superpixel* getMeanDataDevice()
    {
        superpixel* p = nullptr;
        check(kde_nasp_mean_device(h_, &p));
        return p;
    }
    float3* getCentersDevice()
    {
        kde_float3* p = nullptr;
        check(kde_nasp_centers_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    float3* getNormalsDevice()
    {
        kde_float3* p = nullptr;
        check(kde_nasp_normals_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    float* getNormalsVarianceDevice()
    {
        float* p = nullptr;
        check(kde_nasp_normals_variance_device(h_, &p));
        return p;
    }
    // the *_Host members: object-owned pinned copies, refreshed by a blocking copy on the object's stream
    float3* getCentersHost()
    {
        const kde_float3* p = nullptr;
        int count = 0;
        check(kde_nasp_centers_host(h_, stream_, &p, &count));
        return reinterpret_cast<float3*>(const_cast<kde_float3*>(p));
    }
    float3* getNormalsHost()
    {
        const kde_float3* p = nullptr;
        int count = 0;
        check(kde_nasp_normals_host(h_, stream_, &p, &count));
        return reinterpret_cast<float3*>(const_cast<kde_float3*>(p));
    }
    float* getNormalsVarianceHost()
    {
        const float* p = nullptr;
        int count = 0;
        check(kde_nasp_normals_variance_host(h_, stream_, &p, &count));
        return const_cast<float*>(p);
    }
    // cv::Mat_<cv::Vec3b> getNormalImg() (NormalAdaptiveSuperpixel.cpp:38-54): per pixel its superpixel's normal as
    // (unsigned char)(255*(n+1)/2); label -1 (and any label outside the table) renders black instead of indexing element -1
    HostImage8UC3& getNormalImg()
    {
        const int32_t* labels = nullptr;
        const kde_float3* n = nullptr;
        int count = 0;
        check(kde_nasp_labels_host(h_, stream_, &labels));
        check(kde_nasp_normals_host(h_, stream_, &n, &count));
        if (normalImage.rows != Height) normalImage = HostImage8UC3(Height, Width);
        for (int y = 0; y < Height; y++)
            for (int x = 0; x < Width; x++) {
                const int32_t id = labels[static_cast<size_t>(y) * Width + x];
                if (id >= 0 && id < count)
                    normalImage.set(y, x, viewers::normal_byte(n[id].x), viewers::normal_byte(n[id].y), viewers::normal_byte(n[id].z));
                else normalImage.set(y, x, 0, 0, 0);
            }
        return normalImage;
    }
    // ---- viewer members of the base class, as DepthAdaptiveSuperpixel has them ----
    static const int Line = 0, Average = 1;
    template <class ImageLike>
    HostImage8UC3& getSegmentedImage(const ImageLike& input_host, int options)
    {
        const int32_t* labels = nullptr;
        check(kde_nasp_labels_host(h_, stream_, &labels));
        if (SegmentedColor.rows != Height) SegmentedColor = HostImage8UC3(Height, Width);
        if (options == Line) {
            viewers::copy_from(input_host, SegmentedColor);
            viewers::mark_label_borders(labels, SegmentedColor);
        } else {
            const superpixel* mean = nullptr;
            int count = 0;
            check(kde_nasp_mean_host(h_, stream_, &mean, &count));
            for (int y = 0; y < Height; y++)
                for (int x = 0; x < Width; x++) {
                    const int32_t id = labels[static_cast<size_t>(y) * Width + x];
                    if (id >= 0 && id < count) SegmentedColor.set(y, x, mean[id].r, mean[id].g, mean[id].b);
                    else SegmentedColor.set(y, x, 0, 0, 0);
                }
        }
        return SegmentedColor;
    }
    HostImage8UC3& getRandomColorImage()
    {
        const int32_t* labels = nullptr;
        check(kde_nasp_labels_host(h_, stream_, &labels));
        if (SegmentedRandomColor.rows != Height) SegmentedRandomColor = HostImage8UC3(Height, Width);
        viewers::render_random_colours(labels, SegmentedRandomColor);
        return SegmentedRandomColor;
    }
    void releaseVideo() {}
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_nasp* handle() const { return h_; }

private:
    int Width, Height;
    kde_nasp* h_ = nullptr;
    void* stream_ = nullptr;
    HostImage8UC3 SegmentedColor, SegmentedRandomColor, normalImage;
};

// ------------------------------------------------------------------------------------------------
// LabelEquivalenceSeg/LabelEquivalenceSeg.h:7-49: merges 4-adjacent superpixels with similar plane parameters into regions
// (kde_les_*), the consumer of NormalAdaptiveSuperpixel's cluster outputs in KinectDepthEnhancement.cpp:76.  The reference
// class sizes every table W*H and never learns how many superpixels there are; here setClusterCount() says it (rows * cols
// of the segmentation that feeds it) before the first labelImage.
class LabelEquivalenceSeg {
public:
    LabelEquivalenceSeg(int width, int height) : Width(width), Height(height) { check(kde_les_create(&h_, width, height, 1, nullptr)); }
    ~LabelEquivalenceSeg() { kde_les_destroy(h_); }
    LabelEquivalenceSeg(const LabelEquivalenceSeg&) = delete;
    LabelEquivalenceSeg& operator=(const LabelEquivalenceSeg&) = delete;

    void setClusterCount(int n_clusters) { Clusters = n_clusters; }   // added: the length of the three cluster tables
    // LabelEquivalenceSeg.cu:228-282; variance_device is dead in the reference and never read
    void labelImage(float3* cluster_normals_device, int* cluster_label_device, float3* cluster_centers_device, float* variance_device)
    {
        check(kde_les_label_image(h_, reinterpret_cast<const kde_float3*>(cluster_normals_device), cluster_label_device,
                                  reinterpret_cast<const kde_float3*>(cluster_centers_device), variance_device, Clusters, stream_));
    }
    float4* getMergedClusterND_Device() const
    {
        kde_float4* p = nullptr;
        check(kde_les_merged_nd_device(h_, &p));
        return reinterpret_cast<float4*>(p);
    }
    int* getMergedClusterLabel_Device() const
    {
        int32_t* p = nullptr;
        check(kde_les_merged_label_device(h_, &p));
        return p;
    }
    float* getMergedClusterVariance_Device() const
    {
        float* p = nullptr;
        check(kde_les_merged_variance_device(h_, &p));
        return p;
    }
    int* getMergedClusterSize_Device() const
    {
        int32_t* p = nullptr;
        check(kde_les_merged_size_device(h_, &p));
        return p;
    }
    // the *_Host members: object-owned pinned copies, refreshed by a blocking copy on the object's stream
    float4* getMergedClusterND_Host() const
    {
        const kde_float4* p = nullptr;
        check(kde_les_merged_nd_host(h_, stream_, &p));
        return reinterpret_cast<float4*>(const_cast<kde_float4*>(p));
    }
    int* getMergedClusterLabel_Host() const
    {
        const int32_t* p = nullptr;
        check(kde_les_merged_label_host(h_, stream_, &p));
        return const_cast<int32_t*>(p);
    }
    // cv::Mat_<cv::Vec3b> getSegmentResult() (LabelEquivalenceSeg.cpp:87-108): one colour per merged label, black where it is -1
    HostImage8UC3& getSegmentResult()
    {
        if (show.rows != Height) show = HostImage8UC3(Height, Width);
        viewers::render_merged_labels(getMergedClusterLabel_Host(), show);
        return show;
    }
    // cv::Mat_<cv::Vec3b> getNormalImg() (LabelEquivalenceSeg.cpp:109-124)
    HostImage8UC3& getNormalImg()
    {
        if (normalImage.rows != Height) normalImage = HostImage8UC3(Height, Width);
        viewers::render_merged_normals(getMergedClusterLabel_Host(), reinterpret_cast<const float*>(getMergedClusterND_Host()), normalImage);
        return normalImage;
    }
    void viewSegmentResult() { (void)getSegmentResult(); }   // .cpp:63-86 without the .avi writer and cv::imshow
    void releaseVideo() {}
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_les* handle() const { return h_; }

private:
    int Width, Height, Clusters = 0;
    kde_les* h_ = nullptr;
    void* stream_ = nullptr;
    HostImage8UC3 show, normalImage;
};

// ------------------------------------------------------------------------------------------------
// Projection_GPU/Projection_GPU.h:8-42, the five-argument PlaneProjection (kde_proj_*): the consumer of LabelEquivalenceSeg's
// four outputs in KinectDepthEnhancement.cpp:79-80.  The reference class cannot know how long the variance and size
// tables are; here setClusterCount() says it (rows * cols of the segmentation) before the first PlaneProjection.  The
// three-argument overload runs inside SPDepthSuperResolution::Process; the float3-normals overload has no caller.
class Projection_GPU {
public:
    static constexpr int WindowSize = 7;            // Projection_GPU.cpp:3-5
    static constexpr float SpatialSigma = 20.0f;
    static constexpr float DepthSigma = 100.0f;
    template <class MatLike>
    Projection_GPU(int width, int height, const MatLike& intrinsic) : Width(width), Height(height)
    {
        double k[9];
        intrinsic_to_array(intrinsic, k);
        check(kde_proj_create(&h_, width, height, 1, k, nullptr));
    }
    ~Projection_GPU() { kde_proj_destroy(h_); }
    Projection_GPU(const Projection_GPU&) = delete;
    Projection_GPU& operator=(const Projection_GPU&) = delete;

    void setClusterCount(int n_clusters) { Clusters = n_clusters; }   // added: the length of the variance and size tables
    // Projection_GPU.cu:248-272
    void PlaneProjection(const float4* nd_device, const int* labels_device, const float* variance_device, const float3* points3d_device,
                         int* size_device)
    {
        check(kde_proj_plane_projection(h_, reinterpret_cast<const kde_float4*>(nd_device), labels_device, variance_device,
                                        reinterpret_cast<const kde_float3*>(points3d_device), size_device, Clusters, stream_));
    }
    float3* GetPlaneFitted3D_Device() const
    {
        kde_float3* p = nullptr;
        check(kde_proj_plane_fitted_points_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    float3* GetOptimized3D_Device() const
    {
        kde_float3* p = nullptr;
        check(kde_proj_optimized_points_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    // the *_Host members: object-owned pinned copies, refreshed by a blocking copy on the object's stream
    float3* GetPlaneFitted3D_Host() const
    {
        const kde_float3* p = nullptr;
        check(kde_proj_plane_fitted_points_host(h_, stream_, &p));
        return reinterpret_cast<float3*>(const_cast<kde_float3*>(p));
    }
    float3* GetOptimized3D_Host() const
    {
        const kde_float3* p = nullptr;
        check(kde_proj_optimized_points_host(h_, stream_, &p));
        return reinterpret_cast<float3*>(const_cast<kde_float3*>(p));
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_proj* handle() const { return h_; }

private:
    int Width, Height, Clusters = 0;
    kde_proj* h_ = nullptr;
    void* stream_ = nullptr;
};

// ------------------------------------------------------------------------------------------------
// KinectDepthEnhancement.h:19-44 (kde_enh_*): the "PROPOSED" method of main.cpp:198-202.  getRefinedDepth_Device / _Host
// (.cpp:82-87) are not built: they return a buffer of the EdgeRefinedSuperpixel member that Process never writes.
class KinectDepthEnhancement {
public:
    KinectDepthEnhancement(int width, int height) : KinectDepthEnhancement(width, height, 1) {}
    // added: buffers for max_batch frames, the largest chunk a kde::KinectDepthEnhancementFeed on this object may use
    KinectDepthEnhancement(int width, int height, int max_batch) : Width(width), Height(height)
    {
        check(kde_enh_create(&h_, width, height, max_batch));
    }
    ~KinectDepthEnhancement() { kde_enh_destroy(h_); }
    KinectDepthEnhancement(const KinectDepthEnhancement&) = delete;
    KinectDepthEnhancement& operator=(const KinectDepthEnhancement&) = delete;

    template <class MatLike>
    void SetParametor(int rows, int cols, const MatLike& intrinsic)   // [sic], .cpp:46-55
    {
        double k[9];
        intrinsic_to_array(intrinsic, k);
        check(kde_enh_set_parameters(h_, rows, cols, k));
    }
    template <class GpuMatLike>
    void Process(float* depth_device, const GpuMatLike& color_device)   // .cpp:56-81
    {
        require_continuous_8uc3(color_device, Width, Height, "KinectDepthEnhancement::Process");
        check(kde_enh_process_batch(h_, 1, depth_device, color_device.data, stream_));
    }
    // added: n independent frames back to back (kde_enh_process_batch), n at most the max_batch of the constructor
    void ProcessBatch(int n, const float* depth_device, const uint8_t* bgr_device)
    {
        check(kde_enh_process_batch(h_, n, depth_device, bgr_device, stream_));
    }
    float3* getOptimizedPoints_Device()
    {
        kde_float3* p = nullptr;
        check(kde_enh_optimized_points_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    float3* getOptimizedPoints_Host()
    {
        const kde_float3* p = nullptr;
        check(kde_enh_optimized_points_host(h_, stream_, &p));
        return reinterpret_cast<float3*>(const_cast<kde_float3*>(p));
    }
    // added: the intermediate results a caller of the reference would read off the private members
    int* getLabelDevice() const
    {
        int32_t* p = nullptr;
        check(kde_enh_nasp_labels_device(h_, &p));
        return p;
    }
    int* getMergedClusterLabel_Device() const
    {
        int32_t* p = nullptr;
        check(kde_enh_merged_labels_device(h_, &p));
        return p;
    }
    float3* getEdgeEnhanced3DPoints_Device() const
    {
        kde_float3* p = nullptr;
        check(kde_enh_edge_enhanced_points_device(h_, &p));
        return reinterpret_cast<float3*>(p);
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_enh* handle() const { return h_; }

private:
    int Width, Height;
    kde_enh* h_ = nullptr;
    void* stream_ = nullptr;
};

}  // namespace ref

// ------------------------------------------------------------------------------------------------
// extension (no reference counterpart): JointBilateralFilter::Process on frames in host memory, the upload of main.cpp:160-163
// and the uint16 widening of Buffer2D.cpp:18-32 included (kde_jbf_feed_*).  Borrows the filter: it must outlive this object
// and must not be used while process() runs; its getters keep returning what its own Process wrote.  process() blocks.
class JointBilateralFilterFeed {
public:
    explicit JointBilateralFilterFeed(ref::JointBilateralFilter& jbf, int chunk_frames = 8) : JointBilateralFilterFeed(jbf.handle(), chunk_frames) {}
    JointBilateralFilterFeed(kde_jbf* jbf, int chunk_frames) { check(kde_jbf_feed_create(&f_, jbf, chunk_frames)); }
    ~JointBilateralFilterFeed() { kde_jbf_feed_destroy(f_); }
    JointBilateralFilterFeed(const JointBilateralFilterFeed&) = delete;
    JointBilateralFilterFeed& operator=(const JointBilateralFilterFeed&) = delete;

    // n frames back to back: depth in mm (float, or the sensor's uint16 with 0 = invalid), packed BGR, filtered depth out
    void process(int n, const float* depth_host, const uint8_t* bgr_host, float* filtered_host)
    {
        check(kde_jbf_feed_process(f_, n, depth_host, KDE_DEPTH_F32, bgr_host, filtered_host));
    }
    void process(int n, const uint16_t* depth_host, const uint8_t* bgr_host, float* filtered_host)
    {
        check(kde_jbf_feed_process(f_, n, depth_host, KDE_DEPTH_U16, bgr_host, filtered_host));
    }
    kde_feed_stats lastStats() const
    {
        kde_feed_stats st{};
        check(kde_jbf_feed_last_stats(f_, &st));
        return st;
    }
    kde_jbf_feed* handle() const { return f_; }

private:
    kde_jbf_feed* f_ = nullptr;
};

// extension (no reference counterpart): the z of n_points packed points as a depth map on the device (kde_points_to_depth),
// float with the bits unchanged or the sensor's uint16 millimetres (rounded half to even, 0 = invalid); asynchronous on stream
inline void pointsToDepth(size_t n_points, const float3* points_device, float* depth_device, void* hip_stream = nullptr)
{
    check(kde_points_to_depth(n_points, reinterpret_cast<const kde_float3*>(points_device), KDE_DEPTH_F32, depth_device, hip_stream));
}
inline void pointsToDepth(size_t n_points, const float3* points_device, uint16_t* depth_device, void* hip_stream = nullptr)
{
    check(kde_points_to_depth(n_points, reinterpret_cast<const kde_float3*>(points_device), KDE_DEPTH_U16, depth_device, hip_stream));
}

// extension (no reference counterpart): KinectDepthEnhancement::Process on frames in host memory (kde_enh_feed_*), the upload of
// main.cpp:160-163 and the uint16 widening included; the result comes back as the optimized cloud (float3), its depth map
// (float) or that in the sensor's format (uint16_t), chosen by the type of the output pointer.  Borrows the object and runs
// it: it must outlive this feed, must have had SetParametor called and must not be used while process() runs; its getters
// then show the last chunk.  chunk_frames is at most the object's max_batch.  process() blocks.
class KinectDepthEnhancementFeed {
public:
    KinectDepthEnhancementFeed(ref::KinectDepthEnhancement& enh, int chunk_frames) : KinectDepthEnhancementFeed(enh.handle(), chunk_frames) {}
    KinectDepthEnhancementFeed(kde_enh* enh, int chunk_frames) { check(kde_enh_feed_create(&f_, enh, chunk_frames)); }
    ~KinectDepthEnhancementFeed() { kde_enh_feed_destroy(f_); }
    KinectDepthEnhancementFeed(const KinectDepthEnhancementFeed&) = delete;
    KinectDepthEnhancementFeed& operator=(const KinectDepthEnhancementFeed&) = delete;

    // n frames back to back: depth in mm (float, or the sensor's uint16 with 0 = invalid), packed BGR
    template <class Depth, class Out>
    void process(int n, const Depth* depth_host, const uint8_t* bgr_host, Out* out_host)
    {
        check(kde_enh_feed_process(f_, n, depth_host, depth_format(depth_host), bgr_host, out_format(out_host), out_host));
    }
    kde_feed_stats lastStats() const
    {
        kde_feed_stats st{};
        check(kde_enh_feed_last_stats(f_, &st));
        return st;
    }
    kde_enh_feed* handle() const { return f_; }

private:
    static int depth_format(const float*) { return KDE_DEPTH_F32; }
    static int depth_format(const uint16_t*) { return KDE_DEPTH_U16; }
    static int out_format(const float3*) { return KDE_OUT_POINTS_F32; }
    static int out_format(const kde_float3*) { return KDE_OUT_POINTS_F32; }
    static int out_format(const float*) { return KDE_OUT_DEPTH_F32; }
    static int out_format(const uint16_t*) { return KDE_OUT_DEPTH_U16; }
    kde_enh_feed* f_ = nullptr;
};

// extension (no reference counterpart as a class): the mean 3-D error of main.cpp:220-308 for n frames and up to eight candidate
// results against one ground truth, computed on the device (kde_error3d_*).  A source is a cloud (float3*) or a depth map
// (float* / uint16_t*, projected with the camera of setCamera as projectiveToReal(float*) would); compare() is asynchronous
// on the object's stream and capturable; results_Host() synchronises.  The table is [n][m] records of (sum, count, mean).
class MeanError3D {
public:
    MeanError3D(int width, int height, int max_batch = 1, int max_candidates = 8)
    {
        check(kde_error3d_create(&h_, width, height, max_batch, max_candidates));
    }
    ~MeanError3D() { kde_error3d_destroy(h_); }
    MeanError3D(const MeanError3D&) = delete;
    MeanError3D& operator=(const MeanError3D&) = delete;

    static kde_error3d_source source(const float3* points_device) { return {points_device, KDE_SRC_POINTS_F32}; }
    static kde_error3d_source source(const kde_float3* points_device) { return {points_device, KDE_SRC_POINTS_F32}; }
    static kde_error3d_source source(const float* depth_device) { return {depth_device, KDE_SRC_DEPTH_F32}; }
    static kde_error3d_source source(const uint16_t* depth_device) { return {depth_device, KDE_SRC_DEPTH_U16}; }

    template <class MatLike>
    void setCamera(const MatLike& intrinsic)
    {
        double k[9];
        intrinsic_to_array(intrinsic, k);
        check(kde_error3d_set_camera(h_, k));
    }
    void setRange(float z_min, float z_max) { check(kde_error3d_set_range(h_, z_min, z_max)); }
    // n frames, m candidates (a host array of m descriptors) against truth; truth_frames = 1 (one truth for every frame) or n
    void compare(int n, int m, const kde_error3d_source* candidates, const kde_error3d_source& truth, int truth_frames = 1)
    {
        check(kde_error3d_compare_batch(h_, n, m, candidates, &truth, truth_frames, stream_));
    }
    kde_error3d_result* results_Device() const
    {
        kde_error3d_result* p = nullptr;
        check(kde_error3d_results_device(h_, &p));
        return p;
    }
    const kde_error3d_result* results_Host() const
    {
        const kde_error3d_result* p = nullptr;
        check(kde_error3d_results_host(h_, stream_, &p));
        return p;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_error3d* handle() const { return h_; }

private:
    kde_error3d* h_ = nullptr;
    void* stream_ = nullptr;
};

// extension (no reference counterpart as a class): the output step of main.cpp:211-300 for n frames of one method, on the
// device (kde_cloud_*): the organised float3 grid and the colour image become 16-byte XYZRGB records (PCL's PointXYZRGB
// payload: x, y, z in metres with z negated, rgb packed), the valid ones (50 < z < 15000) compacted in raster order at the
// start of each frame's slot of W * H records -- or, with params.organized, every pixel with NaNs where it is invalid.
// A source is what MeanError3D::source describes.  build() is asynchronous on the object's stream and capturable; the *_Host
// members synchronise.  include/kde/pcd_io.hpp writes the records as a PCD file.
class PointCloudXYZRGB {
public:
    static kde_cloud_params defaultParams()
    {
        kde_cloud_params p{};
        check(kde_cloud_default_params(&p));
        return p;
    }
    PointCloudXYZRGB(int width, int height, int max_batch = 1) { check(kde_cloud_create(&h_, width, height, max_batch, nullptr)); }
    PointCloudXYZRGB(int width, int height, int max_batch, const kde_cloud_params& params)
    {
        check(kde_cloud_create(&h_, width, height, max_batch, &params));
    }
    ~PointCloudXYZRGB() { kde_cloud_destroy(h_); }
    PointCloudXYZRGB(const PointCloudXYZRGB&) = delete;
    PointCloudXYZRGB& operator=(const PointCloudXYZRGB&) = delete;

    template <class MatLike>
    void setCamera(const MatLike& intrinsic)
    {
        double k[9];
        intrinsic_to_array(intrinsic, k);
        check(kde_cloud_set_camera(h_, k));
    }
    // n frames of `source` with bgr_frames = 1 (one image for every frame) or n packed BGR images; out_device == nullptr: the
    // object-owned buffer
    void build(int n, const kde_error3d_source& source, const uint8_t* bgr_device, int bgr_frames = 1,
               kde_cloud_point* out_device = nullptr)
    {
        check(kde_cloud_build_batch(h_, n, &source, bgr_device, bgr_frames, out_device, stream_));
    }
    kde_cloud_point* points_Device() const
    {
        kde_cloud_point* p = nullptr;
        check(kde_cloud_points_device(h_, &p));
        return p;
    }
    uint32_t* counts_Device() const
    {
        uint32_t* p = nullptr;
        check(kde_cloud_counts_device(h_, &p));
        return p;
    }
    const uint32_t* counts_Host() const
    {
        const uint32_t* p = nullptr;
        check(kde_cloud_counts_host(h_, stream_, &p));
        return p;
    }
    // the frames packed tightly: frame f is the records offsets[f] .. offsets[f + 1] - 1
    const kde_cloud_point* points_Host(const uint64_t** offsets) const
    {
        const kde_cloud_point* p = nullptr;
        check(kde_cloud_points_host(h_, stream_, &p, offsets));
        return p;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_cloud* handle() const { return h_; }

private:
    kde_cloud* h_ = nullptr;
    void* stream_ = nullptr;
};

// extension (no reference counterpart as a class): the surface of main.cpp:211-300 as a triangle mesh of the organised grid,
// for n frames of one method on the device (kde_mesh_*).  The vertices are exactly PointCloudXYZRGB's dense cloud, the vertex
// index of a valid pixel its rank in raster order; a pixel quad gives 0, 1 or 2 triangles (kde_mesh_triangle, three indices),
// a triangle iff its corners are valid and its edges linked, |za - zb| <= max_diff + rel_diff * min(za, zb).  Triangles are
// ordered by owning pixel; frame f's are the first tri_counts[f] records of its slot of 2 (W - 1) (H - 1).  build() is
// asynchronous on the object's stream and capturable; the *_Host members synchronise.  include/kde/ply_io.hpp writes the
// mesh as a PLY file.
class OrganizedMesh {
public:
    static kde_mesh_params defaultParams()
    {
        kde_mesh_params p{};
        check(kde_mesh_default_params(&p));
        return p;
    }
    OrganizedMesh(int width, int height, int max_batch = 1) { check(kde_mesh_create(&h_, width, height, max_batch, nullptr)); }
    OrganizedMesh(int width, int height, int max_batch, const kde_mesh_params& params)
    {
        check(kde_mesh_create(&h_, width, height, max_batch, &params));
    }
    ~OrganizedMesh() { kde_mesh_destroy(h_); }
    OrganizedMesh(const OrganizedMesh&) = delete;
    OrganizedMesh& operator=(const OrganizedMesh&) = delete;

    template <class MatLike>
    void setCamera(const MatLike& intrinsic)
    {
        double k[9];
        intrinsic_to_array(intrinsic, k);
        check(kde_mesh_set_camera(h_, k));
    }
    // n frames of `source` with bgr_frames = 1 (one image for every frame) or n packed BGR images; an output that is nullptr
    // is the object-owned buffer
    void build(int n, const kde_error3d_source& source, const uint8_t* bgr_device, int bgr_frames = 1,
               kde_cloud_point* vertices_device = nullptr, kde_mesh_triangle* triangles_device = nullptr)
    {
        check(kde_mesh_build_batch(h_, n, &source, bgr_device, bgr_frames, vertices_device, triangles_device, stream_));
    }
    kde_cloud_point* vertices_Device() const
    {
        kde_cloud_point* p = nullptr;
        check(kde_mesh_vertices_device(h_, &p));
        return p;
    }
    kde_mesh_triangle* triangles_Device() const
    {
        kde_mesh_triangle* p = nullptr;
        check(kde_mesh_triangles_device(h_, &p));
        return p;
    }
    uint32_t* counts_Device() const
    {
        uint32_t* p = nullptr;
        check(kde_mesh_counts_device(h_, &p));
        return p;
    }
    uint32_t* triCounts_Device() const
    {
        uint32_t* p = nullptr;
        check(kde_mesh_tri_counts_device(h_, &p));
        return p;
    }
    const uint32_t* counts_Host() const
    {
        const uint32_t* p = nullptr;
        check(kde_mesh_counts_host(h_, stream_, &p));
        return p;
    }
    const uint32_t* triCounts_Host() const
    {
        const uint32_t* p = nullptr;
        check(kde_mesh_tri_counts_host(h_, stream_, &p));
        return p;
    }
    // the frames packed tightly: frame f is the records offsets[f] .. offsets[f + 1] - 1
    const kde_cloud_point* vertices_Host(const uint64_t** offsets) const
    {
        const kde_cloud_point* p = nullptr;
        check(kde_mesh_vertices_host(h_, stream_, &p, offsets));
        return p;
    }
    const kde_mesh_triangle* triangles_Host(const uint64_t** offsets) const
    {
        const kde_mesh_triangle* p = nullptr;
        check(kde_mesh_triangles_host(h_, stream_, &p, offsets));
        return p;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    kde_mesh* handle() const { return h_; }

private:
    kde_mesh* h_ = nullptr;
    void* stream_ = nullptr;
};

namespace detail {
// What the depth-in / depth-out stage classes below share (csrc/kde_depth_stage.h is the same core in the library): the handle
// and its stream, the results of the last batch call on the device and in pinned memory, and the format of a depth pointer.
// A stage derives from it with its handle, its parameter struct and its six C functions, and adds its constructors, its
// calibration, its batch call and whatever only it has.
template <class Handle, class Params, auto DefaultParams, auto Destroy, auto DepthDevice, auto DepthHost, auto FilledDevice, auto FilledHost>
class DepthStage {
public:
    static Params defaultParams()
    {
        Params p{};
        check(DefaultParams(&p));
        return p;
    }
    DepthStage(const DepthStage&) = delete;
    DepthStage& operator=(const DepthStage&) = delete;

    // the frames of the last batch call: out_device of that call or the object-owned buffer, float or uint16 as that call asked
    void* depth_Device() const
    {
        void* p = nullptr;
        check(DepthDevice(h_, &p));
        return p;
    }
    const void* depth_Host() const
    {
        const void* p = nullptr;
        check(DepthHost(h_, stream_, &p));
        return p;
    }
    // the pixels that got a depth, per frame of the last batch call
    uint32_t* filled_Device() const
    {
        uint32_t* p = nullptr;
        check(FilledDevice(h_, &p));
        return p;
    }
    const uint32_t* filled_Host() const
    {
        const uint32_t* p = nullptr;
        check(FilledHost(h_, stream_, &p));
        return p;
    }
    void setStream(void* hip_stream) { stream_ = hip_stream; }
    Handle* handle() const { return h_; }

protected:
    DepthStage() = default;
    ~DepthStage() { Destroy(h_); }
    static int format(const float*) { return KDE_DEPTH_F32; }
    static int format(const uint16_t*) { return KDE_DEPTH_U16; }
    Handle* h_ = nullptr;       // the stage's constructor creates it
    void* stream_ = nullptr;
};
}  // namespace detail

// extension (no reference counterpart as a class): the registration Kinect::InitAllData asks OpenNI for (Kinect.cpp:71-75),
// on the device (kde_reg_*): n depth frames (float* or uint16_t*) warped into the colour camera's view through a z-buffer, so
// that depth pixel (x, y) and colour pixel (x, y) look along the same ray, as every class above assumes.  The rule is stated
// in kde_hip.h: the nearest source pixel wins, the result is deterministic to the bit; cx and cy are kept as floats; no lens
// distortion.  registerDepth() is asynchronous on the object's stream and capturable; the *_Host members synchronise.
class DepthRegistration
    : public detail::DepthStage<kde_reg, kde_reg_params, kde_reg_default_params, kde_reg_destroy, kde_reg_depth_device,
                                kde_reg_depth_host, kde_reg_filled_device, kde_reg_filled_host> {
public:
    DepthRegistration(int depth_width, int depth_height, int color_width, int color_height, int max_batch = 1)
    {
        check(kde_reg_create(&h_, depth_width, depth_height, color_width, color_height, max_batch, nullptr));
    }
    DepthRegistration(int depth_width, int depth_height, int color_width, int color_height, int max_batch, const kde_reg_params& params)
    {
        check(kde_reg_create(&h_, depth_width, depth_height, color_width, color_height, max_batch, &params));
    }

    // the two intrinsic matrices, R (row-major 3 x 3) and t (millimetres): P_colour = R * P_depth + t
    template <class MatLike>
    void setCalibration(const MatLike& depth_intrinsic, const MatLike& color_intrinsic, const double* R9, const double* t3)
    {
        double kd[9], kc[9];
        intrinsic_to_array(depth_intrinsic, kd);
        intrinsic_to_array(color_intrinsic, kc);
        check(kde_reg_set_calibration(h_, kd, kc, R9, t3));
    }
    // n frames back to back; the output format is the type of out_device (nullptr of that type: the object-owned buffer)
    template <class Depth, class Out>
    void registerDepth(int n, const Depth* depth_device, Out* out_device)
    {
        check(kde_reg_register_batch(h_, n, depth_device, format(depth_device), format(out_device), out_device, stream_));
    }
    // the colour image as the depth camera sees it (no occlusion test): bgr_frames = 1 (one image for every frame) or n
    template <class Depth>
    void colorToDepth(int n, const Depth* depth_device, const uint8_t* bgr_device, int bgr_frames, uint8_t* out_bgr_device)
    {
        check(kde_reg_color_to_depth_batch(h_, n, depth_device, format(depth_device), bgr_device, bgr_frames, out_bgr_device, stream_));
    }
};

// extension (no reference counterpart): frames of a camera with lens distortion -- OpenCV's rational model k1, k2, p1, p2, k3,
// k4, k5, k6, of which Brown-Conrady is k4 = k5 = k6 = 0 -- resampled into a pinhole view on the device (kde_undist_*), so that
// sensors calibrated with OpenCV can feed every class above, DepthRegistration first.  The rule is stated in kde_hip.h: colour
// is bilinear with (0, 0, 0) outside the source; depth takes the nearest valid sample or, with depth_interp 1, the bilinear
// value where the four taps are valid and within max_gap of each other; deterministic to the bit; no rectifying rotation.
// undistortColor() and undistortDepth() are asynchronous on the object's stream and capturable; the *_Host members synchronise.
class LensUndistortion
    : public detail::DepthStage<kde_undist, kde_undist_params, kde_undist_default_params, kde_undist_destroy, kde_undist_depth_device,
                                kde_undist_depth_host, kde_undist_filled_device, kde_undist_filled_host> {
public:
    LensUndistortion(int src_width, int src_height, int out_width, int out_height, int max_batch = 1)
    {
        check(kde_undist_create(&h_, src_width, src_height, out_width, out_height, max_batch, nullptr));
    }
    LensUndistortion(int src_width, int src_height, int out_width, int out_height, int max_batch, const kde_undist_params& params)
    {
        check(kde_undist_create(&h_, src_width, src_height, out_width, out_height, max_batch, &params));
    }

    // the distorted camera's intrinsic matrix and dist8 = k1, k2, p1, p2, k3, k4, k5, k6; the pinhole view keeps the matrix
    template <class MatLike>
    void setCalibration(const MatLike& intrinsic, const double* dist8)
    {
        double k[9];
        intrinsic_to_array(intrinsic, k);
        check(kde_undist_set_calibration(h_, k, dist8, nullptr));
    }
    // the same with a camera matrix of its own for the pinhole view (OpenCV's getOptimalNewCameraMatrix, another size, ...)
    template <class MatLike>
    void setCalibration(const MatLike& intrinsic, const double* dist8, const MatLike& new_intrinsic)
    {
        double k[9], kn[9];
        intrinsic_to_array(intrinsic, k);
        intrinsic_to_array(new_intrinsic, kn);
        check(kde_undist_set_calibration(h_, k, dist8, kn));
    }
    // n frames back to back; bgr_frames = 1 (one image for every frame) or n
    void undistortColor(int n, const uint8_t* bgr_device, int bgr_frames, uint8_t* out_bgr_device)
    {
        check(kde_undist_color_batch(h_, n, bgr_device, bgr_frames, out_bgr_device, stream_));
    }
    // n frames back to back; the output format is the type of out_device (nullptr of that type: the object-owned buffer)
    template <class Depth, class Out>
    void undistortDepth(int n, const Depth* depth_device, Out* out_device)
    {
        check(kde_undist_depth_batch(h_, n, depth_device, format(depth_device), format(out_device), out_device, stream_));
    }
    // [out_height][out_width] of (us, vs): OpenCV's initUndistortRectifyMap product, computed at the first request
    const float* map_Device() const
    {
        const float* p = nullptr;
        check(kde_undist_map_device(h_, stream_, &p));
        return p;
    }
};

// extension (no reference counterpart): a low-resolution depth frame brought to the size of its colour image on the device
// (kde_upsample_*) by joint bilateral upsampling -- low-resolution samples weighted by a tent of `radius` samples around the
// output pixel and by the resemblance of the guide colour at the output pixel to the guide colour at the sample -- so that
// sensors whose depth is smaller than their colour can feed every class above.  The rule is stated in kde_hip.h; with max_gap
// > 0 no depth is blended across more than max_gap millimetres; deterministic to the bit.  upsample() is asynchronous on the
// object's stream and capturable; the *_Host members synchronise.
class GuidedDepthUpsampling
    : public detail::DepthStage<kde_upsample, kde_upsample_params, kde_upsample_default_params, kde_upsample_destroy, kde_upsample_depth_device,
                                kde_upsample_depth_host, kde_upsample_filled_device, kde_upsample_filled_host> {
public:
    GuidedDepthUpsampling(int src_width, int src_height, int out_width, int out_height, int max_batch = 1)
    {
        check(kde_upsample_create(&h_, src_width, src_height, out_width, out_height, max_batch, nullptr));
    }
    GuidedDepthUpsampling(int src_width, int src_height, int out_width, int out_height, int max_batch, const kde_upsample_params& params)
    {
        check(kde_upsample_create(&h_, src_width, src_height, out_width, out_height, max_batch, &params));
    }

    // n depth frames back to back, the guide bgr_frames = 1 (one image for every frame) or n images of the output size; the
    // output format is the type of out_device (nullptr of that type: the object-owned buffer)
    template <class Depth, class Out>
    void upsample(int n, const Depth* depth_device, const uint8_t* bgr_device, int bgr_frames, Out* out_device)
    {
        check(kde_upsample_depth_batch(h_, n, depth_device, format(depth_device), bgr_device, bgr_frames, format(out_device), out_device,
                                       stream_));
    }
    // range[k] for k = |db| + |dg| + |dr| = 0 .. 765, as the kernel reads it
    void rangeTable(float (&table_host)[766]) const { check(kde_upsample_range_table(h_, table_host, 766)); }
};

// extension (no reference counterpart): the holes of a depth frame filled on the device under the guide of its colour image
// (kde_holefill_*) -- `iterations` passes, each of which gives the hole pixels with at least `min_taps` usable neighbours within
// `radius` the mean of those neighbours, weighted by distance and by the resemblance of the guide colour -- behind the
// registration, the undistortion and the upsampling, which leave holes, and in front of the filters, which reach two or three
// pixels into one.  iterations * radius bounds how far a fill reaches.  The rule is stated in kde_hip.h; with max_gap > 0 no
// depth is blended across more than max_gap millimetres; deterministic to the bit.  fill() is asynchronous on the object's
// stream and capturable; the *_Host members synchronise.
class DepthHoleFilling
    : public detail::DepthStage<kde_holefill, kde_holefill_params, kde_holefill_default_params, kde_holefill_destroy, kde_holefill_depth_device,
                                kde_holefill_depth_host, kde_holefill_filled_device, kde_holefill_filled_host> {
public:
    DepthHoleFilling(int width, int height, int max_batch = 1) { check(kde_holefill_create(&h_, width, height, max_batch, nullptr)); }
    DepthHoleFilling(int width, int height, int max_batch, const kde_holefill_params& params)
    {
        check(kde_holefill_create(&h_, width, height, max_batch, &params));
    }

    // n depth frames back to back, the guide bgr_frames = 1 (one image for every frame) or n images; the output format is the
    // type of out_device (nullptr of that type: the object-owned buffer), which must not overlap depth_device; pass_of_device:
    // n frames of uint8 (0 original, p filled in pass p, 255 still a hole) or nullptr where it is not wanted
    template <class Depth, class Out>
    void fill(int n, const Depth* depth_device, const uint8_t* bgr_device, int bgr_frames, Out* out_device, uint8_t* pass_of_device = nullptr)
    {
        check(kde_holefill_fill_batch(h_, n, depth_device, format(depth_device), bgr_device, bgr_frames, format(out_device), out_device,
                                      pass_of_device, stream_));
    }
    uint32_t* remaining_Device() const
    {
        uint32_t* p = nullptr;
        check(kde_holefill_remaining_device(h_, &p));
        return p;
    }
    const uint32_t* remaining_Host() const
    {
        const uint32_t* p = nullptr;
        check(kde_holefill_remaining_host(h_, stream_, &p));
        return p;
    }
    // the number of passes one launch performs
    int passesPerLaunch() const
    {
        int k = 0;
        check(kde_holefill_passes_per_launch(h_, &k));
        return k;
    }
    // space[(2 radius + 1)^2] (capacity: the entries table_host holds) and range[k] for k = |db| + |dg| + |dr| = 0 .. 765
    void spaceTable(float* table_host, int capacity) const { check(kde_holefill_space_table(h_, table_host, capacity)); }
    void rangeTable(float (&table_host)[766]) const { check(kde_holefill_range_table(h_, table_host, 766)); }
};

// extension (no reference counterpart): wrong depth taken away on the device (kde_speckle_*) -- the connected components of a
// frame under a depth-difference link (within max_diff + rel_diff * the nearer depth, 4- or 8-connected), those smaller than
// min_size set to 0: flying pixels, speckles, background showing through a registered foreground.  Behind the registration,
// the undistortion and the upsampling and in front of DepthHoleFilling: invalidate first, then fill.  The rule is stated in
// kde_hip.h; deterministic to the bit.  filter() is asynchronous on the object's stream and capturable; the *_Host members
// synchronise.  The count of the shared core is removed[f] here: removed_Device() / removed_Host().
class DepthSpeckleFilter
    : public detail::DepthStage<kde_speckle, kde_speckle_params, kde_speckle_default_params, kde_speckle_destroy, kde_speckle_depth_device,
                                kde_speckle_depth_host, kde_speckle_removed_device, kde_speckle_removed_host> {
public:
    DepthSpeckleFilter(int width, int height, int max_batch = 1) { check(kde_speckle_create(&h_, width, height, max_batch, nullptr)); }
    DepthSpeckleFilter(int width, int height, int max_batch, const kde_speckle_params& params)
    {
        check(kde_speckle_create(&h_, width, height, max_batch, &params));
    }

    // n depth frames back to back; the output format is the type of out_device (nullptr of that type: the object-owned buffer);
    // out_device may be depth_device itself (in place) and must not overlap it otherwise; labels_device: n frames of int32 (the
    // smallest raster index of a kept pixel's component, -1 where the output is 0) or nullptr where it is not wanted
    template <class Depth, class Out>
    void filter(int n, const Depth* depth_device, Out* out_device, int32_t* labels_device = nullptr)
    {
        check(kde_speckle_filter_batch(h_, n, depth_device, format(depth_device), format(out_device), out_device, labels_device, stream_));
    }
    // the pixels with a depth that the last filter() set to 0, per frame
    uint32_t* removed_Device() const { return filled_Device(); }
    const uint32_t* removed_Host() const { return filled_Host(); }
    // the components the last filter() kept, per frame
    uint32_t* components_Device() const
    {
        uint32_t* p = nullptr;
        check(kde_speckle_components_device(h_, &p));
        return p;
    }
    const uint32_t* components_Host() const
    {
        const uint32_t* p = nullptr;
        check(kde_speckle_components_host(h_, stream_, &p));
        return p;
    }
    // 0; anything else is a defect of the library and the frame is not to be trusted
    const uint32_t* capped_Host() const
    {
        const uint32_t* p = nullptr;
        check(kde_speckle_capped_host(h_, stream_, &p));
        return p;
    }
    uint32_t* capped_Device() const
    {
        uint32_t* p = nullptr;
        check(kde_speckle_capped_device(h_, &p));
        return p;
    }

private:
    using DepthStage::filled_Device;        // this stage fills nothing: the names above say what the count is
    using DepthStage::filled_Host;
};

// extension (no reference counterpart; Buffer2D's sequence average folds n frames into one and has no notion of motion):
// motion-aware smoothing of a depth sequence on the device (kde_temporal_*).  Each sample is blended into a per-pixel running
// value while it stays on the same surface (DepthSpeckleFilter's link), starts the value again where it jumps, the value is
// held over short dropouts and forgotten where the colour guide says the scene changed.  The frames of a call are consecutive
// in time and the object carries the state from one call to the next; reset() starts a new sequence.  Beside
// DepthSpeckleFilter and in front of DepthHoleFilling.  The rule is stated in kde_hip.h; deterministic to the bit, however the
// sequence is cut into calls.  filter() and reset() are asynchronous on the object's stream and capturable (a replay advances
// the stream by n frames); the *_Host members synchronise.  The count of the shared core is smoothed[f] here.
class DepthTemporalFilter
    : public detail::DepthStage<kde_temporal, kde_temporal_params, kde_temporal_default_params, kde_temporal_destroy, kde_temporal_depth_device,
                                kde_temporal_depth_host, kde_temporal_smoothed_device, kde_temporal_smoothed_host> {
public:
    DepthTemporalFilter(int width, int height, int max_batch = 1) { check(kde_temporal_create(&h_, width, height, max_batch, nullptr)); }
    DepthTemporalFilter(int width, int height, int max_batch, const kde_temporal_params& params)
    {
        check(kde_temporal_create(&h_, width, height, max_batch, &params));
    }

    // the next n frames of the sequence, back to back; bgr_device: n frames of guide or nullptr; the output format is the type
    // of out_device (nullptr of that type: the object-owned buffer); out_device may be depth_device itself (in place) and must
    // not overlap it otherwise, nor the guide
    template <class Depth, class Out>
    void filter(int n, const Depth* depth_device, const uint8_t* bgr_device, Out* out_device)
    {
        check(kde_temporal_filter_batch(h_, n, depth_device, format(depth_device), bgr_device, format(out_device), out_device, stream_));
    }
    // the state of every pixel becomes empty, as after construction
    void reset() { check(kde_temporal_reset(h_, stream_)); }
    // the object-owned state: value[height][width], hist[height][width] (kde_hip.h); copy it out to checkpoint a stream, copy
    // into it between calls to restore one or to move it to another object
    void state_Device(float*& value, uint32_t*& hist) const { check(kde_temporal_state_device(h_, &value, &hist)); }
    // the pixels per frame of the last filter() whose sample was blended into the running value
    uint32_t* smoothed_Device() const { return filled_Device(); }
    const uint32_t* smoothed_Host() const { return filled_Host(); }
    // ... whose valid sample left the surface of the running value
    uint32_t* jumped_Device() const { return count(kde_temporal_jumped_device); }
    const uint32_t* jumped_Host() const { return count(kde_temporal_jumped_host); }
    // ... the holes that kept the running value
    uint32_t* held_Device() const { return count(kde_temporal_held_device); }
    const uint32_t* held_Host() const { return count(kde_temporal_held_host); }
    // ... whose running value the guide's colour change forgot
    uint32_t* changed_Device() const { return count(kde_temporal_changed_device); }
    const uint32_t* changed_Host() const { return count(kde_temporal_changed_host); }

private:
    using DepthStage::filled_Device;        // this stage fills nothing: the names above say what the count is
    using DepthStage::filled_Host;
    uint32_t* count(int (*get)(kde_temporal*, uint32_t**)) const
    {
        uint32_t* p = nullptr;
        check(get(h_, &p));
        return p;
    }
    const uint32_t* count(int (*get)(kde_temporal*, void*, const uint32_t**)) const
    {
        const uint32_t* p = nullptr;
        check(get(h_, stream_, &p));
        return p;
    }
};

// extension (no reference counterpart: every class of the reference runs at the size of the frame it is given): depth frames
// and their colour guides made `factor` times smaller each way on the device (kde_decimate_*).  An output pixel is the lower
// median (KDE_DECIMATE_MEDIAN) or the guarded mean (KDE_DECIMATE_MEAN) of the valid samples of its factor x factor block, 0
// where fewer than min_valid are valid; the guide is the block's mean colour rounded half up.  The step down of a
// multi-resolution chain: decimate, enhance at the small size, GuidedDepthUpsampling back under the full-resolution guide.
// The rule is stated in kde_hip.h; deterministic to the bit.  decimate() and decimateColor() are asynchronous on the object's
// stream and capturable; the *_Host members synchronise.
class DepthDecimation
    : public detail::DepthStage<kde_decimate, kde_decimate_params, kde_decimate_default_params, kde_decimate_destroy, kde_decimate_depth_device,
                                kde_decimate_depth_host, kde_decimate_filled_device, kde_decimate_filled_host> {
public:
    DepthDecimation(int src_width, int src_height, int max_batch = 1) { check(kde_decimate_create(&h_, src_width, src_height, max_batch, nullptr)); }
    DepthDecimation(int src_width, int src_height, int max_batch, const kde_decimate_params& params)
    {
        check(kde_decimate_create(&h_, src_width, src_height, max_batch, &params));
    }

    // ceil(src / factor) each way
    int outWidth() const
    {
        int w = 0, h = 0;
        check(kde_decimate_out_size(h_, &w, &h));
        return w;
    }
    int outHeight() const
    {
        int w = 0, h = 0;
        check(kde_decimate_out_size(h_, &w, &h));
        return h;
    }
    // n frames back to back; the output format is the type of out_device (nullptr of that type: the object-owned buffer),
    // which must not overlap depth_device
    template <class Depth, class Out>
    void decimate(int n, const Depth* depth_device, Out* out_device)
    {
        check(kde_decimate_depth_batch(h_, n, depth_device, format(depth_device), format(out_device), out_device, stream_));
    }
    // the guides of n frames, [n][src_height][src_width][3] to [n][outHeight()][outWidth()][3]
    void decimateColor(int n, const uint8_t* bgr_device, uint8_t* out_bgr_device)
    {
        check(kde_decimate_color_batch(h_, n, bgr_device, out_bgr_device, stream_));
    }
    // the camera matrix of the small image: fx / k, fy / k, (cx + 0.5) / k - 0.5, (cy + 0.5) / k - 0.5; needs no device
    template <class MatLike>
    void intrinsics(const MatLike& intrinsic, double (&small_intrinsic)[9]) const
    {
        double k[9];
        intrinsic_to_array(intrinsic, k);
        check(kde_decimate_intrinsics(h_, k, small_intrinsic));
    }
    // the output pixels per frame of the last decimate() whose block spans more than max_gap (0 without a guard)
    uint32_t* mixed_Device() const
    {
        uint32_t* p = nullptr;
        check(kde_decimate_mixed_device(h_, &p));
        return p;
    }
    const uint32_t* mixed_Host() const
    {
        const uint32_t* p = nullptr;
        check(kde_decimate_mixed_host(h_, stream_, &p));
        return p;
    }
};

}  // namespace kde

#ifndef KDE_NO_GLOBAL_NAMES
using kde::ref::ArrayBuffer;
using kde::ref::Buffer2D;
using kde::ref::DepthAdaptiveSuperpixel;
using kde::ref::DimensionConvertor;
using kde::ref::EdgeRefinedSuperpixel;
using kde::ref::JointBilateralFilter;
using kde::ref::KinectDepthEnhancement;
using kde::ref::LabelEquivalenceSeg;
using kde::ref::MarkovRandomField;
using kde::ref::NormalAdaptiveSuperpixel;
using kde::ref::NormalMapGenerator;
using kde::ref::Projection_GPU;
using kde::ref::RegionGrowingBilateralFilter;
using kde::ref::SPDepthSuperResolution;
#endif

#endif  // KDE_KDE_HPP
