// SIFT / RootSIFT keypoints and descriptors on the GPU (sift.hip) -- the detector stage of the
// orthophoto / master-frame registration (reference: geotrax/utils/registration.py:59-85,
// detector_name='rsift').
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "common.hpp"

struct gtx_ctx;

namespace gtx {

struct SiftKeypoint {
  float x, y;        // full-resolution pixels of the input image
  float size;        // diameter of the meaningful neighbourhood
  float angle;       // degrees, [0, 360)
  float response;    // |contrast|
  int octave;        // OpenCV packing: octave | layer << 8 | sub-layer offset << 16
};

class Sift {
 public:
  // Buffers are sized for images up to max_h x max_w (the Gaussian / DoG pyramids of the doubled
  // image stay resident: ~ 59 bytes per doubled pixel).
  Sift(int device, hipStream_t stream, int max_h, int max_w);
  ~Sift();
  // image: BGR u8 [h][w][3] on the HOST. Keypoints (OpenCV order: by octave, layer, row, column,
  // orientation bin) with their descriptors (128 floats each; RootSIFT when root) are left on the
  // device; n = number of keypoints (<= max_features, the strongest responses are retained).
  void detect_and_compute(const uint8_t* image_bgr, int h, int w, int max_features, bool root, float root_eps);
  // The same result from a u8 gray image [h][w] in HBM, read in place, with nothing but launches on the object's stream: no host
  // wait and no host work. The counts stay in HBM (counters_dev: candidates, refined, oriented, keypoints kept); the strongest
  // max_features are selected, ordered and finalised by kernels, and the kept keypoints whose rounded position lies inside one of
  // the inclusive rectangles (x1, y1, x2, y2; pixels of the image; device memory) are then dropped, as cv2's detectAndCompute does
  // with a mask. count() and keypoints_host() do not cover this path. reserve_async sizes its buffers and may wait for the device;
  // check_counters fails (as detect_and_compute does) when a stage counted more than its list holds.
  void reserve_async(int max_features);
  void extract_async(const uint8_t* gray_dev, int h, int w, int max_features, bool root, float root_eps, const int4* mask_rects_dev, int n_rects);
  const int* counters_dev() const;               // [4]
  const SiftKeypoint* keypoints_dev() const;     // [kept] rows as gtx_sift_detect reports them
  void check_counters(const int counters[4], int max_features) const;
  static size_t resident_bytes(int max_h, int max_w);     // what an object for images up to max_h x max_w keeps in HBM
  int count() const;
  const float* descriptors_dev() const;         // [n][128] fp32
  const float2* positions_dev() const;          // [n] (x, y)
  void download(std::vector<SiftKeypoint>& kps, std::vector<float>& desc) const;
  const std::vector<SiftKeypoint>& keypoints_host() const;   // the keypoints alone: no copy of the descriptors (128 MB at 250 000 keypoints)
  // test hooks: pyramid image (kind 0 = Gaussian, 1 = DoG) of the last image
  void pyramid_image(int kind, int octave, int layer, std::vector<float>& out, int* h, int* w) const;
  int n_octaves() const;
  // GPU ms of the last detect_and_compute: [0] upload + gray + pyramid, [1] extrema + refine + orientation, [2] descriptors; [3] = pixels
  // of the doubled base image (the pyramid holds 11 x 4/3 fp32 images of that size)
  void stage_ms(float out[4]) const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

// ---- gtx_op_sift_*: one stage each on host arrays (arguments checked by the caller, gtx_ops.cpp; record layouts: include/gtx.h)
// radius of the Gaussian the scale space would use for sigma; fails above the kernels' largest (16), as every blur does
int sift_blur_radius(double sigma);
// one Gaussian blur (+ DoG layer when dog is given): form 0 as the pyramid dispatches it, 1 the generic tile kernel, 2 row / column / subtraction passes
void op_sift_blur(gtx_ctx* ctx, const float* src, int h, int w, double sigma, int form, float* dst, float* dog);
// the three extrema passes over the five DoG layers of one octave: every candidate counted, at most cap stored
void op_sift_extrema(gtx_ctx* ctx, const float* dog5, int h, int w, int octave, int cap, int* count, int* cand);
// refine_kernel on n candidates of that octave: the accepted ones, in no particular order, each with the candidate it came from
void op_sift_refine(gtx_ctx* ctx, const float* dog5, int h, int w, int octave, const int* cand, int n, int* count, void* out);
// orient_kernel on n refined records over one Gaussian layer: every peak counted, at most cap stored; hist [n][36] smoothed histograms
void op_sift_orient(gtx_ctx* ctx, const float* gauss_layer, int h, int w, int octave, const void* refined, int n, int cap, int* count, void* out,
                    float* hist);
// describe_kernel on n final records over one Gaussian layer: desc [n][128]
void op_sift_describe(gtx_ctx* ctx, const float* gauss_layer, int h, int w, const void* finals, int n, int root, float root_eps, float* desc);
// the selection / finalisation / mask launches of extract_async on n oriented records: count kept, then their final records [count][8],
// positions [count][2], keypoint rows [count][5] and octave words [count]; rects [n_rects][4] inclusive (x1, y1, x2, y2)
void op_sift_select(gtx_ctx* ctx, const void* oriented, int n, int max_features, const int* rects, int n_rects, int* count, void* finals, float* xy,
                    float* kp5, int* octave);
int sift_select_max_features();
int sift_select_max_rects();

}  // namespace gtx
