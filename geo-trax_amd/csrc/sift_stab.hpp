// stabilo's `detector_name: sift | rsift` stabilizer as a stream-ordered chain on the detector's half-resolution gray image
// (sift_stab.cpp): SIFT extraction with every count in HBM (Sift::extract_async), L2 2-NN, Lowe's ratio and the pair list on the
// device, the RANSAC launch of the ORB stabilizer, and its robust refit on the host at collect. The blocking form of the same
// registration is register_images (register.cpp); the two give the same pairs, counts and matrix for the same images.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>

#include "../../include/gtx.h"
#include "common.hpp"

struct gtx_ctx;

namespace gtx {

class SiftStab {
 public:
  SiftStab(gtx_ctx* ctx, const gtx_sift_stab_config& cfg);
  ~SiftStab();
  // boxes xywh [n][4] in frame pixels (or null): the vehicle mask, applied to the kept keypoints (mask_use)
  void set_ref_gray_dev(const void* gray, int gh, int gw, const float* boxes_xywh, int n);    // extracts once; waits for the device
  void submit_gray_dev(const void* gray, int gh, int gw, const float* boxes_xywh, int n);     // launches and copies only: no wait
  void collect(double H[9], int* valid, int stats[4]);    // H in working-resolution pixels; stats = keypoints ref, cur, pairs, inliers
  float last_ms() const;
  void keypoints(int which, int cap, int* n, float* kp5, int* octave, float* desc);
  void pairs(int cap, int* n, float* pts);
  void counters(int out[4]) const;                        // of the last collected frame: candidates, refined, oriented, kept

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace gtx

struct gtx_sift_stab {
  std::unique_ptr<gtx::SiftStab> impl;
};
