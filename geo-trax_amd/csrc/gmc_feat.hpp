// BoT-SORT global motion compensation, method 'orb', stream-ordered on the GPU, see gmc_feat.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>

#include "common.hpp"

struct gtx_ctx;

namespace gtx {

class FeatGmc {
 public:
  // frame_h x frame_w: the full-resolution frame; the method works on its half-resolution gray image.
  FeatGmc(gtx_ctx* ctx, int frame_h, int frame_w, int max_features, int seed);
  ~FeatGmc();
  void reset();                                               // forget the previous frame (nothing may be in flight)
  void restart();                                             // the next submitted frame opens a new sequence; frames may be in flight
  // Asynchronous pair, as Gmc's: keypoints + descriptors -> 2-NN against the previous frame's -> ratio / spatial filters ->
  // RANSAC, all on the context's stream; the refit on the host in collect(). Up to 64 frames may be submitted ahead (the image
  // is copied at submit); collect() returns them in submission order. One thread may submit while another collects.
  void submit_gray_dev(const void* gray, int gh, int gw);
  void submit_gray(const uint8_t* gray_host, int gh, int gw);
  // BGR u8 frame in HBM: gray + 2x2 mean first. restart: this frame opens a new sequence (see Gmc::submit_frame_dev).
  void submit_frame_dev(const void* frame_bgr_dptr, int h, int w, bool restart);
  // A: row-major 2x3 f64 in full-resolution pixels (identity on the first frame of a sequence or when fewer than 5 pairs
  // survived; valid tells which). stats = {keypoints of the previous frame, pairs kept, inliers}.
  void collect(double A[6], int* valid, int stats[3]);
  // test hooks. The kept pairs of the frame collected last, rows (prev.x, prev.y, cur.x, cur.y) in match order.
  void debug_pairs(int cap, int* n, float* pairs4) const;
  // The matcher's output for the frame submitted last (nothing may be in flight): per query (= current frame) keypoint the
  // nearest previous-frame keypoint and the two smallest Hamming distances, and both sets' positions. n_q = n_t = 0 when
  // that frame opened a sequence.
  void debug_matches(int cap, int* n_q, int* n_t, int* best_idx, int* best_d, int* second_d, float* q_xy, float* t_xy) const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace gtx
