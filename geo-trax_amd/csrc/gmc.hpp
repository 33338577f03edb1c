// BoT-SORT global motion compensation ('sparseOptFlow') on the GPU, see gmc.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>

#include "common.hpp"

struct gtx_ctx;

namespace gtx {

// Device-side record of one frame's fit: filled by the compaction step (counts, identity model), then by the RANSAC winner.
struct GmcResult {
  int n_prev, n_valid, best_count, winner;   // winner: index of the winning hypothesis (-1: none)
  double a, b, tx, ty;
};

// ---- steps shared with the feature-based methods (gmc_feat.hip), each one enqueued on `s`
constexpr int kGmcHypotheses = 512;
// BGR u8 [2 * oh][w][3] -> gray (cv2 fixed point) -> exact 2x2 mean [oh][ow], as the detector's preprocess pass writes it
void gmc_launch_gray_half(const uint8_t* bgr, int w, uint8_t* out, int oh, int ow, hipStream_t s);
// 512 two-point similarity hypotheses over pairs[0 .. res->n_valid) = (p.x, p.y, q.x, q.y), 3 px threshold, first best wins ->
// res->{best_count, a, b, tx, ty}. model / count: scratch of kGmcHypotheses entries. The procedure gtx_op_estimate_affine_partial states.
void gmc_launch_ransac(const float4* pairs, GmcResult* res, unsigned seed, double4* model, int* count, hipStream_t s);
// Host half of the fit: three rounds of least squares on the inliers of the RANSAC winner, translation x `scale`.
// false (A untouched): fewer than 5 pairs or no hypothesis.
bool gmc_refit(const GmcResult& R, const float4* pairs, double scale, double A[6], int* n_inliers);

class Gmc {
 public:
  // gray_h x gray_w: the half-resolution gray image the method works on (frame size / 2).
  Gmc(int device, hipStream_t stream, int gray_h, int gray_w, int seed);
  ~Gmc();
  void reset();                                               // forget the previous frame (nothing may be in flight)
  void restart();                                             // the next submitted frame opens a new sequence; frames may be in flight
  // asynchronous pair: corners + flow against the previous frame + RANSAC on the stream / refit on the host.
  // Up to 64 frames may be submitted ahead; collect() returns them in submission order. One thread may submit
  // while another collects.
  void submit_gray_dev(const void* gray, int gh, int gw);
  // BGR u8 host frame [2*gray_h][2*gray_w][3]: gray + 2x2 mean on the GPU, then as above
  void submit_frame(const uint8_t* frame_bgr, int h, int w);
  // The same for a frame that already lives in HBM, queued like submit_gray_dev. restart: this frame opens a new
  // sequence (its warp is the identity; the next frame is compensated against it) -- a shard rank uses it to
  // hand the GMC the frame that precedes its batch in the clip.
  void submit_frame_dev(const void* frame_bgr_dptr, int h, int w, bool restart);
  // A: row-major 2x3 f64 in full-resolution pixels (identity on the first frame or when fewer than 5
  // points were tracked; valid tells which). stats = {corners of the previous frame, tracked, inliers}.
  void collect(double A[6], int* valid, int stats[3]);
  // test hook: which 0 = corners of the last frame, 1 = corners of the frame before, 2 = their LK positions
  void debug_points(int which, int cap, int* n, float* xy, int* status) const;
  // test hook: the corner step's record of the last submitted frame = {maxima found, stored, gathered into LDS, narrowing passes}
  void debug_counts(int counts[4]) const;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

// ---- gtx_op_gmc_*: one launcher each on host arrays (arguments checked by the caller, gtx_ops.cpp)
// response + nms + select on a gray image: corners strongest first (n <= 1000) and the corner step's record (debug_counts)
void op_gmc_corners(gtx_ctx* ctx, const uint8_t* gray, int h, int w, int* n, float* xy, int counts[4]);
// pyrdown x 3 on both images + lk_kernel on n <= 1000 given points
void op_gmc_lk(gtx_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int h, int w, const float* pts, int n, float* next, int* status);
// ransac_kernel + argmax_kernel on n <= 1024 pairs: the winner's inlier count, index and (a, b, tx, ty), and every hypothesis' count
void op_gmc_ransac(gtx_ctx* ctx, const float* pairs, int n, unsigned seed, int* best_count, int* winner, double model4[4], int* count);

}  // namespace gtx
