// GPU homography stabilizer (ORB-style keypoints + Hamming matching; the robust homography is homography.hpp's).
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "../../include/gtx.h"
#include "common.hpp"

struct gtx_ctx;

namespace gtx {
class Stabilizer {
 public:
  Stabilizer(gtx_ctx* ctx, const gtx_stab_config& cfg);
  ~Stabilizer();
  void set_ref_frame(const uint8_t* frame_bgr, int h, int w, const float* boxes_xywh, int n);
  void set_ref_gray_dev(const void* gray, int gh, int gw, const float* boxes_xywh, int n);
  void stabilize(const uint8_t* frame_bgr, int h, int w, const float* boxes_xywh, int n, double H[9], int* valid, int stats[4]);
  void stabilize_gray_dev(const void* gray, int gh, int gw, const float* boxes_xywh, int n, double H[9], int* valid, int stats[4]);
  // asynchronous pair: enqueue the whole pass for a gray image in HBM / wait for it and refit
  void submit_gray_dev(const void* gray, int gh, int gw, const float* boxes_xywh, int n);
  void collect(double H[9], int* valid, int stats[4]);
  void keypoints(int which, int cap, int* n, float* xy, int* level, int* angle_bin, uint8_t* desc);
  void promote_cur_to_ref();      // the last stabilized frame's features become the reference (ref_multiplier 1 only)
  void matches(int cap, int* n, int* cur_idx, int* ref_idx, int* dist);
  // rotated sampling pattern table [256 bins][256 tests][ax, ay, bx, by] int8 (data, for the oracle)
  void pattern(int8_t* out) const;
  // Debug read-backs of the LAST extract pass (like Sift::pyramid): keep_pass(true) makes every later pass keep its plan and a
  // copy of its candidate counters (one small device copy per pass; nothing when off). `which` must name the set that pass filled.
  void keep_pass(bool on);
  void level(int which, int i, int* h, int* w, uint8_t* out, size_t cap);           // pyramid level i: h x w bytes (out may be null: sizes only)
  // level i after FAST + 3x3 NMS + mask: n (pix, score) pairs in no particular order; the count stage 1 passed on to the Harris
  // ranking, the keypoints kept, and the candidates that found their sub-list full (the lists are sized so that this is 0)
  void candidates(int which, int i, int cap, int* n, int* pix, int* score, int* n_elig, int* n_kp, int* n_dropped);
  // GPU time (ms, stream-ordered events) of the last collected submit_gray_dev pass: keypoints -> matching -> RANSAC
  float last_ms() const;

  // ---- the stages on their own, for a caller that chains them on the context's stream itself (gmc_feat.hip: every frame is
  // matched against the one before it). Nothing here waits for the device or touches the object's host-side results; the two
  // feature sets must have the same plan (ref_multiplier 1).
  struct FeatureSet { const float2* xy; const int* n; };          // full-resolution keypoint positions and their count, in HBM
  struct RawMatches { const int *best_idx, *best_d, *second_d; };  // per query keypoint: nearest reference keypoint (-1: none), its and the second nearest's Hamming distance
  void extract_cur_async(const void* gray);     // keypoints + descriptors of a gray image in HBM (read in place) -> the current set
  void match_cur_async();                       // Hamming 2-NN of the current set (query) against the reference set
  void swap_sets();                             // current <-> reference: later launches see the swapped sets (host-side handles only)
  FeatureSet feature_set(int which) const;      // 0 = reference, 1 = current
  RawMatches raw_matches() const;
  int slots() const;                            // keypoint slots per set

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

// The steered-BRIEF sampling table [256 bins][256 tests][ax, ay, bx, by] (host only, no device needed).
void stabilizer_pattern_table(std::vector<int8_t>& out);

// frame pixels -> working pixels: fh / 2 x fw / 2 at ratio 0.5, the frame's size at 1.0, else rint(fh * r) x rint(fw * r)
void gray_working_size(int fh, int fw, float ratio, int* gh, int* gw);
// The stabilizer's working-resolution gray image of a BGR u8 frame in HBM, into the caller's buffer (gh * gw bytes, any alignment),
// enqueued on the context's stream: the launch Stabilizer::set_ref_frame / stabilize make for a host frame. op_gray_resize: the same
// on host arrays (staged, synchronous). The caller has validated the sizes (gtx_ops.cpp).
void gray_resize_dev(gtx_ctx* ctx, const void* bgr, int fh, int fw, float ratio, void* gray);
void op_gray_resize(gtx_ctx* ctx, const uint8_t* bgr, int fh, int fw, float ratio, uint8_t* gray);

// Operator hook: one launch of the matcher on host arrays, exactly as the stabilizer launches it (sizes are validated by the caller,
// gtx_ops.cpp). Its ticket word lives with the context (gtx_ctx::orb_match_ticket) and is never re-initialised by the host.
void op_orb_match(gtx_ctx* ctx, const uint8_t* desc_q, int nq, int slots_q, const uint8_t* desc_t, int nt, int slots_t, float ratio, int keep_all,
                  const float* xy_q, const float* xy_t, int* best_idx, int* best_d, int* second_d, int* m_q, int* m_t, int* m_d, float* m_pts,
                  int* n_match);
}  // namespace gtx

struct gtx_stabilizer {
  std::unique_ptr<gtx::Stabilizer> impl;
};
