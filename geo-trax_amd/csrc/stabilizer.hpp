// GPU homography stabilizer (ORB-style keypoints + Hamming matching + RANSAC homography).
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

// clahe.hip: cv2.createCLAHE(2.0, (8, 8)).apply on a u8 image in HBM (src == dst allowed); luts: kClaheLutBytes of scratch.
constexpr int kClaheLutBytes = 8 * 8 * 256;
void clahe_dev(const uint8_t* src, int h, int w, uint8_t* luts, uint8_t* dst, hipStream_t s);
// cv2.createCLAHE(2.0, (8, 8)).apply(gray), host image in / out (what `clahe: true` runs on the working gray image).
void clahe_image(gtx_ctx* ctx, const uint8_t* gray, int h, int w, uint8_t* out);

// Robust homography (MSAC hypotheses on the GPU + IRLS refit on the host, f64) from n_match point pairs
// (x, y) -> (z, w) in HBM; threshold in pixels of the destination. false: no model.
bool ransac_homography(int device, hipStream_t s, const float4* d_pts, int n_match, unsigned seed, int n_hyp, int frame_w, int frame_h,
                       float threshold, double H[9], int* n_inliers);

// The same in two halves, for a caller whose pair count is in HBM and who must not wait between them: state_dev is two words that
// ransac_arm sets once (the kernel leaves them armed), record_dev ransac_record_bytes() of HBM. n_cur_dev is copied into the record.
// After the stream has run: copy the record and the pairs to the host, read the counts, and ransac_finish does the refit.
size_t ransac_record_bytes();
void ransac_arm(unsigned long long* state_dev, hipStream_t s);
void ransac_submit(hipStream_t s, const float4* d_pts, const int* n_pairs_dev, const int* n_cur_dev, unsigned seed, int n_hyp, int frame_w, int frame_h,
                   float threshold, unsigned long long* state_dev, void* record_dev);
void ransac_record_counts(const void* record_host, int* n_pairs, int* n_cur);
bool ransac_finish(const void* record_host, const float4* pts_host, int frame_w, int frame_h, float threshold, double H[9], int* n_inliers);

// Operator hooks: one launch of the matcher / of the RANSAC kernel on host arrays, exactly as the stabilizer launches them (sizes are
// validated by the caller, gtx_ops.cpp). Their ticket / state words live with the context and are never re-initialised by the host.
void op_orb_match(gtx_ctx* ctx, const uint8_t* desc_q, int nq, int slots_q, const uint8_t* desc_t, int nt, int slots_t, float ratio, int keep_all,
                  const float* xy_q, const float* xy_t, int* best_idx, int* best_d, int* second_d, int* m_q, int* m_t, int* m_d, float* m_pts,
                  int* n_match);
void op_orb_ransac(gtx_ctx* ctx, const float* pts, int n, unsigned seed, int n_hyp, int frame_w, int frame_h, float thr, int affine, int* best,
                   long long* cost, double H[9]);
}  // namespace gtx

struct gtx_stabilizer {
  std::unique_ptr<gtx::Stabilizer> impl;
};
