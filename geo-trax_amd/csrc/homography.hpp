// Robust homography from matched point pairs: MSAC-scored hypotheses in one GPU launch (homography.hip), then an IRLS refit of
// the winner on the host in f64 (homography_refit.cpp). The ORB stabilizer, the SIFT stabilizer and the registration share it.
#pragma once
#include <cstddef>

struct gtx_ctx;

namespace gtx {

// The solver's normalised coordinates: (p - c) * sc maps the frame onto [-1, 1] across its width. The kernel and the refit must agree.
struct FrameNorm {
  double cx, cy, sc;
  FrameNorm(int frame_w, int frame_h) : cx(frame_w / 2.0), cy(frame_h / 2.0), sc(2.0 / frame_w) {}
};

// The host half: the IRLS refit of the hypothesis H0 as the kernel wrote it (divided by H0[8] here) on n pairs (x, y) -> (z, w),
// [n][4] float32; thr in pixels. true: H (h33 = 1) and the matches within thr of it. false: no model, H untouched.
bool refine_homography(const float* pairs, int n, int frame_w, int frame_h, double thr, bool affine, const double H0[9], double H[9],
                       int* n_inliers);

}  // namespace gtx

#ifdef __HIPCC__   // the GPU half; the refit and the host-only sanitizer driver are built without HIP and stop here
#include <hip/hip_runtime.h>

namespace gtx {

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
                   float threshold, int affine, unsigned long long* state_dev, void* record_dev);
void ransac_record_counts(const void* record_host, int* n_pairs, int* n_cur);
bool ransac_finish(const void* record_host, const float4* pts_host, int frame_w, int frame_h, float threshold, bool affine, double H[9], int* n_inliers);

// Operator hook: one launch of the RANSAC kernel on host arrays, exactly as the stabilizers launch it (sizes are validated by the
// caller, gtx_ops.cpp). Its state words live with the context (gtx_ctx::orb_ransac_state) and are never re-initialised by the host.
void op_orb_ransac(gtx_ctx* ctx, const float* pts, int n, unsigned seed, int n_hyp, int frame_w, int frame_h, float thr, int affine, int* best,
                   long long* cost, double H[9]);

}  // namespace gtx
#endif
