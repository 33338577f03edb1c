// The GPU half of the robust homography solver (homography.hpp): every hypothesis made, MSAC-scored and the winner picked in one
// launch; then the public functions around it, which end in the host refit (homography_refit.cpp).
#include <hip/hip_runtime.h>

#include <cstring>

#include "homography.hpp"
#include "net_runtime.hpp"   // gtx_ctx
#include "op_staging.hpp"

namespace gtx {

namespace {

// ------------------------------------------------------------------ RANSAC
__device__ __forceinline__ unsigned hash_u32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

// Homography from 4 correspondences by the projective-basis construction: A maps the canonical
// basis (e1, e2, e3, e1+e2+e3) to the four source points, B to the four destination points,
// H = B * adj(A). Closed form, static indexing only (stays in registers), f64.
__device__ __forceinline__ bool basis_matrix(const double* px, const double* py, double* M) {
  // solve [p0 p1 p2] (l0,l1,l2)^T = p3 by Cramer's rule; columns then scaled by l
  const double x0 = px[0], y0 = py[0], x1 = px[1], y1 = py[1], x2 = px[2], y2 = py[2], x3 = px[3], y3 = py[3];
  const double det = x0 * (y1 - y2) - x1 * (y0 - y2) + x2 * (y0 - y1);
  if (!(fabs(det) > 1e-9)) return false;
  const double l0 = (x3 * (y1 - y2) - x1 * (y3 - y2) + x2 * (y3 - y1)) / det;
  const double l1 = (x0 * (y3 - y2) - x3 * (y0 - y2) + x2 * (y0 - y3)) / det;
  const double l2 = (x0 * (y1 - y3) - x1 * (y0 - y3) + x3 * (y0 - y1)) / det;
  if (!(fabs(l0) > 1e-9 && fabs(l1) > 1e-9 && fabs(l2) > 1e-9)) return false;   // three points collinear
  M[0] = l0 * x0; M[1] = l1 * x1; M[2] = l2 * x2;
  M[3] = l0 * y0; M[4] = l1 * y1; M[5] = l2 * y2;
  M[6] = l0;      M[7] = l1;      M[8] = l2;
  return true;
}
__device__ bool homography4(const double* px, const double* py, const double* qx, const double* qy, double* H) {
  double A[9], B[9];
  if (!basis_matrix(px, py, A) || !basis_matrix(qx, qy, B)) return false;
  const double adj[9] = {A[4] * A[8] - A[5] * A[7], A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
                         A[5] * A[6] - A[3] * A[8], A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
                         A[3] * A[7] - A[4] * A[6], A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]};
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) H[r * 3 + c] = B[r * 3] * adj[c] + B[r * 3 + 1] * adj[3 + c] + B[r * 3 + 2] * adj[6 + c];
  if (!(fabs(H[8]) > 1e-12)) return false;
  const double inv = 1.0 / H[8];
#pragma unroll
  for (int i = 0; i < 9; ++i) H[i] *= inv;
  return true;
}

// Affine map from 3 correspondences (Cramer's rule), as a 3x3 matrix with last row (0, 0, 1).
__device__ bool affine3(const double* px, const double* py, const double* qx, const double* qy, double* H) {
  const double x0 = px[0], y0 = py[0], x1 = px[1], y1 = py[1], x2 = px[2], y2 = py[2];
  const double det = x0 * (y1 - y2) - y0 * (x1 - x2) + (x1 * y2 - x2 * y1);
  if (!(fabs(det) > 1e-9)) return false;           // the three source points are collinear
  const double id = 1.0 / det;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double* q = r == 0 ? qx : qy;
    const double u0 = q[0], u1 = q[1], u2 = q[2];
    H[r * 3 + 0] = (u0 * (y1 - y2) - y0 * (u1 - u2) + (u1 * y2 - u2 * y1)) * id;
    H[r * 3 + 1] = (x0 * (u1 - u2) - u0 * (x1 - x2) + (x1 * u2 - x2 * u1)) * id;
    H[r * 3 + 2] = (x0 * (y1 * u2 - y2 * u1) - y0 * (x1 * u2 - x2 * u1) + u0 * (x1 * y2 - x2 * y1)) * id;
  }
  H[6] = 0.0; H[7] = 0.0; H[8] = 1.0;
  return true;
}

// One hypothesis: 4 (projective) or 3 (affine) distinct matches drawn by a counter-based hash of (seed, hypothesis, draw),
// exact minimal solve in normalised coordinates, de-normalised H. Straight-line f64 code without LDS: every lane of a wave
// runs it on the same inputs and gets the same bits, which is how the scoring wave below obtains its hypothesis.
__device__ __forceinline__ bool make_hypothesis(const float4* __restrict__ pts, int n, unsigned seed, int hyp, double cx, double cy, double sc, int affine, double H[9]) {
  // inlined, and every small array indexed by unrolled constants: as a call with H behind a pointer and idx[] indexed by a
  // run-time k the kernel kept 80 bytes of scratch per lane -- 9.2 MB of HBM writes per launch for a one-record result
  // (profiles/r05_pmc_traffic.json)
  const int ns = affine ? 3 : 4;
  if (n < ns) return false;
  int idx[4] = {0, 0, 0, 0};
  unsigned ctr = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= ns) break;
    for (;;) {
      const int cand = (int)(hash_u32(seed ^ hash_u32((unsigned)hyp * 977u + ctr)) % (unsigned)n);
      ++ctr;
      bool dup = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) dup |= (j < k) && idx[j] == cand;
      if (!dup) { idx[k] = cand; break; }
    }
  }
  double px[4], py[4], qx[4], qy[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 p = pts[idx[k]];
    px[k] = ((double)p.x - cx) * sc; py[k] = ((double)p.y - cy) * sc;
    qx[k] = ((double)p.z - cx) * sc; qy[k] = ((double)p.w - cy) * sc;
  }
  double Hn[9];
  if (!(affine ? affine3(px, py, qx, qy, Hn) : homography4(px, py, qx, qy, Hn))) return false;
  // de-normalise: H = T^-1 Hn T with T = [[sc,0,-sc*cx],[0,sc,-sc*cy],[0,0,1]]
  const double is = 1.0 / sc;
  double M[9];
  for (int r = 0; r < 3; ++r) {   // M = Hn T
    M[r * 3 + 0] = Hn[r * 3 + 0] * sc;
    M[r * 3 + 1] = Hn[r * 3 + 1] * sc;
    M[r * 3 + 2] = Hn[r * 3 + 2] - sc * (Hn[r * 3 + 0] * cx + Hn[r * 3 + 1] * cy);
  }
  for (int k = 0; k < 3; ++k) {   // H = T^-1 M, T^-1 = [[is,0,cx],[0,is,cy],[0,0,1]]
    H[0 + k] = is * M[0 + k] + cx * M[6 + k];
    H[3 + k] = is * M[3 + k] + cy * M[6 + k];
    H[6 + k] = M[6 + k];
  }
  return fabs(H[8]) > 1e-12;
}

// Device-side result record of one stabilize pass, fetched with a single D2H copy (the match points follow it in the same
// buffer: StabOut).
struct StabResult {
  int n_match, best, n_cur, pad;
  double H[9];
  long cost;        // the winner's MSAC cost in 1/1024 px^2 (0 when there is none); the record stays 96 bytes with its padding
};

// Hypothesise, score and pick the winner in ONE launch (round 4; three launches before: solve, score, argmin).
// A wave makes hypothesis `hyp` (every lane the same solve) and scores it: truncated squared reprojection error (MSAC) over
// all matches, quantised to 1/1024 px^2 so that the sum is an exact integer regardless of the reduction order. The
// workgroup's 8 costs are reduced in LDS to one key (cost << 16 | hyp: the lowest cost, then the lowest hypothesis index,
// exactly the order of the former argmin) and folded into `state[0]` with one device-scope atomic minimum; `state[1]` is a
// ticket: the workgroup that draws the last one knows every minimum has been applied (each workgroup's ticket add depends on
// the value its minimum returned), reads the winner back with another atomic, re-derives its H from the index, writes the
// result record and re-arms state for the next pass. Device-scope atomics are performed beyond the per-XCD L2s, so no
// fence and no other cross-workgroup visibility is involved.
constexpr unsigned long long kNoHyp = ~0ull;
__global__ __launch_bounds__(512) void ransac_kernel(const float4* __restrict__ pts, const int* __restrict__ n_p, const int* __restrict__ n_cur_p,
                                                      unsigned seed, int n_hyp, double cx, double cy, double sc, int affine, float thr2,
                                                      unsigned long long* __restrict__ state /*[2]: best key (armed: all ones), tickets (0)*/,
                                                      StabResult* __restrict__ res) {
  constexpr int kHypPerWg = 8;
  __shared__ unsigned long long s_key[kHypPerWg];
  __shared__ int s_last;
  const int n = *n_p;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int hyp = blockIdx.x * kHypPerWg + wv;
  unsigned long long key = kNoHyp;
  if (hyp < n_hyp) {
    double H[9];
    if (make_hypothesis(pts, n, seed, hyp, cx, cy, sc, affine, H)) {
      long acc = 0;
      for (int i = lane; i < n; i += 64) {
        const float4 p = pts[i];
        const double x = p.x, y = p.y;
        const double w = H[6] * x + H[7] * y + H[8];
        double e = (double)thr2;
        if (fabs(w) > 1e-12) {
          const double iw = 1.0 / w;
          const double dx = (H[0] * x + H[1] * y + H[2]) * iw - p.z;
          const double dy = (H[3] * x + H[4] * y + H[5]) * iw - p.w;
          e = fmin(dx * dx + dy * dy, (double)thr2);
        }
        acc += (long)(e * 1024.0 + 0.5);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
      key = ((unsigned long long)acc << 16) | (unsigned long long)hyp;     // cost < 2^47 (4096 per match at most), hyp < 2^16
    }
  }
  if (lane == 0) s_key[wv] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long k = s_key[0];
#pragma unroll
    for (int i = 1; i < kHypPerWg; ++i) k = min(k, s_key[i]);
    // The ordering is the memory model's: the minimum is published by the RELEASE half of the ticket's acq_rel read-modify-write
    // (agent scope), and the workgroup that draws the last ticket ACQUIRES every earlier workgroup's release through the
    // ticket word's modification order (a release sequence of RMWs), so its read of state[0] below sees every minimum.
    // The s_waitcnt between the two is not part of that argument: cdna_hip_programming.md (section 6, Guideline 16, Pitfall 12)
    // records that ROCm 7.2 can drop the wait a release implies, and prescribes keeping an explicit one in front of the ticket.
    (void)__hip_atomic_fetch_min(&state[0], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long ticket = __hip_atomic_fetch_add(&state[1], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_last = ticket == (unsigned long long)gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  // ---- the last workgroup: every minimum has been applied
  if (wv != 0) return;
  unsigned long long best_key = 0;
  if (lane == 0) best_key = __hip_atomic_fetch_min(&state[0], kNoHyp, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);   // acquire read-back, in L2
  best_key = __shfl(best_key, 0, 64);
  const int b = best_key == kNoHyp ? -1 : (int)(best_key & 0xffffull);
  double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (b >= 0) make_hypothesis(pts, n, seed, b, cx, cy, sc, affine, H);
  if (lane == 0) {
    res->n_match = n;
    res->n_cur = *n_cur_p;
    res->best = b;
    for (int k = 0; k < 9; ++k) res->H[k] = H[k];
    res->cost = b >= 0 ? (long)(best_key >> 16) : 0;
    atomicExch(&state[0], kNoHyp);                                         // re-arm for the next pass on this stream
    atomicExch(&state[1], 0ull);
  }
}

// The armed state of the two words a launch works on: no winner yet, no ticket drawn. The kernel leaves them so.
constexpr unsigned long long kArmed[2] = {kNoHyp, 0ull};

// The RANSAC launch: n_hyp hypotheses, 8 per workgroup, on a state that is armed between launches.
void launch_ransac_kernel(hipStream_t s, const float4* pts, const int* n_p, const int* n_cur_p, unsigned seed, int n_hyp, int frame_w, int frame_h,
                          int affine, float thr, unsigned long long* state, StabResult* res) {
  const FrameNorm f(frame_w, frame_h);
  hipLaunchKernelGGL(ransac_kernel, dim3(cdiv(n_hyp, 8)), dim3(512), 0, s, pts, n_p, n_cur_p, seed, n_hyp, f.cx, f.cy, f.sc, affine, thr * thr, state, res);
}
}  // namespace

// Blocking robust homography from matched point pairs already in HBM (registration path): the same launch as the per-frame
// stabilizers', then the host IRLS refit.
bool ransac_homography(int device, hipStream_t s, const float4* d_pts, int n_match, unsigned seed, int n_hyp, int frame_w, int frame_h,
                       float threshold, double H[9], int* n_inliers) {
  *n_inliers = 0;
  if (n_match < 4) return false;
  GTX_HIP(hipSetDevice(device));
  DevBuf d_n(sizeof(int) * 2), d_state(sizeof kArmed), d_res(sizeof(StabResult));
  const int two[2] = {n_match, n_match};
  GTX_HIP(hipMemcpyAsync(d_n.p, two, sizeof two, hipMemcpyHostToDevice, s));
  GTX_HIP(hipMemcpyAsync(d_state.p, kArmed, sizeof kArmed, hipMemcpyHostToDevice, s));
  GTX_CHECK(n_hyp <= 65536, "ransac: at most 65536 hypotheses (got %d)", n_hyp);
  launch_ransac_kernel(s, d_pts, d_n.as<int>(), d_n.as<int>() + 1, seed, n_hyp, frame_w, frame_h, 0, threshold, d_state.as<unsigned long long>(),
                       d_res.as<StabResult>());
  GTX_HIP(hipGetLastError());
  StabResult R;
  std::vector<float4> pts(n_match);
  GTX_HIP(hipMemcpyAsync(&R, d_res.p, sizeof R, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipMemcpyAsync(pts.data(), d_pts, sizeof(float4) * n_match, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipStreamSynchronize(s));
  return ransac_finish(&R, pts.data(), frame_w, frame_h, threshold, false, H, n_inliers);
}

// The two halves of ransac_homography for a chain that keeps the pair count in HBM and must not wait (stabilizer.hip, sift_stab.cpp):
// ransac_submit enqueues the one launch on a state that ransac_arm initialised once (the kernel re-arms it), ransac_finish is the host
// half on the record and the pairs the caller copied back.
size_t ransac_record_bytes() { return sizeof(StabResult); }

void ransac_arm(unsigned long long* state_dev, hipStream_t s) {
  GTX_HIP(hipMemcpyAsync(state_dev, kArmed, sizeof kArmed, hipMemcpyHostToDevice, s));
  GTX_HIP(hipStreamSynchronize(s));
}

void ransac_submit(hipStream_t s, const float4* d_pts, const int* n_pairs_dev, const int* n_cur_dev, unsigned seed, int n_hyp, int frame_w, int frame_h,
                   float threshold, int affine, unsigned long long* state_dev, void* record_dev) {
  GTX_CHECK(n_hyp <= 65536, "ransac: at most 65536 hypotheses (got %d)", n_hyp);
  launch_ransac_kernel(s, d_pts, n_pairs_dev, n_cur_dev, seed, n_hyp, frame_w, frame_h, affine, threshold, state_dev, static_cast<StabResult*>(record_dev));
  GTX_HIP(hipGetLastError());
}

void ransac_record_counts(const void* record_host, int* n_pairs, int* n_cur) {
  const StabResult& R = *static_cast<const StabResult*>(record_host);
  *n_pairs = R.n_match;
  *n_cur = R.n_cur;
}

bool ransac_finish(const void* record_host, const float4* pts_host, int frame_w, int frame_h, float threshold, bool affine, double H[9], int* n_inliers) {
  const StabResult& R = *static_cast<const StabResult*>(record_host);
  *n_inliers = 0;
  if (R.n_match < (affine ? 3 : 4) || R.best < 0) return false;
  return refine_homography(reinterpret_cast<const float*>(pts_host), R.n_match, frame_w, frame_h, (double)threshold, affine, R.H, H, n_inliers);
}

// ---- operator hook (gtx_op_orb_ransac): one launch of ransac_kernel on host arrays. The state lives with the context and is armed
// once, when the first hook call allocates it: every later call finds it as the launch before it left it, which is how the kernel's
// re-arming is exercised. The caller has validated all sizes.
void op_orb_ransac(gtx_ctx* ctx, const float* pts, int n, unsigned seed, int n_hyp, int frame_w, int frame_h, float thr, int affine, int* best,
                   long long* cost, double H[9]) {
  GTX_HIP(hipSetDevice(ctx->device));
  if (!ctx->orb_ransac_state) {
    GTX_HIP(hipMalloc(&ctx->orb_ransac_state, sizeof kArmed));
    ransac_arm(static_cast<unsigned long long*>(ctx->orb_ransac_state), ctx->stream);
  }
  DevBuf dp, dn, dr;
  upload(dp, pts, sizeof(float4) * (size_t)n, sizeof(float4));
  const int counts[2] = {n, n};
  upload(dn, counts, sizeof counts, sizeof counts);
  fill_ff(dr, sizeof(StabResult));
  launch_ransac_kernel(ctx->stream, dp.as<float4>(), dn.as<int>(), dn.as<int>() + 1, seed, n_hyp, frame_w, frame_h, affine, thr,
                       static_cast<unsigned long long*>(ctx->orb_ransac_state), dr.as<StabResult>());
  GTX_HIP(hipGetLastError());
  GTX_HIP(hipStreamSynchronize(ctx->stream));
  StabResult R;
  download(&R, dr, sizeof R);
  *best = R.best;
  *cost = R.cost;
  std::memcpy(H, R.H, sizeof R.H);
}

}  // namespace gtx
