// BoT-SORT global motion compensation, method 'orb', on the GPU (gfx950), stream-ordered like gmc.hip's 'sparseOptFlow'.
// Replaces ultralytics.trackers.utils.gmc.GMC.apply_features(method='orb', downscale=2) as BOTSORT.update calls it
// (`gmc_method: orb`, geotrax/cfg/default.yaml:374,419,467). oracle/gmc_ref.py GmcFeatureRef is the CPU restatement.
//
// One submit = one chain on the context's stream, no host round trip before collect():
//   copy / gray    : the caller's half-resolution gray image is copied (or made from the BGR frame by gmc.hip's gray + 2x2 mean)
//   extract        : the stabilizer's kernels -- 8-level pyramid, FAST, Harris ranking, steered BRIEF -> the "current" feature set
//   match          : the stabilizer's Hamming 2-NN kernel, current set (query) against the previous frame's
//   filter         : (this file) one workgroup: Lowe ratio 0.9, |displacement| < 0.25 x frame size, displacement - mean < 2.5 sigma
//                    per axis over the pairs kept so far, ordered compaction -> pairs + counts
//   ransac, argmax : gmc.hip's two-point similarity hypotheses (512, 3 px, first best), pairs in full-resolution pixels
//   D2H            : result record + pairs into pinned ring slots, one event
// and the two feature sets change roles (host-side handles: the launches queued later see them swapped).
// collect(): gmc.hip's least-squares refit on the host.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstring>

#include "detector.hpp"   // gtx_ctx
#include "gmc.hpp"
#include "gmc_feat.hpp"
#include "stabilizer.hpp"

namespace gtx {

namespace {

constexpr int kMaxFeat = 1024;      // keypoints per frame the one-workgroup filter takes
constexpr float kRatio = 0.9f;      // Lowe's ratio of apply_features

// Sum of one value per thread over the workgroup, in a fixed order: a binary tree over the thread index. The sums decide
// which pairs survive (mean and sigma below), so they must not depend on how the waves were scheduled.
__device__ __forceinline__ void block_sum2(double* s_x, double* s_y, int tid, double vx, double vy, double& ox, double& oy) {
  s_x[tid] = vx; s_y[tid] = vy;
  __syncthreads();
  for (int o = kMaxFeat / 2; o >= 1; o >>= 1) {
    if (tid < o) { s_x[tid] += s_x[tid + o]; s_y[tid] += s_y[tid + o]; }
    __syncthreads();
  }
  ox = s_x[0]; oy = s_y[0];
  __syncthreads();
}

// What geotrax_amd/gmc.py did on the host with numpy (float64): ratio test on the matcher's (best, second) distances, then
// filter_matches -- d = previous - current position; |d| < (lim_x, lim_y); over those: d - mean(d) < 2.5 std(d) per axis
// (one-sided, population std, as upstream writes it) --, then the survivors in query order as (prev.x, prev.y, cur.x, cur.y).
// Thread i owns query keypoint i (n_q <= 1024).
__global__ __launch_bounds__(kMaxFeat) void feat_filter_kernel(const int* __restrict__ best_idx, const int* __restrict__ best_d,
                                                               const int* __restrict__ second_d, const int* __restrict__ nq_p,
                                                               const int* __restrict__ nt_p, const float2* __restrict__ q_xy,
                                                               const float2* __restrict__ t_xy, double lim_x, double lim_y,
                                                               float4* __restrict__ pairs, GmcResult* __restrict__ res) {
  __shared__ double s_x[kMaxFeat], s_y[kMaxFeat];
  __shared__ int s_scan[kMaxFeat];
  const int tid = threadIdx.x;
  const int nq = min(*nq_p, kMaxFeat), nt = *nt_p;
  bool keep = false;
  double dx = 0.0, dy = 0.0;
  float2 p = make_float2(0.f, 0.f), q = p;
  if (tid < nq && nt >= 2) {
    const int bi = best_idx[tid];
    if (bi >= 0 && bi < nt && (float)best_d[tid] < kRatio * (float)second_d[tid]) {
      q = q_xy[tid]; p = t_xy[bi];
      dx = (double)p.x - (double)q.x; dy = (double)p.y - (double)q.y;
      keep = fabs(dx) < lim_x && fabs(dy) < lim_y;
    }
  }
  const int n1 = __syncthreads_count(keep ? 1 : 0);
  double sx, sy;
  block_sum2(s_x, s_y, tid, keep ? dx : 0.0, keep ? dy : 0.0, sx, sy);
  const double cnt = (double)max(n1, 1);
  const double ex = dx - sx / cnt, ey = dy - sy / cnt;
  double vx, vy;
  block_sum2(s_x, s_y, tid, keep ? ex * ex : 0.0, keep ? ey * ey : 0.0, vx, vy);
  keep = keep && ex < 2.5 * sqrt(vx / cnt) && ey < 2.5 * sqrt(vy / cnt);
  s_scan[tid] = keep ? 1 : 0;
  __syncthreads();
  for (int o = 1; o < kMaxFeat; o <<= 1) {
    const int v = tid >= o ? s_scan[tid - o] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  if (keep) pairs[s_scan[tid] - 1] = make_float4(p.x, p.y, q.x, q.y);
  if (tid == kMaxFeat - 1) { res->n_prev = nt; res->n_valid = s_scan[tid]; res->best_count = -1; res->winner = -1; res->a = 1; res->b = 0; res->tx = 0; res->ty = 0; }
}

}  // namespace

struct FeatGmc::Impl {
  gtx_ctx* ctx = nullptr;
  int fh = 0, fw = 0, gh = 0, gw = 0;
  unsigned seed = 0;
  std::unique_ptr<Stabilizer> st;      // owns the pyramid / keypoint / matcher buffers and the two feature sets
  DevBuf gray, pairs, res, model, count;
  bool have_prev = false;              // submit-side state
  bool last_first = true;              // the frame submitted last opened a sequence (no match ran for it)
  static constexpr int kRing = 64;
  GmcResult* h_res = nullptr;          // pinned [kRing]
  float4* h_pairs = nullptr;           // pinned [kRing][kMaxFeat]
  hipEvent_t done[kRing] = {};
  bool first[kRing] = {};
  std::atomic<unsigned> submitted{0}, collected{0};
  int last_slot = -1;                  // collect-side: slot of the frame collected last
  int pending() const { return (int)(submitted.load(std::memory_order_acquire) - collected.load(std::memory_order_acquire)); }

  enum Source { kGrayDev, kGrayHost, kFrameDev };
  void submit(const void* src, Source kind);
};

FeatGmc::FeatGmc(gtx_ctx* ctx, int frame_h, int frame_w, int max_features, int seed) : impl_(new Impl) {
  Impl& S = *impl_;
  GTX_CHECK(max_features >= 8 && max_features <= kMaxFeat, "gmc orb: max_features %d outside [8, %d]", max_features, kMaxFeat);
  S.ctx = ctx; S.fh = frame_h; S.fw = frame_w; S.gh = frame_h / 2; S.gw = frame_w / 2; S.seed = (unsigned)seed;
  GTX_HIP(hipSetDevice(ctx->device));
  gtx_stab_config cfg{};
  cfg.downsample_ratio = 0.5f; cfg.max_features = max_features; cfg.ref_multiplier = 1.0f; cfg.filter_ratio = kRatio;
  cfg.ransac_threshold = 2.0f; cfg.ransac_max_iter = 5000; cfg.ransac_confidence = 0.999999f; cfg.mask_use = 0; cfg.mask_margin_ratio = 0.15f;
  cfg.fast_threshold = 20; cfg.n_levels = 8; cfg.scale_factor = 1.2f; cfg.seed = (uint32_t)seed; cfg.frame_h = frame_h; cfg.frame_w = frame_w;
  S.st.reset(new Stabilizer(ctx, cfg));
  GTX_CHECK(S.st->slots() <= kMaxFeat, "gmc orb: %d keypoint slots", S.st->slots());
  S.gray.alloc((size_t)S.gh * S.gw);
  S.pairs.alloc(sizeof(float4) * kMaxFeat);
  S.res.alloc(sizeof(GmcResult));
  S.model.alloc(sizeof(double4) * kGmcHypotheses);
  S.count.alloc(sizeof(int) * kGmcHypotheses);
  GTX_HIP(hipHostMalloc((void**)&S.h_res, sizeof(GmcResult) * Impl::kRing));
  GTX_HIP(hipHostMalloc((void**)&S.h_pairs, sizeof(float4) * kMaxFeat * Impl::kRing));
  for (auto& e : S.done) GTX_HIP(hipEventCreateWithFlags(&e, wait_event_flags(false)));
  GTX_HIP(hipStreamSynchronize(ctx->stream));
}

FeatGmc::~FeatGmc() {
  if (!impl_) return;
  Impl& S = *impl_;
  // the context may be gone already (objects torn down in any order at interpreter exit): nothing here reads it; hipHostFree
  // and hipFree wait for the device themselves
  if (S.h_res) (void)hipHostFree(S.h_res);
  if (S.h_pairs) (void)hipHostFree(S.h_pairs);
  for (auto& e : S.done)
    if (e) (void)hipEventDestroy(e);
}

void FeatGmc::reset() {
  GTX_CHECK(impl_->pending() == 0, "gmc orb: reset while a frame is in flight");
  impl_->have_prev = false;
}

void FeatGmc::restart() { impl_->have_prev = false; }   // submit-side state only

void FeatGmc::Impl::submit(const void* src, Source kind) {
  GTX_CHECK(pending() < kRing, "gmc orb: %d frames already in flight, collect first", pending());
  const int slot = (int)(submitted.load(std::memory_order_relaxed) % kRing);
  GTX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  uint8_t* g = gray.as<uint8_t>();
  // one gray buffer: everything that reads it (pyramid, FAST, BRIEF of this frame) is ahead of the next frame's copy on the stream
  if (kind == kFrameDev) gmc_launch_gray_half(static_cast<const uint8_t*>(src), fw, g, gh, gw, s);
  else GTX_HIP(hipMemcpyAsync(g, src, (size_t)gh * gw, kind == kGrayHost ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
  st->extract_cur_async(g);
  first[slot] = !have_prev;
  if (have_prev) {
    st->match_cur_async();
    const Stabilizer::FeatureSet cur = st->feature_set(1), prev = st->feature_set(0);
    const Stabilizer::RawMatches m = st->raw_matches();
    hipLaunchKernelGGL(feat_filter_kernel, dim3(1), dim3(kMaxFeat), 0, s, m.best_idx, m.best_d, m.second_d, cur.n, prev.n, cur.xy, prev.xy,
                       0.25 * (double)fw, 0.25 * (double)fh, pairs.as<float4>(), res.as<GmcResult>());
    gmc_launch_ransac(pairs.as<float4>(), res.as<GmcResult>(), seed, model.as<double4>(), count.as<int>(), s);
    GTX_HIP(hipMemcpyAsync(h_res + slot, res.p, sizeof(GmcResult), hipMemcpyDeviceToHost, s));
    GTX_HIP(hipMemcpyAsync(h_pairs + (size_t)slot * kMaxFeat, pairs.p, sizeof(float4) * kMaxFeat, hipMemcpyDeviceToHost, s));
  }
  st->swap_sets();                     // this frame's features are the next frame's reference (no second extraction)
  GTX_HIP(hipGetLastError());
  GTX_HIP(hipEventRecord(done[slot], s));
  last_first = first[slot];
  submitted.fetch_add(1, std::memory_order_release);
  have_prev = true;
}

void FeatGmc::submit_gray_dev(const void* gray, int gh, int gw) {
  Impl& S = *impl_;
  GTX_CHECK(gray && gh == S.gh && gw == S.gw, "gmc orb: gray image is %dx%d, expected %dx%d", gw, gh, S.gw, S.gh);
  S.submit(gray, Impl::kGrayDev);
}

void FeatGmc::submit_gray(const uint8_t* gray_host, int gh, int gw) {
  Impl& S = *impl_;
  GTX_CHECK(gray_host && gh == S.gh && gw == S.gw, "gmc orb: gray image is %dx%d, expected %dx%d", gw, gh, S.gw, S.gh);
  S.submit(gray_host, Impl::kGrayHost);
}

void FeatGmc::submit_frame_dev(const void* frame_bgr_dptr, int h, int w, bool restart) {
  Impl& S = *impl_;
  GTX_CHECK(frame_bgr_dptr && h == S.fh && w == S.fw, "gmc orb: frame is %dx%d, created for %dx%d", w, h, S.fw, S.fh);
  if (restart) S.have_prev = false;
  S.submit(frame_bgr_dptr, Impl::kFrameDev);
}

void FeatGmc::collect(double A[6], int* valid, int stats[3]) {
  Impl& S = *impl_;
  GTX_CHECK(S.pending() > 0, "gmc orb: collect without a submitted frame");
  GTX_HIP(hipSetDevice(S.ctx->device));
  const int slot = (int)(S.collected.load(std::memory_order_relaxed) % Impl::kRing);
  GTX_HIP(hipEventSynchronize(S.done[slot]));
  const double I6[6] = {1, 0, 0, 0, 1, 0};
  std::memcpy(A, I6, sizeof I6);
  if (valid) *valid = 0;
  int st3[3] = {0, 0, 0};
  if (!S.first[slot]) {
    const GmcResult& R = S.h_res[slot];
    st3[0] = R.n_prev; st3[1] = R.n_valid;
    int n_inl = 0;
    if (gmc_refit(R, S.h_pairs + (size_t)slot * kMaxFeat, 1.0, A, &n_inl)) {    // the pairs are in full-resolution pixels already
      st3[2] = n_inl;
      if (valid) *valid = 1;
    }
  }
  if (stats) std::memcpy(stats, st3, sizeof st3);
  S.last_slot = slot;                                    // debug_pairs reads it while nothing newer is in flight
  S.collected.fetch_add(1, std::memory_order_release);
}

void FeatGmc::debug_pairs(int cap, int* n, float* pairs4) const {
  const Impl& S = *impl_;
  *n = 0;
  GTX_CHECK(S.pending() == 0, "gmc orb: debug read while a frame is in flight");
  if (S.last_slot < 0 || S.first[S.last_slot]) return;
  const int k = std::min(cap, S.h_res[S.last_slot].n_valid);
  *n = k;
  if (k > 0 && pairs4) std::memcpy(pairs4, S.h_pairs + (size_t)S.last_slot * kMaxFeat, sizeof(float4) * k);
}

void FeatGmc::debug_matches(int cap, int* n_q, int* n_t, int* best_idx, int* best_d, int* second_d, float* q_xy, float* t_xy) const {
  const Impl& S = *impl_;
  GTX_CHECK(S.pending() == 0, "gmc orb: debug read while a frame is in flight");
  *n_q = *n_t = 0;
  if (S.last_first || S.last_slot < 0) return;
  GTX_HIP(hipSetDevice(S.ctx->device));
  GTX_HIP(hipStreamSynchronize(S.ctx->stream));
  // the sets changed roles at the end of the submit: the last frame's is now the reference
  const Stabilizer::FeatureSet q = S.st->feature_set(0), t = S.st->feature_set(1);
  const Stabilizer::RawMatches m = S.st->raw_matches();
  int nq = 0, nt = 0;
  GTX_HIP(hipMemcpy(&nq, q.n, sizeof(int), hipMemcpyDeviceToHost));
  GTX_HIP(hipMemcpy(&nt, t.n, sizeof(int), hipMemcpyDeviceToHost));
  *n_q = nq = std::min(nq, cap); *n_t = nt = std::min(nt, cap);
  if (nq > 0) {
    if (best_idx) GTX_HIP(hipMemcpy(best_idx, m.best_idx, sizeof(int) * nq, hipMemcpyDeviceToHost));
    if (best_d) GTX_HIP(hipMemcpy(best_d, m.best_d, sizeof(int) * nq, hipMemcpyDeviceToHost));
    if (second_d) GTX_HIP(hipMemcpy(second_d, m.second_d, sizeof(int) * nq, hipMemcpyDeviceToHost));
    if (q_xy) GTX_HIP(hipMemcpy(q_xy, q.xy, sizeof(float2) * nq, hipMemcpyDeviceToHost));
  }
  if (nt > 0 && t_xy) GTX_HIP(hipMemcpy(t_xy, t.xy, sizeof(float2) * nt, hipMemcpyDeviceToHost));
}

}  // namespace gtx
