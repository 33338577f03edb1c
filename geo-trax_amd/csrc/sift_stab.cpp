#include "sift_stab.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "homography.hpp"
#include "match_l2.hpp"
#include "net_runtime.hpp"   // gtx_ctx
#include "sift.hpp"

namespace gtx {

namespace {
// What a frame in flight leaves in pinned memory for collect: the RANSAC record, the extraction's counters, the pair list.
constexpr size_t kRecordRoom = 256;
}  // namespace

struct SiftStab::Impl {
  gtx_ctx* ctx;
  gtx_sift_stab_config cfg;
  int gh, gw, k_cur, k_ref, n_hyp;
  bool root;
  std::unique_ptr<Sift> sift;
  // the reference set, extracted once
  DevBuf ref_desc, ref_half, ref_xy, ref_kps;
  int n_ref = 0;
  bool have_ref = false;
  // the frame in flight
  DevBuf cur_half, ws, i1, i2, d1, d2, pts, n_pairs, rstate, record, rects;
  int4* h_rects = nullptr;          // pinned
  char* h_out = nullptr;            // pinned: [record kRecordRoom][counters 4 x i32][pairs k_cur x float4]
  hipEvent_t t0 = nullptr, t1 = nullptr, done = nullptr;
  bool pending = false;
  float ms = 0.f;
  // the last collected frame
  int cnt[4] = {0, 0, 0, 0};
  int n_cur = 0;
  std::vector<float4> last_pairs;

  const int* h_counters() const { return reinterpret_cast<const int*>(h_out + kRecordRoom); }
  const float4* h_pts() const { return reinterpret_cast<const float4*>(h_out + kRecordRoom + 16); }

  // oracle/stabilo_ref.py mask_rects, the rule of the ORB path: boxes grown by the margin, scaled to the working image, floor / ceil,
  // clipped, inclusive
  int build_rects(const float* boxes, int n) {
    if (!cfg.mask_use || !boxes || n <= 0) return 0;
    const float r = cfg.downsample_ratio, m = cfg.mask_margin_ratio;
    const int room = sift_select_max_rects();
    int k = 0;
    for (int i = 0; i < n && k < room; ++i) {
      const float cx = boxes[4 * i], cy = boxes[4 * i + 1], w = boxes[4 * i + 2] * (1.f + m), h = boxes[4 * i + 3] * (1.f + m);
      int x1 = (int)std::floor((cx - w / 2) * r), y1 = (int)std::floor((cy - h / 2) * r);
      int x2 = (int)std::ceil((cx + w / 2) * r), y2 = (int)std::ceil((cy + h / 2) * r);
      x1 = std::max(x1, 0); y1 = std::max(y1, 0); x2 = std::min(x2, gw - 1); y2 = std::min(y2, gh - 1);
      if (x2 >= x1 && y2 >= y1) h_rects[k++] = make_int4(x1, y1, x2, y2);
    }
    if (k > 0) GTX_HIP(hipMemcpyAsync(rects.p, h_rects, sizeof(int4) * (size_t)k, hipMemcpyHostToDevice, ctx->stream));
    return k;
  }
};

SiftStab::SiftStab(gtx_ctx* ctx, const gtx_sift_stab_config& cfg) : impl_(new Impl) {
  Impl& S = *impl_;
  S.ctx = ctx; S.cfg = cfg;
  S.gh = cfg.work_h; S.gw = cfg.work_w;
  GTX_CHECK(S.gh >= 8 && S.gw >= 8, "sift stabilizer: working image %dx%d too small", S.gw, S.gh);
  GTX_CHECK(cfg.max_features >= 1, "sift stabilizer: max_features=%d", cfg.max_features);
  GTX_CHECK(cfg.ref_multiplier >= 1.f / cfg.max_features && cfg.ref_multiplier <= 64.f, "sift stabilizer: ref_multiplier=%g", cfg.ref_multiplier);
  GTX_CHECK(cfg.filter_ratio > 0.f && cfg.filter_ratio <= 1.f, "sift stabilizer: filter_ratio=%g outside (0,1]", cfg.filter_ratio);
  GTX_CHECK(cfg.ransac_threshold > 0.f, "sift stabilizer: ransac threshold must be positive");
  GTX_CHECK(cfg.downsample_ratio > 0.f && cfg.downsample_ratio <= 1.f, "sift stabilizer: downsample_ratio=%g outside (0,1]", cfg.downsample_ratio);
  S.k_cur = cfg.max_features;
  S.k_ref = std::max(1, (int)std::lround(cfg.max_features * (double)cfg.ref_multiplier));      // the ORB plan's reference count
  const int k_max = std::max(S.k_cur, S.k_ref);
  GTX_CHECK(k_max <= sift_select_max_features(), "sift stabilizer: %d keypoints a set, at most %d", k_max, sift_select_max_features());
  S.n_hyp = std::max(256, std::min(cfg.ransac_max_iter, 16384));
  S.root = cfg.root != 0;
  GTX_HIP(hipSetDevice(ctx->device));
  // one resident pyramid per object: refuse here, with the sizes, rather than run out of memory somewhere inside
  size_t free_b = 0, total_b = 0;
  GTX_HIP(hipMemGetInfo(&free_b, &total_b));
  const size_t need = Sift::resident_bytes(S.gh, S.gw) + (size_t)k_max * (128 * 4 * 2 + 128 * 2 * 2 + 256) + (64u << 20);
  GTX_CHECK(need <= free_b, "sift stabilizer: a %dx%d working image keeps %.2f GB in HBM (the Gaussian and DoG pyramids of the doubled image), %.2f GB are free",
            S.gw, S.gh, need / 1e9, free_b / 1e9);
  S.sift.reset(new Sift(ctx->device, ctx->stream, S.gh, S.gw));
  S.sift->reserve_async(k_max);
  const size_t kr = (size_t)S.k_ref, kc = (size_t)S.k_cur;
  S.ref_desc.alloc(kr * 128 * sizeof(float));
  S.ref_half.alloc(kr * 128 * 2);
  S.ref_xy.alloc(kr * sizeof(float2));
  S.ref_kps.alloc(kr * sizeof(SiftKeypoint));
  S.cur_half.alloc(kc * 128 * 2);
  S.ws.alloc(match2nn_workspace_bytes(S.k_cur, S.k_ref));       // the most splits any reference count up to k_ref takes
  for (DevBuf* b : {&S.i1, &S.i2, &S.d1, &S.d2}) b->alloc(kc * 4);
  S.pts.alloc(kc * sizeof(float4));
  S.n_pairs.alloc(sizeof(int));
  S.rstate.alloc(2 * sizeof(unsigned long long));
  GTX_CHECK(ransac_record_bytes() <= kRecordRoom, "sift stabilizer: the RANSAC record grew beyond %zu bytes", kRecordRoom);
  S.record.alloc(kRecordRoom);
  S.rects.alloc(sizeof(int4) * (size_t)sift_select_max_rects());
  GTX_HIP(hipMemset(S.pts.p, 0, S.pts.bytes));
  GTX_HIP(hipMemset(S.n_pairs.p, 0, sizeof(int)));
  ransac_arm(S.rstate.as<unsigned long long>(), ctx->stream);
  GTX_HIP(hipHostMalloc(reinterpret_cast<void**>(&S.h_rects), sizeof(int4) * (size_t)sift_select_max_rects(), hipHostMallocDefault));
  GTX_HIP(hipHostMalloc(reinterpret_cast<void**>(&S.h_out), kRecordRoom + 16 + kc * sizeof(float4), hipHostMallocDefault));
  GTX_HIP(hipEventCreate(&S.t0));
  GTX_HIP(hipEventCreate(&S.t1));
  GTX_HIP(hipEventCreateWithFlags(&S.done, hipEventBlockingSync | hipEventDisableTiming));
}

SiftStab::~SiftStab() {
  if (!impl_) return;
  Impl& S = *impl_;
  (void)hipSetDevice(S.ctx->device);
  (void)hipStreamSynchronize(S.ctx->stream);
  if (S.h_rects) (void)hipHostFree(S.h_rects);
  if (S.h_out) (void)hipHostFree(S.h_out);
  for (hipEvent_t e : {S.t0, S.t1, S.done})
    if (e) (void)hipEventDestroy(e);
}

void SiftStab::set_ref_gray_dev(const void* gray, int gh, int gw, const float* boxes_xywh, int n) {
  Impl& S = *impl_;
  GTX_CHECK(gh == S.gh && gw == S.gw, "sift stabilizer: gray image is %dx%d, expected %dx%d", gw, gh, S.gw, S.gh);
  GTX_CHECK(!S.pending, "sift stabilizer: a frame is in flight");
  GTX_HIP(hipSetDevice(S.ctx->device));
  hipStream_t s = S.ctx->stream;
  const int n_rects = S.build_rects(boxes_xywh, n);
  S.sift->extract_async(static_cast<const uint8_t*>(gray), gh, gw, S.k_ref, S.root, S.cfg.rsift_eps, S.rects.as<int4>(), n_rects);
  int c[4];
  GTX_HIP(hipMemcpyAsync(c, S.sift->counters_dev(), sizeof c, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipStreamSynchronize(s));
  S.have_ref = false;
  S.sift->check_counters(c, S.k_ref);
  S.n_ref = c[3];
  const size_t k = (size_t)S.n_ref;
  if (k > 0) {
    GTX_HIP(hipMemcpyAsync(S.ref_desc.p, S.sift->descriptors_dev(), k * 128 * sizeof(float), hipMemcpyDeviceToDevice, s));
    GTX_HIP(hipMemcpyAsync(S.ref_xy.p, S.sift->positions_dev(), k * sizeof(float2), hipMemcpyDeviceToDevice, s));
    GTX_HIP(hipMemcpyAsync(S.ref_kps.p, S.sift->keypoints_dev(), k * sizeof(SiftKeypoint), hipMemcpyDeviceToDevice, s));
    descriptors_to_half(S.ref_desc.as<float>(), S.ref_half.p, k * 128, s);
  }
  GTX_HIP(hipStreamSynchronize(s));
  S.have_ref = true;
}

void SiftStab::submit_gray_dev(const void* gray, int gh, int gw, const float* boxes_xywh, int n) {
  Impl& S = *impl_;
  if (!S.have_ref) fail(GTX_ERR_STATE, "sift stabilizer: a frame before set_ref_gray_dev");
  GTX_CHECK(!S.pending, "sift stabilizer: a frame is already in flight");
  GTX_CHECK(gh == S.gh && gw == S.gw, "sift stabilizer: gray image is %dx%d, expected %dx%d", gw, gh, S.gw, S.gh);
  GTX_HIP(hipSetDevice(S.ctx->device));
  hipStream_t s = S.ctx->stream;
  GTX_HIP(hipEventRecord(S.t0, s));
  const int n_rects = S.build_rects(boxes_xywh, n);
  S.sift->extract_async(static_cast<const uint8_t*>(gray), gh, gw, S.k_cur, S.root, S.cfg.rsift_eps, S.rects.as<int4>(), n_rects);
  const int* n_cur_dev = S.sift->counters_dev() + 3;
  if (S.n_ref >= 2) {
    // the query rows are launched at capacity: those past the count hold whatever an earlier frame left and reach nothing
    descriptors_to_half(S.sift->descriptors_dev(), S.cur_half.p, (size_t)S.k_cur * 128, s);
    match2nn(S.cur_half.p, S.sift->descriptors_dev(), S.k_cur, S.ref_half.p, S.ref_desc.as<float>(), S.n_ref, S.ws.p, S.i1.as<int>(), S.i2.as<int>(),
             S.d1.as<float>(), S.d2.as<float>(), s);
    ratio_pairs(S.i1.as<int>(), S.i2.as<int>(), S.d1.as<float>(), S.d2.as<float>(), n_cur_dev, S.k_cur, S.n_ref, S.cfg.filter_ratio,
                S.sift->positions_dev(), S.ref_xy.as<float2>(), S.pts.as<float4>(), S.n_pairs.as<int>(), s);
  } else {
    GTX_HIP(hipMemsetAsync(S.n_pairs.p, 0, sizeof(int), s));
  }
  ransac_submit(s, S.pts.as<float4>(), S.n_pairs.as<int>(), n_cur_dev, S.cfg.seed, S.n_hyp, S.gw, S.gh, S.cfg.ransac_threshold, 0,
                S.rstate.as<unsigned long long>(), S.record.p);
  GTX_HIP(hipMemcpyAsync(S.h_out, S.record.p, ransac_record_bytes(), hipMemcpyDeviceToHost, s));
  GTX_HIP(hipMemcpyAsync(S.h_out + kRecordRoom, S.sift->counters_dev(), 16, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipMemcpyAsync(S.h_out + kRecordRoom + 16, S.pts.p, sizeof(float4) * (size_t)S.k_cur, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipEventRecord(S.t1, s));
  GTX_HIP(hipEventRecord(S.done, s));
  S.pending = true;
}

void SiftStab::collect(double H[9], int* valid, int stats[4]) {
  Impl& S = *impl_;
  GTX_CHECK(S.pending, "sift stabilizer: collect without a submitted frame");
  GTX_HIP(hipSetDevice(S.ctx->device));
  GTX_HIP(hipEventSynchronize(S.done));
  S.pending = false;
  GTX_HIP(hipEventElapsedTime(&S.ms, S.t0, S.t1));
  std::memcpy(S.cnt, S.h_counters(), sizeof S.cnt);
  S.n_cur = 0;
  S.last_pairs.clear();
  S.sift->check_counters(S.cnt, S.k_cur);
  int n_pairs = 0, n_cur = 0;
  ransac_record_counts(S.h_out, &n_pairs, &n_cur);
  GTX_CHECK(n_cur == S.cnt[3] && n_pairs >= 0 && n_pairs <= n_cur, "sift stabilizer: %d pairs of %d keypoints (%d counted)", n_pairs, n_cur, S.cnt[3]);
  S.n_cur = n_cur;
  S.last_pairs.assign(S.h_pts(), S.h_pts() + n_pairs);
  double Hc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  int n_inl = 0, ok = 0;
  if (n_cur >= 1 && S.n_ref >= 2 && n_pairs >= 4 && ransac_finish(S.h_out, S.h_pts(), S.gw, S.gh, S.cfg.ransac_threshold, false, Hc, &n_inl)) ok = 1;
  if (!ok) n_inl = 0;
  if (H) std::memcpy(H, Hc, sizeof Hc);
  if (valid) *valid = ok;
  if (stats) { stats[0] = S.n_ref; stats[1] = n_cur; stats[2] = n_pairs; stats[3] = n_inl; }
}

float SiftStab::last_ms() const { return impl_->ms; }

void SiftStab::counters(int out[4]) const { std::memcpy(out, impl_->cnt, sizeof impl_->cnt); }

void SiftStab::keypoints(int which, int cap, int* n, float* kp5, int* octave, float* desc) {
  Impl& S = *impl_;
  GTX_CHECK(which == 0 || which == 1, "sift stabilizer: which must be 0 (reference) or 1 (current)");
  GTX_CHECK(!S.pending, "sift stabilizer: a frame is in flight");
  GTX_HIP(hipSetDevice(S.ctx->device));
  GTX_HIP(hipStreamSynchronize(S.ctx->stream));
  const int have = which == 0 ? (S.have_ref ? S.n_ref : 0) : S.n_cur;
  *n = have;
  const int m = std::min(std::max(cap, 0), have);
  if (m == 0) return;
  std::vector<SiftKeypoint> k(m);
  GTX_HIP(hipMemcpy(k.data(), which == 0 ? S.ref_kps.p : (const void*)S.sift->keypoints_dev(), sizeof(SiftKeypoint) * (size_t)m, hipMemcpyDeviceToHost));
  for (int i = 0; i < m; ++i) {
    if (kp5) { kp5[5 * i] = k[i].x; kp5[5 * i + 1] = k[i].y; kp5[5 * i + 2] = k[i].size; kp5[5 * i + 3] = k[i].angle; kp5[5 * i + 4] = k[i].response; }
    if (octave) octave[i] = k[i].octave;
  }
  if (desc) GTX_HIP(hipMemcpy(desc, which == 0 ? S.ref_desc.p : (const void*)S.sift->descriptors_dev(), sizeof(float) * 128 * (size_t)m, hipMemcpyDeviceToHost));
}

void SiftStab::pairs(int cap, int* n, float* pts) {
  Impl& S = *impl_;
  *n = (int)S.last_pairs.size();
  const int m = std::min(std::max(cap, 0), *n);
  if (m > 0 && pts) std::memcpy(pts, S.last_pairs.data(), sizeof(float4) * (size_t)m);
}

}  // namespace gtx
