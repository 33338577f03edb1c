// Host-only driver for the sanitizer builds (make -C geo-trax_amd asan | tsan): the tracker and the projective-geometry
// helpers are the parts of libgtx that run on the host inside the hot loop (the reference has no
// sanitizer story; a multi-threaded, multi-stream build should own one). GPU AddressSanitizer is not available on this
// pool, so the HIP kernels are out of reach of this target; the C++ that manages tracks, lists and the LAP is not.
//   asan: one long seeded detection stream through ByteTrack and BoT-SORT (births, deaths, empty frames, dense overlaps,
//         >1000 removed tracks so that the ring of removed ids wraps), box warps and point transforms on edge inputs.
//   tsan: the same streams on several tracker objects from several threads at once (objects are independent; the library
//         promises nothing shared between them).
//   both: the result-file writers, whose worker threads format chunks and pass the file to each other in row order.
#include <cmath>
#include <cstdio>
#include <random>
#include <thread>
#include <vector>

#include <cstdint>
#include <string>

#include "../../../include/gtx.h"
#include "../geometry.hpp"
#include "../homography.hpp"
#include "../tracker.hpp"
#include "../vec_acos.hpp"
#include "../yolo_tables.hpp"

namespace {
struct Frame { std::vector<float> xyxy, conf; std::vector<int> cls; };

std::vector<Frame> stream(unsigned seed, int n_obj, int n_frames, float w, float h) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  std::vector<float> px(n_obj), py(n_obj), vx(n_obj), vy(n_obj), sw(n_obj), sh(n_obj), cf(n_obj);
  for (int k = 0; k < n_obj; ++k) {
    px[k] = 50 + U(rng) * (w - 100); py[k] = 50 + U(rng) * (h - 100); vx[k] = (U(rng) - 0.5f) * 12; vy[k] = (U(rng) - 0.5f) * 12;
    sw[k] = 40 + U(rng) * 120; sh[k] = 25 + U(rng) * 45; cf[k] = 0.3f + U(rng) * 0.65f;
  }
  std::vector<Frame> out(n_frames);
  for (int t = 0; t < n_frames; ++t) {
    if (t % 37 == 17) continue;                       // an empty frame now and then
    for (int k = 0; k < n_obj; ++k) {
      if (U(rng) < 0.1f) continue;
      if ((t + k) % 61 == 0) { px[k] = 50 + U(rng) * (w - 100); py[k] = 50 + U(rng) * (h - 100); }   // teleport: old track dies, new one is born
      const float cx = px[k] + vx[k] * (t % 40), cy = py[k] + vy[k] * (t % 40);
      out[t].xyxy.insert(out[t].xyxy.end(), {cx - sw[k] / 2, cy - sh[k] / 2, cx + sw[k] / 2, cy + sh[k] / 2});
      out[t].conf.push_back(U(rng) < 0.1f ? 0.12f + 0.1f * U(rng) : cf[k]);
      out[t].cls.push_back(k % 4);
    }
  }
  return out;
}

long run_tracker(int type, unsigned seed) {
  gtx_tracker_config cfg{};
  cfg.type = type; cfg.track_high_thresh = 0.25f; cfg.track_low_thresh = 0.1f; cfg.new_track_thresh = 0.25f; cfg.track_buffer = 30;
  cfg.match_thresh = 0.8f; cfg.fuse_score = 1; cfg.frame_rate = 30;
  gtx::ByteTracker trk(cfg);
  const int cap = 512;
  std::vector<float> ob(cap * 4), os(cap);
  std::vector<int> oi(cap), oc(cap), od(cap);
  long rows = 0;
  for (int rep = 0; rep < 2; ++rep) {
    for (const Frame& f : stream(seed, rep ? 150 : 60, 400, rep ? 900.f : 3840.f, rep ? 600.f : 2160.f)) {   // second pass: dense overlaps
      const double warp[6] = {1.0, 1e-4, 0.3, -1e-4, 1.0, -0.2};
      int n = 0;
      trk.update((int)f.conf.size(), f.xyxy.data(), f.conf.data(), f.cls.data(), type == 1 ? warp : nullptr, cap, &n, ob.data(), oi.data(),
                 os.data(), oc.data(), od.data());
      rows += n;
    }
    if (rep == 0) trk.reset();
  }
  return rows;
}

// Round 6: the trackers with an appearance branch (Deep OC-SORT, TrackTrack; BoT-SORT's is in run_tracker's type 1 when feats are
// handed in) on the same streams with one seeded vector per detection, a camera warp, and the partial-affine fit of the feature GMC.
template <class Tracker>
long run_reid_tracker(int type, unsigned seed) {
  gtx_tracker_config cfg{};
  cfg.type = type; cfg.track_high_thresh = 0.3f; cfg.track_low_thresh = 0.1f; cfg.new_track_thresh = 0.3f; cfg.track_buffer = 30;
  cfg.match_thresh = 0.8f; cfg.fuse_score = 1; cfg.frame_rate = 30; cfg.delta_t = 3; cfg.inertia = 0.2f; cfg.min_hits = 3;
  cfg.with_reid = 1; cfg.proximity_thresh = 0.3f; cfg.appearance_thresh = 0.5f; cfg.alpha_fixed_emb = 0.9f;
  cfg.iou_weight = 0.5f; cfg.reid_weight = 0.5f; cfg.conf_weight = 0.1f; cfg.angle_weight = 0.05f; cfg.penalty_p = 0.2f; cfg.penalty_q = 0.4f;
  cfg.reduce_step = 0.05f; cfg.tai_thr = 0.55f; cfg.min_track_len = 3; cfg.lost_match_thr = 0.9f;
  Tracker trk(cfg);
  const int cap = 512, dim = 24;
  std::vector<float> ob(cap * 4), os(cap);
  std::vector<int> oi(cap), oc(cap), od(cap);
  std::mt19937 rng(seed * 7 + 1);
  std::normal_distribution<float> N(0.f, 1.f);
  long rows = 0;
  for (const Frame& f : stream(seed, 80, 300, 1920.f, 1080.f)) {
    const int n_det = (int)f.conf.size();
    std::vector<float> feats((size_t)n_det * dim);
    for (int i = 0; i < n_det; ++i)
      for (int k = 0; k < dim; ++k) feats[(size_t)i * dim + k] = (float)((f.cls[i] + 1) * ((k % 5) - 2)) + 0.4f * N(rng);
    const double warp[6] = {1.0, 2e-4, 0.5, -2e-4, 1.0, -0.3};
    int n = 0;
    trk.update(n_det, f.xyxy.data(), f.conf.data(), f.cls.data(), warp, cap, &n, ob.data(), oi.data(), os.data(), oc.data(), od.data(),
               n_det ? feats.data() : nullptr, dim);
    rows += n;
  }
  return rows;
}

// vec_acos.hpp against libm over the whole argument range, the range borders and the neighbourhoods of +-1 (where acos is
// steepest): at most 2 ulp of pi apart, 0 and pi exactly at the ends.
bool run_acos_check(unsigned seed) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  const int n = 1 << 18;
  std::vector<double> x(n), y(n);
  for (int i = 0; i < n; ++i) x[i] = U(g);
  const double edge[] = {1.0, -1.0, 0.0, -0.0, 0.5, -0.5, 0.49999999999999994, -0.49999999999999994, 1.0 - 1e-16, -1.0 + 1e-16, 1e-300, -1e-300};
  int k = 0;
  for (double e : edge) x[k++] = e;
  for (int i = 0; i < 4000; ++i) { x[k++] = std::cos(i * 1e-9); x[k++] = -std::cos(i * 1e-9); }
  gtx::acos_block(x.data(), y.data(), n);
  if (y[0] != 0.0 || y[1] != M_PI) return false;
  for (int i = 0; i < n; ++i)
    if (!(std::fabs(y[i] - std::acos(x[i])) <= 9e-16)) { std::fprintf(stderr, "acos_block(%.17g) = %.17g, libm %.17g\n", x[i], y[i], std::acos(x[i])); return false; }
  return true;
}

bool run_affine_fit(unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> U(0.f, 1000.f);
  for (int n : {0, 1, 2, 5, 400}) {
    std::vector<float> p((size_t)2 * n), q((size_t)2 * n);
    for (int i = 0; i < n; ++i) {
      p[2 * i] = U(rng); p[2 * i + 1] = U(rng);
      q[2 * i] = 1.001f * p[2 * i] - 0.002f * p[2 * i + 1] + 3.f + (i % 4 == 0 ? U(rng) * 0.3f : 0.f);     // a quarter of the pairs are outliers
      q[2 * i + 1] = 0.002f * p[2 * i] + 1.001f * p[2 * i + 1] - 2.f;
    }
    double A[6];
    int inl = 0;
    const bool ok = gtx::estimate_affine_partial(p.data(), q.data(), n, seed, A, &inl);
    if (n >= 5 && (!ok || std::fabs(A[0] - 1.001) > 0.01 || inl < n / 2)) return false;
    if (n < 2 && ok) return false;
  }
  return true;
}

// The robust homography's host refit (homography_refit.cpp) on seeded pairs of a 1920x1080 frame: every size around the minimal
// sets, projective and affine, about 30 % gross outliers, a winner nowhere near the pairs (no support: false) and n identical
// pairs (a singular normal matrix: the Cholesky step must bail out). Only what must hold is asserted: false leaves H alone, true
// gives finite entries with h33 = 1. (h33 leaves the refit as x * (1 / x): exactly 1 for every case of the seed main() passes, one
// ulp below 1 for some cases of other seeds -- 1, 2, 4, 5, 6, 8, 11 of the first twelve. Change the seed and that comparison with it.)
bool run_homography_refit(unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  std::normal_distribution<float> N(0.f, 0.3f);
  const int w = 1920, h = 1080;
  auto check = [&](const std::vector<float>& pairs, int n, bool affine, const double* H0, int want) {   // want: 1 true, 0 false, -1 either
    double H[9];
    for (double& v : H) v = 7.0;
    int inl = -1;
    const bool ok = gtx::refine_homography(pairs.data(), n, w, h, 2.0, affine, H0, H, &inl);
    if (want >= 0 && ok != (want == 1)) return false;
    for (double v : H)
      if (ok ? !std::isfinite(v) : v != 7.0) return false;
    return !ok || (H[8] == 1.0 && inl >= (affine ? 3 : 4) && inl <= n);
  };
  for (int affine = 0; affine < 2; ++affine) {
    const double p6 = affine ? 0.0 : 2e-6, p7 = affine ? 0.0 : -1e-6;
    const double Ht[9] = {1.002, -0.01, 12.5, 0.01, 1.002, -7.25, p6, p7, 1.0};
    double H0[9], Hfar[9];                              // the winner as a kernel leaves it: close to the truth, any scale
    for (int k = 0; k < 9; ++k) { H0[k] = 2.0 * Ht[k]; Hfar[k] = Ht[k]; }
    H0[2] += 1.0; Hfar[2] += 500.0;
    for (int n : {0, 3, 4, 5, 60, 800}) {
      std::vector<float> pairs((size_t)4 * n);
      for (int i = 0; i < n; ++i) {
        const double x = U(rng) * w, y = U(rng) * h, d = Ht[6] * x + Ht[7] * y + 1.0;
        pairs[4 * i] = (float)x; pairs[4 * i + 1] = (float)y;
        pairs[4 * i + 2] = (float)((Ht[0] * x + Ht[1] * y + Ht[2]) / d) + N(rng);
        pairs[4 * i + 3] = (float)((Ht[3] * x + Ht[4] * y + Ht[5]) / d) + N(rng);
        if (n >= 60 && U(rng) < 0.3f) { pairs[4 * i + 2] += (U(rng) - 0.5f) * 400.f; pairs[4 * i + 3] += (U(rng) - 0.5f) * 400.f; }
      }
      if (!check(pairs, n, affine != 0, H0, n < (affine ? 3 : 4) ? 0 : (n >= 60 ? 1 : -1))) return false;
      if (n == 60 && !check(pairs, n, affine != 0, Hfar, 0)) return false;                    // under-supported
      if (n == 60) {                                                                           // n identical pairs, on the model
        const double x = 700.0, y = 400.0, d = Ht[6] * x + Ht[7] * y + 1.0;
        const float one[4] = {(float)x, (float)y, (float)((Ht[0] * x + Ht[1] * y + Ht[2]) / d), (float)((Ht[3] * x + Ht[4] * y + Ht[5]) / d)};
        for (int i = 0; i < n; ++i)
          for (int k = 0; k < 4; ++k) pairs[4 * i + k] = one[k];
        if (!check(pairs, n, affine != 0, H0, 1)) return false;                               // the winner comes back, normalised
      }
    }
  }
  return true;
}
}  // namespace

// The result-file writers (table_writer.cpp): several chunks per call so that their own threads hand the file to each other in
// order, awkward values, a categorical column with missing cells; the anchor walk over ragged tracks incl. an empty one.
bool run_writers(unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> U(-4000.f, 4000.f);
  const int64_t rows = 40000;
  std::vector<float> t((size_t)rows * 12);
  for (float& v : t) v = U(rng);
  t[5] = NAN; t[17] = INFINITY; t[29] = -0.0f; t[41] = 1e-38f;
  const std::string base = "/tmp/gtx_sanitize_" + std::to_string(seed);
  if (gtx_write_table_f32((base + ".txt").c_str(), t.data(), rows, 12, 6, 4) != GTX_OK) return false;
  std::vector<double> d(t.begin(), t.begin() + 9 * 1000);
  if (gtx_write_table_f64((base + "_h.txt").c_str(), d.data(), 1000, 9, 20, 3) != GTX_OK) return false;
  std::vector<int64_t> ids((size_t)rows);
  std::vector<double> val((size_t)rows);
  std::vector<int32_t> code((size_t)rows);
  for (int64_t i = 0; i < rows; ++i) { ids[i] = i / 7 - 3; val[i] = i % 11 ? (double)t[i] * 1e-3 : (double)NAN; code[i] = (int32_t)(i % 4) - 1; }
  const char* labels[3] = {"A", "\"B,1\"", ""};
  const int kinds[3] = {0, 1, 2};
  const void* cols[3] = {ids.data(), val.data(), code.data()};
  const char* const* cats[3] = {nullptr, nullptr, labels};
  const int ncat[3] = {0, 0, 3};
  if (gtx_write_csv((base + ".csv").c_str(), "Vehicle_ID,Value,Section", 3, kinds, cols, cats, ncat, rows, 4) != GTX_OK) return false;
  if (gtx_write_csv("/no/such/dir/x.csv", "a,b,c", 3, kinds, cols, cats, ncat, rows, 2) == GTX_OK) return false;   // the error path closes nothing twice
  std::vector<int64_t> start = {0, 0, 1, 300, 2000, 2001, (int64_t)rows};
  std::vector<uint8_t> anchor((size_t)rows, 7);
  std::vector<float> dx((size_t)rows), dy((size_t)rows);
  if (gtx_track_anchor_walk(t.data(), t.data() + rows, start.data(), (int)start.size() - 1, 45.87156f, anchor.data(), dx.data(), dy.data()) != GTX_OK) return false;
  std::remove((base + ".txt").c_str()); std::remove((base + "_h.txt").c_str()); std::remove((base + ".csv").c_str());
  return anchor[0] == 0 && anchor[1] <= 1;
}

// The YOLO trunks' layer tables are walkable (yolov10.yaml's, yolo26.yaml's and yolo12.yaml's among them), a broken one is caught at its row, and the depthwise
// weight transposition touches exactly its taps x channels values (odd sizes: 7x7 on 24 channels, 3x3 on 8, 5x5 on 40); the depthwise and
// attention launchers' kernel names follow their dispatch predicates
static bool run_trunk_tables() {
  using namespace gtx;
  using namespace gtx::tables;
  const struct { const TrunkRow* rows; int n; } all[] = {{kYolov8, (int)(sizeof(kYolov8) / sizeof(TrunkRow))}, {kYolov8P2, (int)(sizeof(kYolov8P2) / sizeof(TrunkRow))},
                                                          {kYolo11, (int)(sizeof(kYolo11) / sizeof(TrunkRow))}, {kYolo10, (int)(sizeof(kYolo10) / sizeof(TrunkRow))},
                                                          {kYolo11Cls, (int)(sizeof(kYolo11Cls) / sizeof(TrunkRow))}, {kYolov8, kClsBackboneRows},
                                                          {kYolo26, (int)(sizeof(kYolo26) / sizeof(TrunkRow))}, {kYolo12, (int)(sizeof(kYolo12) / sizeof(TrunkRow))}};
  for (const auto& t : all)
    if (trunk_table_error(t.rows, t.n) >= 0) return false;
  int scdown = 0, psa = 0;
  for (const TrunkRow& r : kYolo10) { scdown += r.mod == TrunkRow::SCDOWN; psa += r.mod == TrunkRow::PSA; }
  if (scdown != 3 || psa != 1 || kYolo10[23].mod != TrunkRow::DETECT) return false;
  // yolo26.yaml: kYolo11's modules row for row; its SPPF row alone carries the linear-cv1 + residual flag
  for (int i = 0; i < 24; ++i)
    if (kYolo26[i].mod != kYolo11[i].mod || (kYolo26[i].mod == TrunkRow::SPPF) != (i == 9) || (i == 9 && (!kYolo26[i].shortcut || kYolo11[i].shortcut))) return false;
  // yolo12.yaml: 22 rows, five A2C2f blocks of which the two in the backbone carry an area (4 at stride 16, 1 at stride 32), Detect last;
  // a map cuts into its areas exactly when its positions are a multiple of them
  int a2 = 0;
  for (const TrunkRow& r : kYolo12) a2 += r.mod == TrunkRow::A2C2F;
  if (sizeof(kYolo12) / sizeof(TrunkRow) != 22 || a2 != 5 || kYolo12[6].area != 4 || kYolo12[8].area != 1 || kYolo12[11].area != 0 || kYolo12[21].mod != TrunkRow::DETECT) return false;
  for (const auto& t : all)
    for (int i = 0; i < t.n; ++i)
      if (t.rows != kYolo12 && t.rows[i].area != 0) return false;
  for (int h = 1; h <= 12; ++h)
    for (int w = 1; w <= 12; ++w)
      for (int area = 0; area <= 5; ++area)
        if (area_attention_fits(h, w, area) != (area > 0 && h * w % area == 0)) return false;
  std::vector<TrunkRow> bad12(kYolo12, kYolo12 + 22);
  bad12[10].from[1] = 11;                             // yolo12.yaml's first Concat reading a later layer
  if (trunk_table_error(bad12.data(), 22) != 10) return false;
  // yolov5.yaml: 25 rows, eight C3 blocks (shortcut on in the backbone only), the neck's 1x1 Convs at 10 / 14 each feed one Concat (22 / 19)
  // besides their Upsample, Detect last on 17 / 20 / 23; the 6x6 / 2 / pad 2 stem's output side, odd sides and the smallest one included
  constexpr int n5 = (int)(sizeof(kYolov5u) / sizeof(TrunkRow));
  int c3 = 0;
  for (const TrunkRow& r : kYolov5u) c3 += r.mod == TrunkRow::C3 && r.shortcut == (r.i < 9) && r.area == 0;
  if (n5 != 25 || trunk_table_error(kYolov5u, n5) >= 0 || c3 != 8 || kYolov5u[24].mod != TrunkRow::DETECT || kYolov5u[24].from[0] != 17 ||
      kYolov5u[24].from[1] != 20 || kYolov5u[24].from[2] != 23 || kYolov5u[22].from[1] != 10 || kYolov5u[19].from[1] != 14)
    return false;
  std::vector<TrunkRow> bad5(kYolov5u, kYolov5u + n5);
  bad5[19].from[1] = 10;                              // model.10 in two Concats
  if (trunk_table_error(bad5.data(), n5) != 22) return false;
  for (int n = 2; n <= 40; ++n)
    if (stem6_out(n) != (n + 2 * 2 - 6) / 2 + 1 || 2 * (stem6_out(n) - 1) - 2 + 5 > n + 1 || 2 * stem6_out(n) - 2 + 5 <= n + 1) return false;
  std::vector<TrunkRow> bad(kYolo10, kYolo10 + 24);
  bad[12].from[1] = 13;                               // a Concat that reads a later layer
  if (trunk_table_error(bad.data(), 24) != 12) return false;
  bad.assign(kYolo10, kYolo10 + 24);
  bad[21].from[1] = 6;                                // model.6 in two Concats
  if (trunk_table_error(bad.data(), 24) != 21) return false;
  // the kernel names the graph builders label their ops with: <3>, <5> and <7> forms, tiled exactly at stride 1 on whole 32-channel groups
  for (int k : {3, 5, 7})
    for (int stride : {1, 2})
      for (int c : {8, 24, 32, 40, 64, 96}) {
        const bool tiled = stride == 1 && c % 32 == 0;
        const std::string want = std::string(tiled ? "rt_dwconv_tile_kernel<" : "rt_dwconv_kernel<") + std::to_string(k) + ">";
        if (rt_dwconv_tiled(stride, c) != tiled || want != rt_dwconv_kernel_name(k, stride, c)) return false;
      }
  for (int h = 1; h <= 12; ++h)
    for (int w = 1; w <= 12; ++w) {
      if (psa_attention_small(h, w) != (h * w <= 64)) return false;
      if (std::string(psa_attention_kernel_name(h, w)) != (psa_attention_small(h, w) ? "psa_attn_small_kernel" : "psa_attn_kernel")) return false;
    }
  const int sizes[3][2] = {{24, 49}, {8, 9}, {40, 25}};   // {40, 25}: rtdetr-l's LightConv 5x5
  for (const auto& ck : sizes) {
    const int c = ck[0], taps = ck[1];
    std::vector<float> w((size_t)c * taps);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)i;
    const std::vector<float> wt = dw_tap_major(w.data(), c, taps);
    if (wt.size() != w.size()) return false;
    for (int ch = 0; ch < c; ++ch)
      for (int t = 0; t < taps; ++t)
        if (wt[(size_t)t * c + ch] != (float)(ch * taps + t)) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  const bool threads = argc > 1 && argv[1][0] == 't';
  long rows = 0;
  if (!run_writers(threads ? 2 : 1)) { std::fprintf(stderr, "result-file writers failed\n"); return 3; }
  if (!run_trunk_tables()) { std::fprintf(stderr, "trunk layer tables / depthwise packing wrong\n"); return 6; }
  if (threads) {
    std::vector<long> r(6);
    std::vector<std::thread> th;
    for (int i = 0; i < 6; ++i)
      th.emplace_back([&r, i] {
        r[i] = i < 4 ? run_tracker(i & 1, 100 + i) : (i == 4 ? run_reid_tracker<gtx::OcSortTracker>(3, 104) : run_reid_tracker<gtx::TrackTrackTracker>(5, 105));
      });
    bool refit[2] = {false, false};                    // the refit shares nothing between calls: two at once
    for (int i = 0; i < 2; ++i) th.emplace_back([&refit, i] { refit[i] = run_homography_refit(7); });
    for (auto& t : th) t.join();
    for (long v : r) rows += v;
    if (!refit[0] || !refit[1]) { std::fprintf(stderr, "homography refit wrong\n"); return 7; }
  } else {
    rows = run_tracker(0, 1) + run_tracker(1, 2);
    rows += run_reid_tracker<gtx::OcSortTracker>(3, 3) + run_reid_tracker<gtx::TrackTrackTracker>(5, 4);
    if (!run_affine_fit(5)) { std::fprintf(stderr, "partial-affine fit wrong\n"); return 4; }
    if (!run_homography_refit(7)) { std::fprintf(stderr, "homography refit wrong\n"); return 7; }
    if (!run_acos_check(6)) { std::fprintf(stderr, "vector acos differs from libm\n"); return 5; }
    // geometry helpers on edge inputs: zero boxes, a point on the line at infinity, a degenerate matrix
    const double H[9] = {1.01, 0.002, 3.0, -0.001, 0.99, -6.0, 1e-7, -1e-7, 1.0};
    std::vector<float> in = {100, 200, 50, 20, 3800, 2100, 90, 40}, outb(8);
    gtx::warp_boxes(H, in.data(), 2, outb.data());
    gtx::warp_boxes(H, in.data(), 0, outb.data());
    const double Hinf[9] = {1, 0, 0, 0, 1, 0, 1, 0, -5};
    double x[2] = {5.0, 1.0}, y[2] = {7.0, 2.0}, ox[2], oy[2];
    gtx::perspective_points(Hinf, x, y, 2, ox, oy);
    if (!(ox[0] == 0.0 && oy[0] == 0.0) || !std::isfinite(outb[0])) { std::fprintf(stderr, "geometry edge cases wrong\n"); return 2; }
  }
  std::printf("sanitize_host ok: %ld track rows\n", rows);
  return rows > 10000 ? 0 : 1;
}
