// Embedder (reid.hpp): YOLOv8-cls or YOLO11-cls backbone over a batch of detection crops, pooled into one vector per crop, and its C ABI.
//
// What upstream does per frame (ultralytics >= 8.4.80, trackers/bot_sort.py ReID.__call__), and where it is done here:
//   crops = [save_one_box(det, img, save=False) for det in xywh2xyxy(dets[:, :4])]   -> reid_crop_box (host)
//   ClassificationPredictor.preprocess: classify_transforms(imgsz) on each crop         -> reid_resample_coeffs (host) + reid_crop_kernel
//   model(crops, embed=[len(model) - 2]): adaptive_avg_pool2d(model.8 output)           -> YoloTrunk's backbone rows + reid_pool_kernel
//     (yolo11-cls: model.9, the C2PSA output; its attention runs psa_attn_small_kernel on the crops' 2 x 2 to 8 x 8 maps)
// Choices restated from memory of the pinned upstream rather than pinned by a test against it (the resample is pinned against PIL):
//   - the box chain: Boxes.xywh in float32, then float64 (BOTSORT.init_track concatenates the boxes with np.arange), save_one_box's
//     gain 1.02 / pad 10 / .long() truncation and clip to the frame;
//   - the channel order the network sees (kNetChannelsBgr);
//   - the embedded layer: model.8, the last backbone layer of yolov8-cls (len(model) - 2 for a .pt checkpoint); model.9 of yolo11-cls.
#include "reid.hpp"
#include "api_guard.hpp"
#include "split_format.hpp"

#include <cmath>

namespace gtx {

// save_one_box(..., BGR=False) reverses the crop's channels and ClassificationPredictor.preprocess applies cv2.cvtColor(BGR2RGB)
// before the PIL transforms: reversed twice, the network's input channel 0 is the frame's B. reid_crop_kernel writes the
// frame's bytes in their own order into the stem's channel slots, which is that order.
constexpr bool kNetChannelsBgr = true;
static_assert(kNetChannelsBgr, "reid_crop_kernel writes slot c = frame byte c");

namespace {
constexpr int kPrecBits = 22;   // PIL PRECISION_BITS

// PIL Resample.c precompute_coeffs (bilinear filter, support 1) + normalize_coeffs_8bpc for output indices [first, first + S) of
// out_size: bounds [S][2] (xmin, count) and int coefficients [S][ksize] appended to pool. Returns ksize. Double arithmetic,
// one rounding per operation.
int reid_resample_coeffs(int in_size, int out_size, int first, int S, std::vector<int>& pool, int* boff, int* koff) {
#pragma clang fp contract(off)
  const double scale = (double)(float)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  *boff = (int)pool.size();
  pool.resize(pool.size() + 2 * (size_t)S);
  *koff = (int)pool.size();
  pool.resize(pool.size() + (size_t)S * ksize, 0);
  std::vector<double> k(ksize);
  for (int i = 0; i < S; ++i) {
    const int xx = first + i;
    const double center = 0.0 + (xx + 0.5) * scale;
    double ww = 0.0;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      const double wgt = t < 1.0 ? 1.0 - t : 0.0;
      k[x] = wgt;
      ww += wgt;
    }
    for (int x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (int x = 0; x < xmax; ++x)
      pool[*koff + (size_t)i * ksize + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << kPrecBits)) : (int)(0.5 + k[x] * (1 << kPrecBits));
    pool[*boff + 2 * i] = xmin;
    pool[*boff + 2 * i + 1] = xmax;
  }
  return ksize;
}

// torchvision CenterCrop: int(round((size - S) / 2.0)), Python's round (ties to even)
int center_offset(int size, int S) {
  const int d = size - S, k = d / 2;
  return (d % 2 == 0) ? k : ((k % 2 == 0) ? k : k + 1);
}

}  // namespace

void reid_crop_box(const float b[4], int h, int w, int out[4]) {
#pragma clang fp contract(off)
  // Boxes.xywh (float32)
  const float xc = (b[0] + b[2]) / 2.f, yc = (b[1] + b[3]) / 2.f, bw = b[2] - b[0], bh = b[3] - b[1];
  // ReID.__call__: xywh2xyxy, float64 from here on
  const double x1 = (double)xc - (double)bw / 2, x2 = (double)xc + (double)bw / 2;
  const double y1 = (double)yc - (double)bh / 2, y2 = (double)yc + (double)bh / 2;
  // save_one_box: xyxy2xywh, wh * gain + pad, xywh2xyxy, .long(), clip_boxes
  const double cx = (x1 + x2) / 2, cy = (y1 + y2) / 2;
  const double ww = (x2 - x1) * 1.02 + 10, hh = (y2 - y1) * 1.02 + 10;
  const long long q[4] = {(long long)(cx - ww / 2), (long long)(cy - hh / 2), (long long)(cx + ww / 2), (long long)(cy + hh / 2)};
  out[0] = (int)std::min<long long>(std::max<long long>(q[0], 0), w);
  out[1] = (int)std::min<long long>(std::max<long long>(q[1], 0), h);
  out[2] = (int)std::min<long long>(std::max<long long>(q[2], 0), w);
  out[3] = (int)std::min<long long>(std::max<long long>(q[3], 0), h);
}

Embedder::Embedder(gtx_ctx* ctx, int imgsz, int max_crops, bool fp32_split)
    : NetRuntime(ctx, fp32_split ? DT_F32S : DT_F32, 4, max_crops), S_(imgsz), trunk_(*this, ops_, DT_F32) {
  GTX_CHECK(imgsz >= 32 && imgsz <= 320 && imgsz % 32 == 0, "reid imgsz must be a multiple of 32 in [32, 320] (got %d)", imgsz);
  GTX_CHECK(max_crops >= 1, "max_crops must be positive");
  GTX_HIP(hipSetDevice(ctx->device));
  GTX_HIP(hipEventCreateWithFlags(&done_, wait_event_flags(false)));
}

Embedder::~Embedder() {
  if (pin_) (void)hipHostFree(pin_);
  if (h_emb_) (void)hipHostFree(h_emb_);
  if (done_) (void)hipEventDestroy(done_);
}

std::unique_ptr<NetRuntime> Embedder::make_exact() const {
  return std::unique_ptr<NetRuntime>(new Embedder(ctx_, S_, max_batch_, false));
}

// model.0-8 (yolov8-cls) or model.0-9 (yolo11-cls) through the trunk's walk (no fusion: fuse() is never called, so the stem gets no
// front-packed weights)
void Embedder::build_graph() {
  img_ = new_view(S_, S_, 1);                                  // [N][S][S] uchar4: 4 bytes per pixel
  img_.plain = true;
  alloc_sat_flag();
  last_ = trunk_.build(img_, trunk_.choose_cls_graph(), false).in[0];
  dim_ = last_.c;
}

void Embedder::finalize() {
  GTX_CHECK(!finalized_, "finalize called twice");
  GTX_HIP(hipSetDevice(ctx_->device));
  build_graph();
  drop_tensors_unless_fallback();
  set_batch(1);
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  finalized_ = true;
}

void Embedder::set_batch(int nb) {
  if (nb == cur_nb_) return;
  set_batch_ops(ops_, nb, 4, false);
  cur_nb_ = nb;
}

// Crop table + coefficients of the pass on the host, one copy to the device, then chunk by chunk of max_crops: crop kernel ->
// backbone -> pool into the vectors' rows. Everything on the context's stream, so the frames are read before anything the
// caller enqueues behind this call on that stream.
void Embedder::enqueue(int n) {
  hipStream_t s = ctx_->stream;
  const int H = cur_h_, W = cur_w_;
  h_crops_.clear();
  h_pool_.clear();
  int frame = 0, left = cur_counts_.empty() ? 0 : cur_counts_[0];
  for (int i = 0; i < n; ++i) {
    while (left == 0) left = cur_counts_[++frame];
    --left;
    int q[4];
    reid_crop_box(&cur_xyxy_[(size_t)i * 4], H, W, q);
    ReidCrop c{};
    c.frame = frame;
    c.x0 = q[0]; c.y0 = q[1]; c.cw = q[2] - q[0]; c.ch = q[3] - q[1];
    GTX_CHECK(c.cw > 0 && c.ch > 0, "box %d (%.1f %.1f %.1f %.1f) leaves an empty crop in a %dx%d frame", i, cur_xyxy_[i * 4], cur_xyxy_[i * 4 + 1],
              cur_xyxy_[i * 4 + 2], cur_xyxy_[i * 4 + 3], W, H);
    // torchvision Resize(S) on the PIL image: short side S, long side int(S * long / short)
    int rw, rh;
    if (c.cw <= c.ch) { rw = S_; rh = (int)((double)((long long)S_ * c.ch) / c.cw); }
    else { rh = S_; rw = (int)((double)((long long)S_ * c.cw) / c.ch); }
    c.kh = reid_resample_coeffs(c.cw, rw, center_offset(rw, S_), S_, h_pool_, &c.bh, &c.hoff);
    c.kv = reid_resample_coeffs(c.ch, rh, center_offset(rh, S_), S_, h_pool_, &c.bv, &c.voff);
    h_crops_.push_back(c);
  }
  const size_t crop_bytes = h_crops_.size() * sizeof(ReidCrop), pool_off = (crop_bytes + 255) / 256 * 256;
  const size_t bytes = pool_off + h_pool_.size() * sizeof(int);
  if (pin_bytes_ < bytes) {
    if (pin_) GTX_HIP(hipHostFree(pin_));
    pin_ = nullptr;
    GTX_HIP(hipHostMalloc(&pin_, bytes * 2));
    pin_bytes_ = bytes * 2;
  }
  if (d_params_.bytes < bytes) d_params_.alloc(bytes * 2);
  if (d_emb_.bytes < std::max<size_t>((size_t)n * dim_ * 4, 4)) d_emb_.alloc(std::max<size_t>((size_t)n * dim_ * 4 * 2, 256));
  if (h_emb_n_ < (size_t)n * dim_) {
    if (h_emb_) GTX_HIP(hipHostFree(h_emb_));
    h_emb_ = nullptr;
    h_emb_n_ = std::max<size_t>((size_t)n * dim_ * 2, 1);
    GTX_HIP(hipHostMalloc((void**)&h_emb_, h_emb_n_ * 4));
  }
  if (n == 0) return;                                         // zero crops: nothing is launched
  memcpy(pin_, h_crops_.data(), crop_bytes);
  memcpy((uint8_t*)pin_ + pool_off, h_pool_.data(), h_pool_.size() * sizeof(int));
  GTX_HIP(hipMemcpyAsync(d_params_.p, pin_, bytes, hipMemcpyHostToDevice, s));
  const ReidCrop* d_crops = d_params_.as<ReidCrop>();
  const int* d_pool = (const int*)((const uint8_t*)d_params_.p + pool_off);
  for (int c0 = 0; c0 < n; c0 += max_batch_) {
    const int k = std::min(max_batch_, n - c0);
    set_batch(k);
    launch_reid_crop((const uint8_t*)cur_frames_, H, W, d_crops + c0, d_pool, k, S_, img_.ptr, s);
    run_ops(k, s, nullptr);
    launch_reid_pool(last_.ptr, fmt_ == DT_F32S ? 1 : 0, k, last_.h * last_.w, last_.cstride, last_.coff, dim_,
                     d_emb_.as<float>() + (size_t)c0 * dim_, s);
    last_chunk_ = c0;
    last_chunk_n_ = k;
  }
  GTX_HIP(hipMemcpyAsync(h_emb_, d_emb_.p, (size_t)n * dim_ * 4, hipMemcpyDeviceToHost, s));
  if (sat_dev_) GTX_HIP(hipMemcpyAsync(h_sat_, sat_dev_, sizeof(int), hipMemcpyDeviceToHost, s));
}

void Embedder::submit_dev(const void* frames, int nb, int h, int w, const int* counts, const float* xyxy) {
  GTX_CHECK(finalized_, "embedder not finalized");
  GTX_CHECK(!in_flight_, "submit while a pass is in flight: call collect first");
  GTX_CHECK(nb >= 1 && h > 0 && w > 0, "bad frame batch %d x %dx%d", nb, w, h);
  GTX_HIP(hipSetDevice(ctx_->device));
  int n = 0;
  for (int b = 0; b < nb; ++b) {
    GTX_CHECK(counts[b] >= 0, "negative box count");
    n += counts[b];
  }
  GTX_CHECK(n == 0 || frames, "frames: NULL");
  cur_frames_ = frames; cur_h_ = h; cur_w_ = w;
  cur_counts_.assign(counts, counts + nb);
  cur_xyxy_.assign(xyxy, xyxy + (size_t)n * 4);
  n_flight_ = n;
  enqueue(n);
  GTX_HIP(hipEventRecord(done_, ctx_->stream));
  in_flight_ = true;
}

int Embedder::collect(float* out, int cap) {
  GTX_CHECK(in_flight_, "collect without a submitted pass");
  GTX_HIP(hipSetDevice(ctx_->device));
  GTX_HIP(hipEventSynchronize(done_));
  in_flight_ = false;
  const int n = n_flight_;
  if (n > 0 && h_sat_ && *h_sat_) {
    sat_seen_ = true;
    if (can_fall_back()) {                                      // this pass again at fp32's range, and every later one
      const void* f = cur_frames_;
      const std::vector<int> counts = cur_counts_;
      const std::vector<float> xyxy = cur_xyxy_;
      fall_back_to_exact();
      live()->submit_dev(f, (int)counts.size(), cur_h_, cur_w_, counts.data(), xyxy.data());
      return live()->collect(out, cap);
    }
  }
  GTX_CHECK(cap >= n, "output holds %d vectors, the pass has %d", cap, n);
  if (n > 0 && out) memcpy(out, h_emb_, (size_t)n * dim_ * sizeof(float));
  return n;
}

void Embedder::crops(int i, uint8_t* out) {
  GTX_CHECK(!in_flight_, "crops while a pass is in flight: call collect first");
  GTX_CHECK(i >= last_chunk_ && i < last_chunk_ + last_chunk_n_, "crop %d is not in the last chunk of the last pass", i);
  GTX_HIP(hipMemcpy(out, (const uint8_t*)img_.ptr + (size_t)(i - last_chunk_) * S_ * S_ * 4, (size_t)S_ * S_ * 4, hipMemcpyDeviceToHost));
}

void Embedder::layer_output(int i, const std::string& layer, float* out, int* h, int* w, int* c) {
  GTX_CHECK(!(out && in_flight_), "layer_output while a pass is in flight: call collect first");
  auto it = layer_views_.find(layer);
  if (it == layer_views_.end()) fail(-1, "unknown layer '%s'", layer.c_str());
  const View& v = it->second;
  if (h) *h = v.h;
  if (w) *w = v.w;
  if (c) *c = v.c;
  if (!out) return;
  GTX_CHECK(i >= last_chunk_ && i < last_chunk_ + last_chunk_n_, "crop %d is not in the last chunk of the last pass", i);
  read_view(v, i - last_chunk_, out);
}

void Embedder::profile(int n, int iters, std::vector<std::string>& names, std::vector<float>& ms, std::vector<double>& flops) {
  GTX_CHECK(finalized_ && !in_flight_, "profile: embedder not finalized or a pass in flight");
  GTX_CHECK(n >= 1 && n <= max_batch_ && iters >= 1, "bad profile arguments");
  names.clear(); ms.assign(ops_.size(), 0.f); flops.assign(ops_.size(), 0.0);
  for (const Op& op : ops_) names.push_back(op.name + " " + op.family);
  time_ops(n, iters, [&](size_t i, float t) {
    ms[i] += t / iters;
    flops[i] = ops_[i].flops;
  });
}

}  // namespace gtx

// ------------------------------------------------------------------ C ABI (include/gtx.h, "ReID embedder")
using gtx::guarded;
using gtx::need;

int gtx_embedder_create(gtx_ctx* ctx, int imgsz, int max_crops, int fp32_split, gtx_embedder** out) {
  return guarded([&] {
    need(ctx, "ctx"); need(out, "out");
    std::unique_ptr<gtx_embedder> e(new gtx_embedder);
    e->impl.reset(new gtx::Embedder(ctx, imgsz, max_crops, fp32_split != 0));
    *out = e.release();
  });
}
void gtx_embedder_destroy(gtx_embedder* e) { delete e; }
int gtx_embedder_set_tensor(gtx_embedder* e, const char* name, const float* data, int ndim, const int64_t* shape) {
  return guarded([&] {
    need(e, "embedder"); need(name, "name"); need(data, "data"); need(shape, "shape");
    e->impl->set_tensor(name, data, ndim, shape);
  });
}
int gtx_embedder_finalize(gtx_embedder* e) {
  return guarded([&] { need(e, "embedder"); e->impl->finalize(); });
}
int gtx_embedder_dim(gtx_embedder* e, int* dim) {
  return guarded([&] { need(e, "embedder"); need(dim, "dim"); *dim = e->impl->live()->dim(); });
}
int gtx_embedder_submit_dev(gtx_embedder* e, const void* frames_dptr, int nb, int h, int w, const int* counts, const float* xyxy) {
  return guarded([&] {
    need(e, "embedder"); need(counts, "counts");
    int n = 0;
    for (int b = 0; b < nb; ++b) n += counts[b];
    if (n > 0) need(xyxy, "xyxy");
    e->impl->live()->submit_dev(frames_dptr, nb, h, w, counts, xyxy);
  });
}
int gtx_embedder_collect(gtx_embedder* e, float* out, int cap, int* n) {
  return guarded([&] { need(e, "embedder"); need(n, "n"); *n = e->impl->live()->collect(out, cap); });
}
int gtx_embedder_embed_dev(gtx_embedder* e, const void* frames_dptr, int nb, int h, int w, const int* counts, const float* xyxy, float* out,
                           int cap, int* n) {
  const int rc = gtx_embedder_submit_dev(e, frames_dptr, nb, h, w, counts, xyxy);
  return rc != GTX_OK ? rc : gtx_embedder_collect(e, out, cap, n);
}
int gtx_embedder_crops(gtx_embedder* e, int i, uint8_t* out) {
  return guarded([&] { need(e, "embedder"); need(out, "out"); e->impl->live()->crops(i, out); });
}
int gtx_embedder_layer_output(gtx_embedder* e, int i, const char* layer, float* out, int* h, int* w, int* c) {
  return guarded([&] { need(e, "embedder"); need(layer, "layer"); e->impl->live()->layer_output(i, layer, out, h, w, c); });
}
int gtx_embedder_saturated(gtx_embedder* e, int clear, int* flag) {
  return guarded([&] { need(e, "embedder"); need(flag, "flag"); *flag = e->impl->saturated(clear != 0) ? 1 : 0; });
}
int gtx_embedder_fell_back(gtx_embedder* e, int* fell_back) {
  return guarded([&] { need(e, "embedder"); need(fell_back, "fell_back"); *fell_back = e->impl->fell_back() ? 1 : 0; });
}
int gtx_embedder_profile(gtx_embedder* e, int n, int iters, int cap, char* names, float* ms, double* flops, int* n_ops) {
  return guarded([&] {
    need(e, "embedder"); need(n_ops, "n_ops");
    std::vector<std::string> nm;
    std::vector<float> t;
    std::vector<double> f;
    e->impl->live()->profile(n, iters, nm, t, f);
    *n_ops = (int)nm.size();
    for (int i = 0; i < (int)nm.size() && i < cap; ++i) {
      if (names) { memset(names + (size_t)i * 128, 0, 128); strncpy(names + (size_t)i * 128, nm[i].c_str(), 127); }
      if (ms) ms[i] = t[i];
      if (flops) flops[i] = f[i];
    }
  });
}
int gtx_reid_crop_boxes(const float* xyxy, int n, int h, int w, int* out) {
  return guarded([&] {
    if (n > 0) { need(xyxy, "xyxy"); need(out, "out"); }
    for (int i = 0; i < n; ++i) gtx::reid_crop_box(xyxy + (size_t)i * 4, h, w, out + (size_t)i * 4);
  });
}
