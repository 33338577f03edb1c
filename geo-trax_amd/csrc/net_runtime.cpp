// NetRuntime / DetectorBase (net_runtime.hpp): the plumbing the YOLOv8, RT-DETR and ReID networks share.
#include "net_runtime.hpp"
#include "split_format.hpp"

#include <array>
#include <deque>
#include <functional>
#include <mutex>

namespace gtx {

void KernelTable::add(const std::string& label, int n, float t, double f, double b) {
  auto it = idx.find(label);
  size_t k;
  if (it == idx.end()) {
    k = names.size();
    idx[label] = k;
    names.push_back(label);
    launches.push_back(0); ms.push_back(0.f); flops.push_back(0.0); bytes.push_back(0.0);
  } else {
    k = it->second;
  }
  launches[k] += n;
  ms[k] += t;
  flops[k] += f;
  bytes[k] += b;
}

NetRuntime::~NetRuntime() {
  if (h_sat_) (void)hipHostFree(h_sat_);
}

void NetRuntime::set_tensor(const std::string& name, const float* data, int ndim, const int64_t* shape) {
  GTX_CHECK(!finalized_, "set_tensor after finalize");
  HostTensor t;
  size_t n = 1;
  for (int i = 0; i < ndim; ++i) {
    t.shape.push_back(shape[i]);
    n *= (size_t)shape[i];
  }
  t.data.assign(data, data + n);
  tensors_[name] = std::move(t);
}

const HostTensor& NetRuntime::tensor(const std::string& name) const {
  auto it = tensors_.find(name);
  if (it == tensors_.end()) fail(-1, "missing tensor '%s'", name.c_str());
  return it->second;
}

const float* NetRuntime::bias_of(const std::string& name, int cout) const {
  if (!has(name + ".bias")) return nullptr;
  const HostTensor& b = tensor(name + ".bias");
  GTX_CHECK((int)b.data.size() == cout, "%s: bias size", name.c_str());
  return b.data.data();
}

void* NetRuntime::alloc(size_t bytes) {
  bufs_.emplace_back(bytes);
  GTX_HIP(hipMemset(bufs_.back().p, 0, bufs_.back().bytes));
  return bufs_.back().p;
}

void NetRuntime::repoint_layer_views(const void* from, void* to) {
  for (auto& kv : layer_views_)
    if (kv.second.ptr == from) kv.second.ptr = to;
}

size_t NetRuntime::release_buffer(const void* p) {
  for (size_t b = 0; b < bufs_.size(); ++b) {
    if (bufs_[b].p != p) continue;
    const size_t bytes = bufs_[b].bytes;
    bufs_.erase(bufs_.begin() + (long)b);
    return bytes;
  }
  return 0;
}

float* NetRuntime::upload(const std::vector<float>& v) {
  float* d = (float*)alloc(std::max<size_t>(v.size(), 1) * sizeof(float));
  if (!v.empty()) GTX_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return d;
}

View NetRuntime::new_view(int h, int w, int c, bool plain) {
  View v;
  v.n = max_batch_;
  v.h = h;
  v.w = w;
  v.cstride = c;
  v.coff = 0;
  v.c = c;
  v.plain = plain;
  v.ptr = alloc((size_t)v.n * h * w * c * view_es_);
  return v;
}

void NetRuntime::run_ops(int nb, hipStream_t s, hipEvent_t* ev) {
  const size_t n = op_count();
  for (size_t i = 0; i < n; ++i) {
    if (ev) GTX_HIP(hipEventRecord(ev[i], s));
    launch_op(i, nb, s);
  }
  if (ev) GTX_HIP(hipEventRecord(ev[n], s));
}

namespace {
// Packed weight images are a pure function of (tensor bytes, tile configuration). An engine builds several detectors from
// the same tensors (one per stream) and a run builds engines video after video: the image is made once per process and
// shared (packing YOLOv8s takes ~0.15 s of host time per detector, most of what creating one costs).
struct PackedWeights {
  std::vector<uint8_t> bytes;
  float acc_scale = 1.f;
  std::vector<float> source;      // the tensor the image was packed from: a hit is a hit only when these floats are the caller's
};
std::shared_ptr<const PackedWeights> packed_weights(const float* w, size_t n, int cout, int cin, const ConvConfig& cfg,
                                                    const std::function<PackedWeights()>& make) {
  static std::mutex mu;
  static std::map<std::array<uint64_t, 4>, std::shared_ptr<const PackedWeights>> cache;
  uint64_t h = 1469598103934665603ull;                       // FNV-1a over the tensor's bytes, 8 at a time
  const uint64_t* q = reinterpret_cast<const uint64_t*>(w);
  for (size_t i = 0; i < n / 2; ++i) h = (h ^ q[i]) * 1099511628211ull;
  if (n & 1) h = (h ^ (uint64_t)__builtin_bit_cast(uint32_t, w[n - 1])) * 1099511628211ull;
  const std::array<uint64_t, 4> key = {h, (uint64_t)n, ((uint64_t)cout << 32) | (uint64_t)cin,
                                       ((uint64_t)cfg.dtype << 40) | ((uint64_t)cfg.ks << 32) | ((uint64_t)cfg.bn << 16) | ((uint64_t)cfg.kc << 4) | (uint64_t)cfg.variant};
  // The key's 64-bit FNV-1a is a filter, not an identity: a hit must also hold the same floats (a collision between two layers or
  // checkpoints of one shape would otherwise run the network on another tensor's weights, silently). Bounded by bytes: the
  // images + sources of a YOLOv8x are ~1 GB; past 2 GB the oldest entries go.
  static std::deque<std::array<uint64_t, 4>> order;
  static size_t held = 0;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end() && it->second->source.size() == n && memcmp(it->second->source.data(), w, n * sizeof(float)) == 0)
      return it->second;
  }
  PackedWeights fresh = make();
  fresh.source.assign(w, w + n);
  auto made = std::make_shared<const PackedWeights>(std::move(fresh));
  const size_t cost = made->bytes.size() + made->source.size() * sizeof(float);
  std::lock_guard<std::mutex> lk(mu);
  auto old = cache.find(key);
  if (old != cache.end()) {                                    // same key, other floats: the newer tensor takes the slot
    held -= old->second->bytes.size() + old->second->source.size() * sizeof(float);
    cache.erase(old);
    order.erase(std::remove(order.begin(), order.end(), key), order.end());
  }
  while (!order.empty() && held + cost > ((size_t)2 << 30)) {
    auto victim = cache.find(order.front());
    if (victim != cache.end()) {
      held -= victim->second->bytes.size() + victim->second->source.size() * sizeof(float);
      cache.erase(victim);                                     // nets that use the image keep it alive through their shared_ptr
    }
    order.pop_front();
  }
  held += cost;
  order.push_back(key);
  return cache.emplace(key, std::move(made)).first->second;
}
}  // namespace

View NetRuntime::conv_problem(const std::string& name, const float* w, int cout, int cin, int ks, const float* bias, const View& x,
                              const ConvArgs& a, ConvConfig& cfg, ConvProblem& p) {
  GTX_CHECK(cin == x.c, "%s: weight expects %d input channels, input view has %d", name.c_str(), cin, x.c);
  const int pad = ks / 2;
  const int ho = (x.h + 2 * pad - ks) / a.stride + 1, wo = (x.w + 2 * pad - ks) / a.stride + 1;
  View out = a.out_slice ? *a.out_slice : new_view(ho, wo, cout);
  GTX_CHECK(out.h == ho && out.w == wo && out.c == cout, "%s: output view mismatch", name.c_str());
  out.plain = fmt_ != DT_F16 && (a.plain_out || out.plain);        // fp16 maps everywhere, the score maps included
  GTX_CHECK(fmt_ == DT_F32 || (!x.plain && (!a.residual || !a.residual->plain)), "%s: a plain fp32 tensor cannot feed this convolution", name.c_str());
  if (fmt_ == DT_F32S)                                              // pair format: whole 8-channel groups everywhere
    GTX_CHECK(x.cstride % 8 == 0 && x.coff % 8 == 0 && out.cstride % 8 == 0 && out.coff % 8 == 0 &&
                  (!a.residual || (a.residual->cstride % 8 == 0 && a.residual->coff % 8 == 0)),
              "%s: channel strides / offsets of the split-f16x3 path must be multiples of 8", name.c_str());
  cfg = conv_pick_config(fmt_, ks, a.stride, cin, cout, a.force_kc, a.force_bn);
  const size_t n = (size_t)cout * cin * ks * ks;
  const auto pw = packed_weights(w, n, cout, cin, cfg, [&] {
    PackedWeights r;
    std::vector<float> ohwi(n);                                     // OIHW -> OHWI
    const int taps = ks * ks;
    parallel_for(cout, [&](int o) {
      for (int i = 0; i < cin; ++i)
        for (int t = 0; t < taps; ++t) ohwi[((size_t)o * taps + t) * cin + i] = w[((size_t)o * cin + i) * taps + t];
    });
    r.bytes = pack_conv_weights(ohwi.data(), cout, cin, cfg, &r.acc_scale);
    return r;
  });
  void* dw = alloc(pw->bytes.size());
  GTX_HIP(hipMemcpy(dw, pw->bytes.data(), pw->bytes.size(), hipMemcpyHostToDevice));
  float* db = (float*)alloc(((cout + 63) / 64 * 64) * sizeof(float));   // zero-filled up to a whole cout tile: the kernels load a tile's bias unconditionally
  if (bias) GTX_HIP(hipMemcpy(db, bias, cout * sizeof(float), hipMemcpyHostToDevice));
  p = ConvProblem{};
  p.in = x.ptr; p.out = out.ptr; p.wpack = dw; p.bias = db;
  p.res = a.residual ? a.residual->ptr : nullptr;
  p.N = x.n; p.H = x.h; p.W = x.w; p.Ho = ho; p.Wo = wo; p.Cin = cin; p.Cout = cout;
  p.in_cstride = x.cstride; p.in_coff = x.coff;
  p.out_cstride = out.cstride; p.out_coff = out.coff;
  p.res_cstride = a.residual ? a.residual->cstride : 0;
  p.res_coff = a.residual ? a.residual->coff : 0;
  p.act = a.act;
  p.acc_scale = pw->acc_scale;
  p.out_plain = (fmt_ == DT_F32S && out.plain) ? 1 : 0;
  p.sat_flag = fmt_ == DT_F32S ? sat_dev_ : nullptr;
  return out;
}

void NetRuntime::read_view(const View& v, int slot, float* out) const {
  const size_t px = (size_t)v.h * v.w;
  const size_t es = (fmt_ == DT_F16 && !v.plain) ? 2 : 4;
  std::vector<uint8_t> host(px * v.cstride * es);
  GTX_HIP(hipMemcpy(host.data(), (const uint8_t*)v.ptr + (size_t)slot * px * v.cstride * es, host.size(), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < px; ++p)
    for (int k = 0; k < v.c; ++k) {
      const size_t src = p * v.cstride + v.coff + k;
      float f;
      if (fmt_ == DT_F32S && !v.plain) {
        f = pair_element(host.data(), src);
      } else if (es == 2) {
        _Float16 hv;
        memcpy(&hv, host.data() + src * 2, 2);
        f = (float)hv;
      } else {
        memcpy(&f, host.data() + src * 4, 4);
      }
      out[p * v.c + k] = f;
    }
}

void NetRuntime::alloc_sat_flag() {
  if (fmt_ != DT_F32S) return;
  sat_dev_ = (int*)alloc(sizeof(int));
  GTX_HIP(hipHostMalloc((void**)&h_sat_, sizeof(int)));
  *h_sat_ = 0;
}

void NetRuntime::drop_tensors_unless_fallback() {
  static const bool fallback = env_flag("GTX_SAT_FALLBACK", true);
  if (fmt_ != DT_F32S || !fallback) tensors_.clear();
}

bool NetRuntime::saturated(bool clear) {
  const bool r = sat_seen_;
  if (clear) {
    sat_seen_ = false;
    if (sat_dev_ && !exact_) {
      GTX_HIP(hipSetDevice(ctx_->device));
      GTX_HIP(hipMemsetAsync(sat_dev_, 0, sizeof(int), ctx_->stream));
    }
  }
  return r;
}

// A split-f16x3 pass clamped an activation: from here on this object is a shell around an exact-fp32 twin built from the same
// tensors on the same context. The split graph's device memory (activations, packed weights) is given back.
void NetRuntime::fall_back_to_exact() {
  std::unique_ptr<NetRuntime> d = make_exact();
  for (const auto& kv : tensors_) d->set_tensor(kv.first, kv.second.data.data(), (int)kv.second.shape.size(), kv.second.shape.data());
  d->finalize();
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  release_graph();
  layer_views_.clear();
  bufs_.clear();
  tensors_.clear();
  exact_ = std::move(d);
}

// ---------------------------------------------------------------------------- DetectorBase

DetectorBase::DetectorBase(gtx_ctx* ctx, const gtx_det_config& cfg, int fmt, size_t view_es, int in_dtype)
    : NetRuntime(ctx, fmt, view_es, std::max(cfg.max_batch, 1)), cfg_(cfg), in_dtype_(in_dtype) {
  GTX_CHECK(cfg.imgsz > 0 && cfg.imgsz % 32 == 0, "imgsz must be a positive multiple of 32 (got %d)", cfg.imgsz);
  GTX_CHECK(cfg.max_det > 0 && cfg.nc > 0 && cfg.nc <= 128, "max_det must be positive and nc in [1, 128] (got %d, %d)", cfg.max_det, cfg.nc);
  GTX_CHECK(cfg.frame_h > 0 && cfg.frame_w > 0, "frame size must be given");
  cfg_.max_batch = max_batch_;
  GTX_HIP(hipSetDevice(ctx->device));
  for (auto& e : ev_) GTX_HIP(hipEventCreateWithFlags(&e, wait_event_flags(true)));
  for (auto& e : ev_up_) GTX_HIP(hipEventCreate(&e));
}

DetectorBase::~DetectorBase() {
  if (h_out_n_) (void)hipHostFree(h_out_n_);
  if (h_out_rows_) (void)hipHostFree(h_out_rows_);
  for (auto& e : ev_)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : ev_up_)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : trace_ev_)
    if (e) (void)hipEventDestroy(e);
}

void DetectorBase::alloc_outputs() {
  const int N = cfg_.max_batch;
  gray_h_ = cfg_.frame_h / 2;
  gray_w_ = cfg_.frame_w / 2;
  gray_.alloc((size_t)kGrayRing * N * gray_h_ * gray_w_);
  GTX_HIP(hipHostMalloc((void**)&h_out_n_, sizeof(int) * N));
  GTX_HIP(hipHostMalloc((void**)&h_out_rows_, sizeof(float) * 6 * N * cfg_.max_det));
}

// Asynchronous half: enqueue preprocess -> forward -> the family's post stage (with the D2H copies of the result rows) on the
// context's stream and return. Results are picked up by collect(). The gray image of this batch goes to the next slot of the
// ring so that consumers on other streams (stabilizers) can still read the images of the batches before the newest collected one.
void DetectorBase::submit_dev(const void* frames, int nb, int h, int w) {
  GTX_CHECK(finalized_, "detector not finalized");
  GTX_CHECK(!in_flight_, "submit while a batch is in flight: call collect first");
  GTX_CHECK(nb >= 1 && nb <= cfg_.max_batch, "batch %d outside [1,%d]", nb, cfg_.max_batch);
  GTX_CHECK(h == cfg_.frame_h && w == cfg_.frame_w, "frame is %dx%d, detector was created for %dx%d", w, h, cfg_.frame_w, cfg_.frame_h);
  GTX_HIP(hipSetDevice(ctx_->device));
  hipStream_t s = ctx_->stream;
  set_batch(nb);
  cur_frames_ = frames;
  gray_slot_ = (gray_slot_ + 1) % kGrayRing;
  uint8_t* gray = gray_.as<uint8_t>() + (size_t)gray_slot_ * cfg_.max_batch * gray_h_ * gray_w_;
  GTX_HIP(hipEventRecord(ev_[0], s));
  launch_preprocess(in_dtype_, (const uint8_t*)frames, nb, lb_, img_.ptr, gray, gray_h_, gray_w_, s);
  GTX_HIP(hipEventRecord(ev_[1], s));
  flight_traced_ = trace_every_ > 0 && (trace_count_++ % trace_every_) == 0;
  run_ops(nb, s, flight_traced_ ? trace_ev_.data() : nullptr);
  GTX_HIP(hipEventRecord(ev_[2], s));
  run_post(nb, s);
  GTX_HIP(hipEventRecord(ev_[3], s));
  in_flight_ = true;
  flight_nb_ = nb;
}

void DetectorBase::collect(int* n_out, float* xyxy, float* conf, int* cls, float speed_ms[3]) {
  GTX_CHECK(in_flight_, "collect without a submitted batch");
  GTX_HIP(hipSetDevice(ctx_->device));
  GTX_HIP(hipEventSynchronize(ev_[3]));
  in_flight_ = false;
  collected_gray_slot_ = gray_slot_;
  if (h_sat_ && *h_sat_) {
    sat_seen_ = true;
    if (can_fall_back()) {
      // this batch again, at fp32's range: the frames are still where the caller put them (one batch in flight per detector)
      flight_traced_ = false;
      fall_back_to_exact();
      if (trace_every_ > 0) live()->set_trace(trace_every_);
      return live()->detect_dev(cur_frames_, flight_nb_, cfg_.frame_h, cfg_.frame_w, n_out, xyxy, conf, cls, speed_ms);
    }
  }
  if (flight_traced_) {
    for (size_t i = 0; i < op_count(); ++i) {
      float t = 0.f;
      GTX_HIP(hipEventElapsedTime(&t, trace_ev_[i], trace_ev_[i + 1]));
      trace_ms_[i] += t;
      trace_n_[i] += 1;
      trace_flops_[i] += op_info(i).flops;        // of THIS pass's batch size (set_batch ran in submit_dev)
      trace_bytes_[i] += op_info(i).bytes;
    }
    flight_traced_ = false;
  }
  after_pass(flight_nb_);
  for (int b = 0; b < flight_nb_; ++b) {
    const int n = h_out_n_[b];
    n_out[b] = n;
    const float* rows = h_out_rows_ + (size_t)b * cfg_.max_det * 6;
    for (int i = 0; i < n; ++i) {
      float* bx = xyxy + ((size_t)b * cfg_.max_det + i) * 4;
      bx[0] = rows[i * 6 + 0]; bx[1] = rows[i * 6 + 1]; bx[2] = rows[i * 6 + 2]; bx[3] = rows[i * 6 + 3];
      conf[(size_t)b * cfg_.max_det + i] = rows[i * 6 + 4];
      cls[(size_t)b * cfg_.max_det + i] = (int)rows[i * 6 + 5];
    }
  }
  if (speed_ms)
    for (int i = 0; i < 3; ++i) GTX_HIP(hipEventElapsedTime(&speed_ms[i], ev_[i], ev_[i + 1]));
}

void DetectorBase::detect_dev(const void* frames, int nb, int h, int w, int* n_out, float* xyxy, float* conf, int* cls, float speed_ms[3]) {
  submit_dev(frames, nb, h, w);
  collect(n_out, xyxy, conf, cls, speed_ms);
}

void DetectorBase::detect_host(const uint8_t* frame, int h, int w, int* n_out, float* xyxy, float* conf, int* cls, float speed_ms[3]) {
  GTX_CHECK(finalized_, "detector not finalized");
  GTX_HIP(hipSetDevice(ctx_->device));
  const size_t bytes = (size_t)h * w * 3;
  if (frame_stage_.bytes < bytes) frame_stage_.alloc(bytes);
  GTX_HIP(hipEventRecord(ev_up_[0], ctx_->stream));
  GTX_HIP(hipMemcpyAsync(frame_stage_.p, frame, bytes, hipMemcpyHostToDevice, ctx_->stream));
  GTX_HIP(hipEventRecord(ev_up_[1], ctx_->stream));
  detect_dev(frame_stage_.p, 1, h, w, n_out, xyxy, conf, cls, speed_ms);
  if (speed_ms) {
    float up_ms = 0.f;
    GTX_HIP(hipEventElapsedTime(&up_ms, ev_up_[0], ev_up_[1]));
    speed_ms[0] += up_ms;  // the host->device copy is part of "preprocess"
  }
}

const void* DetectorBase::gray(int b, int* gh, int* gw) const {
  if (gh) *gh = gray_h_;
  if (gw) *gw = gray_w_;
  if (b < 0 || b >= cfg_.max_batch) return nullptr;
  // the image of the most recently *collected* batch (a newer batch may already be in flight)
  return gray_.as<uint8_t>() + ((size_t)collected_gray_slot_ * cfg_.max_batch + b) * gray_h_ * gray_w_;
}

void DetectorBase::profile(int nb, int iters, std::vector<std::string>& names, std::vector<int>& launches, std::vector<float>& ms,
                           std::vector<double>& flops, std::vector<double>& bytes) {
  GTX_CHECK(finalized_, "detector not finalized");
  GTX_CHECK(nb >= 1 && nb <= cfg_.max_batch && iters >= 1, "bad profile arguments");
  const bool per_op = std::getenv("GTX_PROFILE_PER_OP") != nullptr;   // one line per launch (its module path) instead of per kernel family
  KernelTable table{names, launches, ms, flops, bytes, {}};
  time_ops(nb, iters, [&](size_t i, float t) {
    const OpInfo& op = op_info(i);
    const std::string n = std::to_string(i);
    table.add(per_op ? std::string(n.size() < 3 ? 3 - n.size() : 0, '0') + n + " " + op.name : op.family, 1, t, op.flops, op.bytes);
  });
}

void DetectorBase::set_trace(int every_n) {
  GTX_CHECK(finalized_ && every_n >= 0, "set_trace: detector not finalized or bad period");
  GTX_CHECK(!in_flight_, "set_trace while a batch is in flight");
  trace_every_ = every_n;
  trace_count_ = 0;
  const size_t n = op_count();
  if (every_n > 0 && trace_ev_.empty()) {
    trace_ev_.resize(n + 1);
    for (auto& e : trace_ev_) GTX_HIP(hipEventCreate(&e));
  }
  trace_ms_.assign(n, 0.0);
  trace_n_.assign(n, 0);
  trace_flops_.assign(n, 0.0);
  trace_bytes_.assign(n, 0.0);
}

void DetectorBase::trace_report(std::vector<std::string>& names, std::vector<int>& launches, std::vector<float>& ms,
                                std::vector<double>& flops, std::vector<double>& bytes) {
  KernelTable table{names, launches, ms, flops, bytes, {}};
  const size_t n = op_count();
  for (size_t i = 0; i < n && i < trace_n_.size(); ++i)
    if (trace_n_[i] > 0) table.add(op_info(i).family, trace_n_[i], (float)trace_ms_[i], trace_flops_[i], trace_bytes_[i]);
  trace_ms_.assign(n, 0.0);
  trace_n_.assign(n, 0);
  trace_flops_.assign(n, 0.0);
  trace_bytes_.assign(n, 0.0);
}

}  // namespace gtx
