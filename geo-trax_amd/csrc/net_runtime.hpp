// What every network built on the convolution kernels shares (YOLOv8 / P2 and RT-DETR detectors, the YOLOv8-cls ReID
// embedder): the host copies of the tensors, a zero-filled device arena, the conv-op emitter, per-op timing, the read-back of
// a layer to fp32, and the split-f16x3 saturation policy with its exact-fp32 twin. DetectorBase adds the detector skeleton
// (letterbox, gray ring, submit / collect) around a family's forward graph.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gtx.h"
#include "common.hpp"
#include "conv_igemm.hpp"
#include "det_kernels.hpp"
#include "rtdetr_kernels.hpp"

struct gtx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipDeviceProp_t prop{};
  // device words of the two operator hooks, each allocated and initialised by its hook's first call and never written by the host again
  void* orb_match_ticket = nullptr;  // gtx_op_orb_match (stabilizer.hip): match_kernel's ticket
  void* orb_ransac_state = nullptr;  // gtx_op_orb_ransac (homography.hip): ransac_kernel's two state words
  // gtx_op_gray_resize(_dev) (stabilizer.hip): the column / row tap tables of every (frame, working size) pair the context was asked
  // for, uploaded once each and never written again (a run asks for one pair)
  struct GrayTab { int fh, fw, gh, gw; void* tab; };
  std::vector<GrayTab> gray_tabs;
  ~gtx_ctx() {
    for (auto& t : gray_tabs)
      if (t.tab) (void)hipFree(t.tab);
    if (orb_match_ticket) (void)hipFree(orb_match_ticket);
    if (orb_ransac_state) (void)hipFree(orb_ransac_state);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace gtx {

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
};

// A channel slice of an NHWC device buffer.
struct View {
  void* ptr = nullptr;
  int n = 0, h = 0, w = 0;
  int cstride = 0, coff = 0, c = 0;
  bool plain = false;      // split-f16x3 path: plain fp32 instead of the pair format (the Detect head's last stage, token rows, score maps)
  View slice(int off, int cnt) const {
    View v = *this;
    v.coff = coff + off;
    v.c = cnt;
    return v;
  }
  // what the map-side kernels take by value (rtdetr_kernels.hpp); the one place that orders the fields
  RtMap map() const { return RtMap{ptr, h, w, cstride, coff, c}; }
};

// What the timing helpers read of an op of a forward graph. flops / bytes are algorithmic (2 * MAC; inputs read once + outputs
// written once + weights) and are those of one pass at the batch size of the last set_batch().
struct OpInfo {
  std::string name;      // ultralytics module path ("model.2.m.0.cv1") or group label
  std::string family;    // kernel symbol, as rocprof prints it
  double flops = 0;
  double bytes = 0;
};

// Rows of a per-kernel-family (or per-launch) timing table, one per label in first-seen order.
struct KernelTable {
  std::vector<std::string>& names;
  std::vector<int>& launches;
  std::vector<float>& ms;
  std::vector<double>& flops;
  std::vector<double>& bytes;
  std::map<std::string, size_t> idx;
  void add(const std::string& label, int n, float t, double f, double b);
};

class YoloTrunk;

class NetRuntime {
 public:
  NetRuntime(gtx_ctx* ctx, int fmt, size_t view_es, int max_batch) : ctx_(ctx), fmt_(fmt), view_es_(view_es), max_batch_(max_batch) {}
  virtual ~NetRuntime();
  NetRuntime(const NetRuntime&) = delete;
  NetRuntime& operator=(const NetRuntime&) = delete;
  // The YOLOv8 trunk (yolo_trunk.hpp) is a part of the net that holds it, not a family: it builds through the protected calls
  // below (tensor / has, alloc / new_view, emit_conv / emit_named_conv, bias_of, upload, set_layer_view, repoint_layer_views, release_buffer, format, device, sat_flag)
  // and touches no data member.
  friend class YoloTrunk;
  void set_tensor(const std::string& name, const float* data, int ndim, const int64_t* shape);
  // split-f16x3 path: true when some activation of a collected pass (since the last call with clear) had to be clamped to fp16's
  // range on its way into the pair format. The pass is then re-run on an exact-fp32 twin built from the same tensors and every
  // later call goes there (`ultralytics.half: false` promises fp32's range, default.yaml:245); GTX_SAT_FALLBACK=0 keeps the flag only.
  bool saturated(bool clear);
  bool fell_back() const { return exact_ != nullptr; }
  virtual void finalize() = 0;

 protected:
  // ---- the forward graph, as the shared helpers see it
  virtual size_t op_count() const = 0;
  virtual const OpInfo& op_info(size_t i) const = 0;
  virtual void launch_op(size_t i, int nb, hipStream_t s) = 0;
  virtual void set_batch(int nb) = 0;
  // every op of the graph on `s`; ev (may be null): an event in front of every launch and one behind the last
  void run_ops(int nb, hipStream_t s, hipEvent_t* ev);
  // `iters` passes at batch nb with events around every launch; fold(i, ms) per op and pass
  template <class F> void time_ops(int nb, int iters, F fold);

  // ---- host tensors and device memory
  const HostTensor& tensor(const std::string& name) const;
  bool has(const std::string& name) const { return tensors_.count(name) != 0; }
  const float* bias_of(const std::string& name, int cout) const;   // "<name>.bias" or null
  void* alloc(size_t bytes);                                         // zero-filled, freed with the net
  float* upload(const std::vector<float>& v);
  View new_view(int h, int w, int c, bool plain = false);           // [max_batch][h][w][c] elements of view_es_ bytes

  // ---- one Conv op: OIHW weights (cout x cin x ks x ks), bias (may be null: zeros). Picks the tile configuration, packs the
  // weights (shared packed-image cache), uploads weights and bias and fills the op's ConvProblem; the output is *out_slice or a
  // new view. plain_out: the split path writes plain fp32. The op is appended to `ops`.
  struct ConvArgs {
    int stride = 1, act = 1;
    const View* out_slice = nullptr;
    const View* residual = nullptr;
    bool plain_out = false;
    int force_kc = 0, force_bn = 0;
  };
  template <class OpT>
  View emit_conv(std::vector<OpT>& ops, const std::string& name, const float* w_oihw, int cout, int cin, int ks, const float* bias,
                 const View& x, const ConvArgs& a) {
    OpT op;
    op.kind = OpT::CONV;
    op.name = name;
    const View out = conv_problem(name, w_oihw, cout, cin, ks, bias, x, a, op.cfg, op.grp.p[0]);
    op.grp.count = 1;
    op.family = conv_kernel_name(op.cfg);
    ops.push_back(op);
    layer_views_[name] = out;
    return out;
  }
  // The same from the tensors "<name>.weight" (OIHW, square kernel) and "<name>.bias" (optional).
  template <class OpT>
  View emit_named_conv(std::vector<OpT>& ops, const std::string& name, const View& x, const ConvArgs& a) {
    const HostTensor& w = tensor(name + ".weight");
    GTX_CHECK(w.shape.size() == 4 && w.shape[2] == w.shape[3], "%s: expected OIHW square kernel", name.c_str());
    const int cout = (int)w.shape[0], cin = (int)w.shape[1], ks = (int)w.shape[2];
    return emit_conv(ops, name, w.data.data(), cout, cin, ks, bias_of(name, cout), x, a);
  }

  // ---- the layers layer_output() can read, by module path
  void set_layer_view(const std::string& name, const View& v) { layer_views_[name] = v; }
  void repoint_layer_views(const void* from, void* to);   // every layer on buffer `from` now points at `to`
  size_t release_buffer(const void* p);                    // gives arena buffer p back early: its size (0: p is none of them)
  int format() const { return fmt_; }
  int device() const { return ctx_->device; }
  int* sat_flag() const { return sat_dev_; }                // null off the split-f16x3 path

  // ---- layer v of batch slot `slot` as fp32 [h][w][c] (pair format, fp16 or fp32 per the net's format and v.plain)
  void read_view(const View& v, int slot, float* out) const;

  // ---- saturation policy
  void alloc_sat_flag();            // split path: the flag the kernels raise, and its pinned copy
  void drop_tensors_unless_fallback();   // at finalize: the host copies stay only while a fallback can happen
  bool can_fall_back() const { return !tensors_.empty(); }
  virtual std::unique_ptr<NetRuntime> make_exact() const = 0;   // the exact-fp32 twin, not finalized
  virtual void release_graph() = 0;                             // the family's ops and what refers to the released buffers
  void fall_back_to_exact();
  template <class T> T* live_as() { return exact_ ? static_cast<T*>(exact_.get()) : static_cast<T*>(this); }

  gtx_ctx* ctx_;
  int fmt_;                 // activation format of the maps: DT_F16, DT_F32 or DT_F32S (what the conv kernels compute in)
  size_t view_es_;          // bytes per element new_view allocates
  int max_batch_;
  bool finalized_ = false;
  int cur_nb_ = 0;
  std::map<std::string, HostTensor> tensors_;
  std::vector<DevBuf> bufs_;
  std::map<std::string, View> layer_views_;
  std::unique_ptr<NetRuntime> exact_;
  int* sat_dev_ = nullptr;  // set by the split kernels when they clamp (ConvProblem::sat_flag)
  int* h_sat_ = nullptr;    // pinned copy, refreshed by every pass
  bool sat_seen_ = false;

 private:
  View conv_problem(const std::string& name, const float* w_oihw, int cout, int cin, int ks, const float* bias, const View& x,
                    const ConvArgs& a, ConvConfig& cfg, ConvProblem& p);
};

template <class F>
void NetRuntime::time_ops(int nb, int iters, F fold) {
  hipStream_t s = ctx_->stream;
  set_batch(nb);
  const size_t n = op_count();
  std::vector<hipEvent_t> ev(n + 1);
  for (auto& e : ev) GTX_HIP(hipEventCreate(&e));
  for (int it = 0; it < iters; ++it) {
    run_ops(nb, s, ev.data());
    GTX_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
      float t = 0.f;
      GTX_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
      fold(i, t);
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
}

// What the C ABI's gtx_detector_* entry points call: one implementation per detector family (gtx_det_config::arch), the way the
// reference swaps YOLO for RTDETR on the model's yaml (geotrax/extract.py:222-225). The calls that run or read a pass go to
// live(): the exact-fp32 twin once a split-f16x3 pass has saturated.
class DetectorBase : public NetRuntime {
 public:
  DetectorBase(gtx_ctx* ctx, const gtx_det_config& cfg, int fmt, size_t view_es, int in_dtype);
  ~DetectorBase() override;
  DetectorBase* live() { return live_as<DetectorBase>(); }
  void input_size(int* h, int* w) const { *h = lb_.net_h; *w = lb_.net_w; }
  // frames: device pointer, nb frames [h][w][3] u8 back to back. Outputs sized [nb][max_det].
  void detect_dev(const void* frames, int nb, int h, int w, int* n_out, float* xyxy, float* conf, int* cls, float speed_ms[3]);
  // asynchronous pair: submit enqueues the whole pass, collect waits for it and unpacks
  void submit_dev(const void* frames, int nb, int h, int w);
  void collect(int* n_out, float* xyxy, float* conf, int* cls, float speed_ms[3]);
  void detect_host(const uint8_t* frame, int h, int w, int* n_out, float* xyxy, float* conf, int* cls, float speed_ms[3]);
  const void* gray(int b, int* gh, int* gw) const;
  virtual void raw_output(int b, float* out, int* n_anchors, bool logits = false) = 0;
  virtual void layer_output(int b, const std::string& layer, float* out, int* h, int* w, int* c) = 0;
  // per-kernel-family totals of `iters` forward passes at batch nb (GTX_PROFILE_PER_OP: one line per launch, "NNN <module path>")
  void profile(int nb, int iters, std::vector<std::string>& names, std::vector<int>& launches, std::vector<float>& ms,
               std::vector<double>& flops, std::vector<double>& bytes);
  // Live tracing: every `every_n`-th submitted pass gets a HIP event in front of every launch of the forward graph (on the launch
  // stream); collect() folds the elapsed times into per-op totals that trace_report() returns per kernel family and clears.
  // every_n = 0 switches tracing off.
  void set_trace(int every_n);
  void trace_report(std::vector<std::string>& names, std::vector<int>& launches, std::vector<float>& ms, std::vector<double>& flops,
                    std::vector<double>& bytes);
  virtual void features(int b, float* out, int cap, int* n, int* dim) const = 0;
  virtual void pad_skip(int* on, int* skipped, int* total) const = 0;
  virtual void sparse_box(int* on, int* overflows) const = 0;

  // gray images of the last batches: a batch's image lives until kGrayRing - 2 more batches have been submitted after the one
  // that follows it (engine.py sizes its queues from this)
  static constexpr int kGrayRing = GTX_GRAY_RING;

 protected:
  void alloc_outputs();                   // the gray ring and the pinned result rows / counts (at finalize)
  // after the forward pass: decode / NMS and the copies of the result rows / counts (and the saturation flag) to the pinned buffers
  virtual void run_post(int nb, hipStream_t s) = 0;
  // in collect(), before the rows are unpacked: what the pass left out for this batch
  virtual void after_pass(int nb) { (void)nb; }
  void record_post_end(hipStream_t s) { GTX_HIP(hipEventRecord(ev_[3], s)); }   // a re-run in after_pass counts as postprocess

  gtx_det_config cfg_;
  int in_dtype_;                          // what launch_preprocess writes into img_
  Letterbox lb_{};                        // set by the family's constructor
  View img_;                              // the network input, [N][net_h][net_w] RGB0 bytes
  int* h_out_n_ = nullptr;                // pinned result counts / rows [N][max_det][6]
  float* h_out_rows_ = nullptr;
  bool in_flight_ = false;
  int flight_nb_ = 0;

 private:
  DevBuf frame_stage_;                    // device copy of host frames for detect_host
  DevBuf gray_;                           // [kGrayRing][N][gh][gw] u8
  int gray_h_ = 0, gray_w_ = 0;
  int gray_slot_ = 0, collected_gray_slot_ = 0;
  const void* cur_frames_ = nullptr;
  hipEvent_t ev_[4]{};
  hipEvent_t ev_up_[2]{};
  int trace_every_ = 0, trace_count_ = 0;
  bool flight_traced_ = false;
  std::vector<hipEvent_t> trace_ev_;      // one per op + 1
  std::vector<double> trace_ms_;          // per op
  std::vector<int> trace_n_;
  std::vector<double> trace_flops_, trace_bytes_;   // per op, summed over the traced passes (each at its own batch size)
};

}  // namespace gtx

struct gtx_detector {
  std::unique_ptr<gtx::DetectorBase> impl;
};
