// RT-DETR detector runtime: builds the layer graph from ultralytics-named fused tensors and runs preprocess -> trunk -> query
// selection -> deformable-attention decoder -> score / box stage on a HIP stream. Stands in for what ultralytics' RTDETR predictor
// does underneath model.track() when the model's yaml names RT-DETR (geotrax/extract.py:222-225, :153). Two topologies, told apart
// by the tensor names:
//   rtdetr-l.yaml       HGNetv2 backbone, AIFI + CCFM encoder (model.0-27), RTDETRDecoder = model.28
//   yolov8-rtdetr.yaml  the YOLOv8 backbone + neck (model.0-21, yolo_trunk.hpp: the YOLOv8 detector's own trunk, under its storage
//                       conventions), RTDETRDecoder = model.22 on model.15 / 18 / 21
// Widths, class count and layer counts are read off the tensors.
//
// Convolutions (and the per-anchor linear layers, which are 1x1 convolutions on the three feature levels) run on the
// detector's MFMA kernels in the activation format of the run (split-f16x3 pair format by default, exact fp32 with
// fp32_split = 0); everything on AIFI's tokens and the decoder's 300 queries runs at exact fp32 (rtdetr_kernels.hpp).
#pragma once
#include "detector.hpp"
#include "rtdetr_kernels.hpp"

namespace gtx {

class RtDetr : public DetectorBase {
 public:
  RtDetr(gtx_ctx* ctx, const gtx_det_config& cfg);
  void finalize() override;
  // [nq][4 + nc]: xywh normalised to the frame + class scores of every query of image b (logits: the pre-sigmoid class logits)
  void raw_output(int b, float* out, int* n_anchors, bool logits = false) override;
  void layer_output(int b, const std::string& layer, float* out, int* h, int* w, int* c) override;
  void features(int, float*, int, int*, int*) const override { fail(-3, "RT-DETR: appearance vectors (obj_feats) are not implemented"); }
  void pad_skip(int* on, int* skipped, int* total) const override { if (on) *on = 0; if (skipped) *skipped = 0; if (total) *total = 0; }
  void sparse_box(int* on, int* overflows) const override { if (on) *on = 0; if (overflows) *overflows = 0; }

 private:
  // MAP: a plain map-side layer (convolution, depthwise convolution, 2x upsampling): the trunk's op, built by its builders, launched by
  // its run_op and accounted for by set_batch_op. The other kinds are the family's own.
  struct Op : OpInfo {
    enum Kind { MAP, STEM1, POOL2, TOKENS_IN, LINEAR, LAYERNORM, MHA, MASK, TOPK, GATHER, REFER, DEFORM } kind = MAP;
    gtx::Op map;                     // MAP (its OpInfo is the op's)
    RtMap a{}, b{};                  // map in / out
    const float* w = nullptr;        // STEM1 weights; LAYERNORM gamma
    const float* bias = nullptr;
    int level = 0, mode = 0;
    RtLinear lin{};                  // LINEAR (M = rows per image; scaled by the batch at launch)
    RtRows r_in{}, r_out{};          // LAYERNORM
    long rows = 0;                   // LAYERNORM: rows per image
    int C = 0, heads = 0, T = 0;     // LAYERNORM width / MHA
    const float* p0 = nullptr;       // TOKENS_IN pos; MHA qkv; REFER delta; DEFORM offaw; GATHER idx (int)
    float* p1 = nullptr;             // TOKENS_IN src; MHA out; REFER anchors; DEFORM out; GATHER embed
    float* p2 = nullptr;             // TOKENS_IN q; REFER refer; DEFORM refer; GATHER anchors
    int ld0 = 0, ld1 = 0;
    RtLevels lv{};                   // TOPK scores / GATHER enc / DEFORM values
    double img_flops = 0, img_bytes = 0;   // per image (set_batch scales them to the pass)
  };

  size_t op_count() const override { return ops_.size(); }
  const OpInfo& op_info(size_t i) const override { return ops_[i].kind == Op::MAP ? (const OpInfo&)ops_[i].map : ops_[i]; }
  void launch_op(size_t i, int nb, hipStream_t s) override { run_op(ops_[i], nb, s); }
  std::unique_ptr<NetRuntime> make_exact() const override;
  void release_graph() override { ops_.clear(); trunk_ops_.clear(); trunk_.clear(); }
  float* new_tokens(int rows_per_image, int ld, const std::string& name);
  // graph building
  View conv_raw(const std::string& name, const std::vector<float>& w_oihw, int cout, int cin, int ks, const float* bias_host, const View& x, int stride,
                int act, const View* out_slice, const View* residual, bool plain_out = false);
  View conv(const std::string& name, const View& x, int stride, int act, const View* out_slice = nullptr, const View* residual = nullptr);
  View conv2x2(const std::string& name, const View& x, const View* out_slice);
  View hg_cat(const std::string& pfx, int h, int w, int* c1);
  View hgblock(const std::string& pfx, const View& cat, int c1, bool shortcut, const View* out_slice);
  View repc3(const std::string& pfx, const View& x);
  float* linear(const std::string& name, const std::vector<float>& w, const std::vector<float>& bias, int nout, int k, const float* x, int ldx, const float* x2,
                int rows, int act, const float* res, int ldr, float* y, int ldy, const std::string& out_name);
  float* layernorm_tokens(const std::string& name, const float* x, int rows, int C, const std::string& out_name, const View* map_out = nullptr);
  void build_graph();
  void build_hgnet(View feats[3]);                  // rtdetr-l: HGStem .. CCFM; feats = model.21 / 24 / 27
  void build_decoder(const std::string& D, const View feats[3]);   // the RTDETRDecoder at prefix D on three maps, finest first
  void run_op(const Op& op, int nb, hipStream_t s);
  void run_post(int nb, hipStream_t s) override;
  void set_batch(int nb) override;

  // The trunk's builders (and emit_conv) append to trunk_ops_; what stands there from `first` on moves into ops_ at position `at`
  // as MAP ops. A layer of the family's own goes behind the ops before it at once (first = n_trunk_); the YOLOv8 trunk's n_trunk_ ops
  // stay until YoloTrunk::fuse() has rewritten them and then go in front.
  void adopt_map_ops(size_t first, size_t at);
  void adopt_map_ops() { adopt_map_ops(n_trunk_, ops_.size()); }

  std::vector<Op> ops_;
  bool yolo_ = false;                // yolov8-rtdetr.yaml: the YOLOv8 trunk
  std::vector<gtx::Op> trunk_ops_;
  size_t n_trunk_ = 0;
  YoloTrunk trunk_;
  int nh_ = 8, npts_ = 4, nq_ = 300, enc_heads_ = 8, hd_ = 256, nc_ = 0, ncp_ = 0, ndl_ = 0;

  // post stage
  const float* logits_ = nullptr;    // [N * nq][ncp]
  float* refer_ = nullptr;           // [N * nq][16]
  float* raw_ = nullptr;             // [N][nq][4 + nc]
  unsigned long long class_mask_[2] = {~0ull, ~0ull};
  float* out_rows_ = nullptr;
  int* out_n_ = nullptr;
};

}  // namespace gtx
