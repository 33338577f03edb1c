// YOLOv8 detector runtime: builds the layer graph from ultralytics-named fused tensors, plans
// the NHWC buffers (concats are channel slices, never copies), and runs
// preprocess -> forward -> decode -> NMS on a HIP stream. Stands in for what
// ultralytics' predictor does underneath model.track() (geotrax/extract.py:153).
#pragma once
#include <map>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "yolo_trunk.hpp"

namespace gtx {

class Detector : public DetectorBase {
 public:
  Detector(gtx_ctx* ctx, const gtx_det_config& cfg);
  ~Detector() override;
  void finalize() override;
  void raw_output(int b, float* out, int* n_anchors, bool logits = false) override;
  void layer_output(int b, const std::string& layer, float* out, int* h, int* w, int* c) override;
  // gtx_det_config::obj_feats: appearance vectors of image b's boxes of the most recently collected batch, [n][dim] (n = its box count)
  void features(int b, float* out, int cap, int* n, int* dim) const override;
  void pad_skip(int* on, int* skipped, int* total) const override {
    if (on) *on = (!exact_ && pad_skip_on_) ? 1 : 0;
    if (skipped) *skipped = pad_skip_rows_;
    if (total) *total = pad_skip_total_;
  }
  void sparse_box(int* on, int* overflows) const override {
    if (on) *on = (!exact_ && sparse_on_) ? 1 : 0;
    if (overflows) *overflows = sparse_overflows_;
  }

 private:
  size_t op_count() const override { return ops_.size(); }
  const OpInfo& op_info(size_t i) const override { return ops_[i]; }
  void launch_op(size_t i, int nb, hipStream_t s) override { run_op(ops_[i], nb, s); }
  std::unique_ptr<NetRuntime> make_exact() const override;
  void release_graph() override { ops_.clear(); trunk_.clear(); }
  // graph building: the trunk (yolo_trunk.hpp), then the Detect head on its outputs
  View head_conv(const std::string& name, const View& x, const View* out_slice);
  void build_graph();
  void run_op(const Op& op, int nb, hipStream_t s);
  void run_post(int nb, hipStream_t s) override;
  void after_pass(int nb) override;   // the overflow / large-NMS re-run and the appearance vectors' copy
  void set_batch(int nb) override;

  int dtype_;                // activation type in HBM (DT_F16 / DT_F32); fmt_: what the conv kernels compute in (dtype_, or DT_F32S)
  size_t es_;
  std::vector<Op> ops_;
  YoloTrunk trunk_;          // emits the backbone + neck into ops_ and launches its ops
  int force_kc_ = 0;         // K chunk forced on the convs being built (grouped head stages)
  int force_bn_ = 0;         // cout tile forced on them

  HeadParams head_{};
  NmsBuffers nms_{};
  // gtx_det_config.end2end (yolov10.yaml's one-to-one head): the entries v10_select keeps (v10_select.hip) and its score scratch
  bool end2end_ = false;
  NmsBuffers sel_{};
  float* v10_scores_ = nullptr;
  static constexpr int kSelCap = 304;       // >= kV10Keep, whole groups of 16 for the sparse box branch
  DevBuf raw_;               // debug raw output
  bool plain_out_ = false;   // convs being built write plain fp32 (head stage 2)
  FeatLevels feat_levels_{};
  // sparse box branch (head_sparse.hip): on for the split-f16x3 path when the head's layers have the 16x16x32 kernel's weight images
  static constexpr int kSparseCap = 8192;   // candidates per image its buffer holds
  bool sparse_on_ = false;
  SparseBox sparse_{};
  Op head_ops_[kMaxLevels][3];
  std::string det_pfx_ = "model.22";   // the Detect module: model.22 (yolov8.yaml) or model.28 (yolov8-p2.yaml)
  std::vector<Op> dense_box_ops_;
  bool dense_head_valid_ = false;
  int* h_count_ = nullptr;   // pinned: candidates per image of the pass in flight
  int sparse_overflows_ = 0;
  void run_dense_box(hipStream_t s);
  // letterbox-padding rows: activations there do not depend on the frame; computed once (finalize), skipped afterwards
  bool pad_skip_on_ = false;
  int pad_skip_rows_ = 0, pad_skip_total_ = 0;   // tile rows skipped / planned over all convolution launches (for the report)
  void plan_pad_skip();
  void prime_pad_skip();
  float* d_feats_ = nullptr;  // [max_batch][max_det][dim]
  float* h_feats_ = nullptr;  // pinned
  std::vector<float> c_feats_;   // the collected batch's vectors
  std::vector<int> c_feat_n_;
};

}  // namespace gtx
