// The YOLO detector runtime (YOLOv8 / P2, YOLOv9, YOLOv10, YOLO11, YOLO26 `detect` checkpoints): builds the layer graph from
// ultralytics-named fused tensors -- the trunk through YoloTrunk, the Detect head through the builder in detect_head.cpp -- plans
// the NHWC buffers (concats are channel slices, never copies), and runs preprocess -> forward -> decode -> NMS (or the one-to-one
// head's top-300 cut) on a HIP stream. Stands in for what ultralytics' predictor does underneath model.track()
// (geotrax/extract.py:153).
#pragma once
#include <map>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "yolo_trunk.hpp"

namespace gtx {

// What the head builder passes between its steps (detect_head.cpp).
struct HeadConvOpts {        // how one head convolution is built
  int kc = 0, bn = 0;        // K chunk / cout tile forced on it (0: the kernel's own choice): a grouped stage's members share both
  bool plain = false;        // split-f16x3 path: it writes plain fp32 (stage 2, which the decode kernels read)
};
struct HeadLayer { Op op; View out; };   // one layer of the head: its op, held back from the op list, and its output
struct LevelHead {           // one Detect level, as either level builder returns it
  Op box1;                   // cv2[l][0]; the plain head stacks cv3[l][0] behind it (after plan_sparse_box: the class tiles alone)
  Op box2, cls2;             // cv2[l][1] and the class branch's last layer in front of its final 1x1: the two halves of `feat`
  bool dw_cls = false;       // yolo11.yaml's class branch, DWConv + 1x1 twice: dw_a -> pw_a -> dw_b -> cls2
  Op dw_a, pw_a, dw_b;
  View feat;                 // [cb + cc] channels: what the decode kernels read
  bool box1_in_pass = true, box2_in_pass = true;   // false: the sparse box branch evaluates it at the candidates instead
};

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
  // graph building (detect_head.cpp): the trunk (yolo_trunk.hpp), then the Detect head on its outputs, step by step
  void build_graph();
  std::pair<std::string, std::string> choose_head_pair();   // ".cv2." / ".cv3." or the one-to-one pair; sets end2end_
  HeadLayer head_conv(const std::string& name, const View& x, const HeadConvOpts& o, const View* out_slice = nullptr);
  HeadLayer head_dwconv(const std::string& name, const View& x);
  // b2 / b3: the level's box and class branch, "<det>.cv2.<l>" / "<det>.cv3.<l>"; x: its input; in_x32: every level's input is a multiple of 32 wide
  LevelHead build_plain_level(int l, const std::string& b2, const std::string& b3, const View& x, bool in_x32);
  LevelHead build_dw_cls_level(int l, const std::string& b2, const std::string& b3, const View& x, bool in_x32);
  void fill_decode_tail(int l, const std::string& b2, const std::string& b3, const LevelHead& h, float stride, int anchor_begin);
  bool sparse_box_applies(const std::vector<LevelHead>& lv) const;
  void plan_sparse_box(std::vector<LevelHead>& lv);
  void emit_head_stages(const std::vector<LevelHead>& lv);
  void set_feat_levels(const std::vector<View>& lvl_in);
  void alloc_level_lists(NmsBuffers& b, int cap);   // the sparse box branch's per-level candidate lists, cap entries each
  void run_op(const Op& op, int nb, hipStream_t s);
  void run_post(int nb, hipStream_t s) override;
  void after_pass(int nb) override;   // the overflow / large-NMS re-run and the appearance vectors' copy
  // the copies of r's counts and rows (sat: and of the saturation flag) to the pinned buffers; with obj_feats the vectors' launch and copy
  void read_back(const NmsBuffers& r, int nb, bool sat, hipStream_t s);
  void set_batch(int nb) override;

  int dtype_;                // activation type in HBM (DT_F16 / DT_F32); fmt_: what the conv kernels compute in (dtype_, or DT_F32S)
  size_t es_;
  std::vector<Op> ops_;
  YoloTrunk trunk_;          // emits the backbone + neck into ops_ and launches its ops

  HeadParams head_{};
  NmsBuffers nms_{};
  // gtx_det_config.end2end (yolov10.yaml's one-to-one head): the entries v10_select keeps (v10_select.hip) and its score scratch
  bool end2end_ = false;
  NmsBuffers sel_{};
  float* v10_scores_ = nullptr;
  static constexpr int kSelCap = 304;       // >= kV10Keep, whole groups of 16 for the sparse box branch
  DevBuf raw_;               // debug raw output
  FeatLevels feat_levels_{};
  // sparse box branch (head_sparse.hip): on for the split-f16x3 path when the head's layers have the 16x16x32 kernel's weight images
  static constexpr int kSparseCap = 8192;   // candidates per image its buffer holds
  bool sparse_on_ = false;
  SparseBox sparse_{};
  std::string det_pfx_ = "model.22";   // the Detect module: model.22 (yolov8.yaml), model.28 (yolov8-p2.yaml) or model.23
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
