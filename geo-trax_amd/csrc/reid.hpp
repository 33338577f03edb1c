// Separate ReID network: the YOLOv8-cls backbone (model.0 - model.8 of ultralytics' yolov8-cls.yaml) or the YOLO11-cls one (model.0 -
// model.9 of yolo11-cls.yaml: C3k2 blocks, then C2PSA) run over one crop per detection, its last map average-pooled into one vector per crop. Stands in for ultralytics' trackers/bot_sort.py ReID
// (`with_reid: true, model: <cls checkpoint>` of BoT-SORT, Deep OC-SORT and TrackTrack; geotrax/cfg/default.yaml:379, :421, :470):
// save_one_box per detection -> ClassificationPredictor (classify_transforms(imgsz)) -> model(embed=[len(model) - 2]).
// The graph is the YOLO trunk's (yolo_trunk.hpp: the backbone rows of its yolov8.yaml table) with the batch dimension equal to the
// number of crops; the Classify head is never run.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "detector.hpp"
#include "reid_kernels.hpp"

namespace gtx {

// save_one_box(xyxy, im, gain=1.02, pad=10, square=False) of one detection: the clipped crop [x1, x2) x [y1, y2) of an h x w frame
void reid_crop_box(const float xyxy[4], int h, int w, int out[4]);

class Embedder : public NetRuntime {
 public:
  Embedder(gtx_ctx* ctx, int imgsz, int max_crops, bool fp32_split);
  ~Embedder() override;
  // the calls that run or read a pass go here: the exact-fp32 twin once a split-f16x3 pass has saturated
  Embedder* live() { return live_as<Embedder>(); }
  void finalize() override;
  int dim() const { return dim_; }
  // frames: nb device frames [h][w][3] BGR u8; counts[nb] boxes per frame, xyxy [sum counts][4] host, frame pixels
  void submit_dev(const void* frames, int nb, int h, int w, const int* counts, const float* xyxy);
  // waits for the submitted pass; out [n][dim] (n = the pass's box count, <= cap)
  int collect(float* out, int cap);
  void crops(int i, uint8_t* out);                                          // [S][S][4] u8 of crop i of the last pass
  void layer_output(int i, const std::string& layer, float* out, int* h, int* w, int* c);
  // per-op times of `iters` forward passes over the first n crops of the last pass (events around every launch)
  void profile(int n, int iters, std::vector<std::string>& names, std::vector<float>& ms, std::vector<double>& flops);

 private:
  size_t op_count() const override { return ops_.size(); }
  const OpInfo& op_info(size_t i) const override { return ops_[i]; }
  void launch_op(size_t i, int nb, hipStream_t s) override { trunk_.run_op(ops_[i], nb, s); }
  std::unique_ptr<NetRuntime> make_exact() const override;
  void release_graph() override { ops_.clear(); }
  void build_graph();
  void set_batch(int nb) override;
  void enqueue(int n_total);

  int S_;
  std::vector<Op> ops_;
  YoloTrunk trunk_;          // builds the classifier's rows (YoloTrunk::choose_cls_graph) into ops_ and launches them
  View img_, last_;
  int dim_ = 0;
  // the pass in flight (kept for the exact re-run of a saturated pass)
  bool in_flight_ = false;
  const void* cur_frames_ = nullptr;
  int cur_h_ = 0, cur_w_ = 0;
  std::vector<int> cur_counts_;
  std::vector<float> cur_xyxy_;
  int n_flight_ = 0, last_chunk_ = 0, last_chunk_n_ = 0;
  // per-pass crop table + coefficient pool (pinned staging, device copies) and the vectors
  std::vector<ReidCrop> h_crops_;
  std::vector<int> h_pool_;
  void* pin_ = nullptr; size_t pin_bytes_ = 0;
  DevBuf d_params_;
  DevBuf d_emb_;
  float* h_emb_ = nullptr; size_t h_emb_n_ = 0;
  hipEvent_t done_ = nullptr;
};

}  // namespace gtx

struct gtx_embedder {
  std::unique_ptr<gtx::Embedder> impl;
};
