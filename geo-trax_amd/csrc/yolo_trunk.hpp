// The YOLO trunk: everything in front of the Detect layer of ultralytics' yolov8.yaml (model.0-21), yolov8-p2.yaml (model.0-27) and
// yolo11.yaml / yolov10.yaml / yolo26.yaml (model.0-22), and the YOLOv8-cls (model.0-8) and YOLO11-cls (model.0-9) backbones. Each graph is a constant table with one row per yaml layer
// (yolo_trunk.cpp); one walk over a table emits its launches into the caller's op list. Every family that runs a trunk builds
// through it: the YOLOv8 / P2 / YOLO11 detector (Detect on its outputs, detect_head.cpp), YOLOv8-RTDETR (an RTDETRDecoder on model.15 /
// 18 / 21, rtdetr.cpp) and the ReID embedder (reid.cpp). It also owns the fused front (stem + model.1 + model.2.cv1 in one launch on
// the split-f16x3 path) with the stand-alone forms it hides, and launches its op kinds.
#pragma once
#include <string>
#include <vector>

#include "net_runtime.hpp"
#include "yolo_tables.hpp"

namespace gtx {

struct Op : OpInfo {
  enum Kind { CONV, STEM, POOL, UPSAMPLE, DWCONV, ATTN, POOLDOWN, AREAATTN, SCALEADD } kind = CONV;
  ConvGroup grp{};       // CONV
  ConvConfig cfg{};
  // STEM / POOL / UPSAMPLE parameters
  View in, out;
  const float* w27 = nullptr;        // the stem's weights, tap-major: [27][c0], or [108][c0] for stem_k = 6
  int stem_k = 3;                    // STEM: 3 (Conv 3x3 / 2 / pad 1) or 6 (yolov5.yaml's Conv 6x6 / 2 / pad 2, stem6.hpp)
  const float* bias = nullptr;
  const void* wpk = nullptr;   // fp16 MFMA / split-f16x3 stem weights
  float stem_scale = 1.f;      // split-f16x3 stem: inverse of the weights' power-of-two scaling
  const void* front_wpk = nullptr;   // the same weights packed for the front stage of model.1 (ConvProblem::front_w)
  float front_scale = 1.f;
  // DWCONV (depthwise dw_k x dw_k, stride dw_stride, on `in` -> `out`; act 0 none, 1 SiLU, 2 ReLU; dw_res: added after the activation when it
  // has a buffer) / ATTN (C2PSA's attention on the qkv map `in`, dw_w / dw_bias = its pe) / AREAATTN (AAttn's attention on the planar qkv
  // map `in`, cut into `area` bands; area_attn.hpp) / SCALEADD (A2C2f's residual: out = dw_res + dw_w[c] * in)
  const float* dw_w = nullptr;       // [k * k][C] tap-major
  const float* dw_bias = nullptr;
  int dw_act = 0, heads = 0, area = 0;
  int dw_k = 3, dw_stride = 1;
  View dw_res;
  View out2;                         // POOLDOWN (pool_down.hpp): `in` -> `out` (the 2x2 average) and, ADown, out2 (its 3x3 stride-2 maximum)
  int* sat = nullptr;                // the net's saturation flag (split-f16x3 path)
  // rows of the output that depend on the frame (Detector::plan_pad_skip), as tile rows per group member; count 0 = all
  int ty_first[kMaxGroup] = {0}, ty_count[kMaxGroup] = {0};
};

// N of a conv op (and the rows it computes) and the op's flops / bytes for a pass at batch nb (es: bytes per activation); every op of a list
void set_batch_op(Op& op, int nb, size_t es, bool pad_skip_on);
void set_batch_ops(std::vector<Op>& ops, int nb, size_t es, bool pad_skip_on);

class YoloTrunk {
 public:
  // dtype: the activation type in HBM (DT_F16 / DT_F32); the net's format (DT_F32S on the split path) is what the convs compute in
  YoloTrunk(NetRuntime& net, std::vector<Op>& ops, int dtype) : net_(net), ops_(ops), dtype_(dtype) {}

  struct Levels {
    std::vector<View> in;        // the Detect row's inputs, finest level first (a table without one: its last layer's output)
    std::vector<float> strides;  // net height / level height
    std::string det_pfx;         // the Detect row: model.22 (yolov8.yaml), model.28 (yolov8-p2.yaml) or model.23 (yolo11.yaml, yolov10.yaml, yolo26.yaml) or model.21 (yolo12.yaml) or model.24 (yolov5.yaml)
    bool dw_cls = false;         // TrunkGraph::dw_cls
  };
  // The graph the tensors were built from, by their names: yolov5.yaml, yolo12.yaml, yolov10.yaml, yolo26.yaml, yolo11.yaml, yolov9.yaml, yolov8-p2.yaml, else yolov8.yaml
  TrunkGraph choose_graph() const;
  static TrunkGraph cls_backbone();   // model.0-8 of yolov8.yaml = yolov8-cls.yaml's backbone
  // The classification graph the tensors were built from: yolo11-cls.yaml (model.0-8 of yolo11.yaml + C2PSA = model.9), else cls_backbone()
  TrunkGraph choose_cls_graph() const;
  // Emits every row of g in front of its Detect on img ([N][H][W][4] RGB0 bytes). front: the stem also gets its weights packed for
  // fuse() (a net that never calls fuse() passes false).
  Levels build(const View& img, const TrunkGraph& g, bool front = true);
  Levels build(const View& img) { return build(img, choose_graph()); }
  // One Conv op (SiLU). up_src: the leading up_src->c channels of x are the 2x nearest upsampling of *up_src and are read from
  // there (split-f16x3 1x1 convs; ConvProblem::in2) -- the slice of x they would occupy is never written.
  View conv(const std::string& name, const View& x, int stride, const View* out_slice, const View* residual = nullptr,
            const View* up_src = nullptr);
  // After the whole graph is built: fuse_front, fuse_stem, then the buffers only the stand-alone forms of fused layers write go back.
  void fuse();
  void run_op(const Op& op, int nb, hipStream_t s) const;
  // layer_output of a layer the fused launches do not write (the stem's output, model.1's): its buffer is re-created and the
  // stand-alone launches run up to it on the input of the last pass (nb images). False for every other layer.
  bool recompute_hidden(const std::string& layer, int nb, hipStream_t s);
  // p is the placeholder of a released buffer that no layer_output() has re-created yet (no device address)
  bool hidden(const void* p) const;
  void clear() { unfused_.clear(); hidden_.clear(); }
  // Depthwise convolution "<name>.weight" [C][1][k][k] (+ bias), k = 3, 5 or 7 read off the tensor, stride 1 or 2 (2: k = 3), act 0 none, 1 SiLU,
  // 2 ReLU (YOLO11's DWConv, used by its Detect; YOLOv10's SCDown and CIB; rtdetr-l's DWConv and LightConv). out_slice: where it writes
  // (null: a view of its own); residual: added after the activation
  View dwconv(const std::string& name, const View& x, int act, int stride = 1, const View* out_slice = nullptr, const View* residual = nullptr);
  void upsample(const std::string& name, const View& src, const View& dst);   // nearest 2x of src into dst, a channel slice

 private:
  View stem(const View& img, bool front);
  View stem6(const View& img);                                                                                   // yolov5.yaml's 6x6 stem
  void read_upsampled(Op& op, const View& x, const View& up_src);
  View c3(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src);    // yolov5.yaml's C3
  View c2f(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src);   // C2f and C3k2
  // one stride-1 Conv op with activation `act`; channel counts that are no multiple of 16 are zero-padded (YOLO11-n's 8-channel hidden layer).
  // in_seg > 0: x is segments of in_seg channels, each followed by its zero padding up to a multiple of 16 (a concat of padded maps)
  View conv_act(const std::string& name, const View& x, int act, const View* out_slice, const View* residual, int in_seg = 0);
  View bottleneck(const std::string& m, const View& src, const View& dst, bool shortcut);
  View c3k(const std::string& m, const View& src, const View& dst, bool shortcut);
  View c2psa(const std::string& pfx, const View& x, const View* out_slice, bool bare = false);   // bare: PSA, the one block's tensors directly under pfx
  // A2C2f (yolo12.yaml): members of two ABlocks cut into `area` bands, or of one C3k (c3k_shortcut) each -- the tensors tell which
  View a2c2f(const std::string& pfx, const View& x, int area, bool c3k_shortcut, const View* out_slice, const View* up_src);
  void ablock(const std::string& m, const View& x, const View& dst, int area);                  // one ABlock: x + AAttn(x), then + mlp
  void psa_block(const std::string& m, const View& b, const View& dst);                         // one PSABlock (C2PSA's, PSA's, the C3k2 with attention's)
  View cib(const std::string& m, const View& src, const View& dst, bool shortcut);
  View scdown(const std::string& pfx, const View& x, const View* out_slice);
  View elan(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src);   // ELAN1 and RepNCSPELAN4
  View adown(const std::string& pfx, const View& x, const View* out_slice);                                     // AConv and ADown
  // SPPELAN: last = ".cv5.conv"; linear_res: yolo26.yaml's SPPF (cv1 without activation, x added to the output)
  void sppf(const std::string& pfx, const View& x, const View& out, const char* last = ".cv2.conv", bool linear_res = false);
  void fuse_front();         // model.1 (3x3 stride 2) + model.2.cv1 (1x1) as one launch on the split-f16x3 path
  void fuse_stem();          // model.0 (the stem) computed inside model.1's launch: its output never reaches HBM
  void release_hidden_layers();
  void materialize_hidden_layers();

  NetRuntime& net_;
  std::vector<Op>& ops_;
  int dtype_;
  std::vector<Op> unfused_;  // the stand-alone forms of fused ops (layer_output of an intermediate runs them on demand)
  struct Hidden { void* token; size_t bytes; void* real; };
  std::vector<Hidden> hidden_;
};

}  // namespace gtx
