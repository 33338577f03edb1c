// The Detect head's builder. Detector::build_graph() is a sequence of steps; each takes what it needs as arguments and returns
// what it built. Channel widths are read off the tensor shapes, so every scale (n / s / m / l / x) builds unchanged.
//   1. the trunk (yolo_trunk.cpp) up to the Detect row's inputs
//   2. choose_head_pair: cv2 / cv3, or a YOLOv10 / YOLO26 checkpoint's one-to-one pair (gtx_det_config.end2end)
//   3. per level build_plain_level or build_dw_cls_level (yolo11.yaml's depthwise class branch): both return a LevelHead, whose
//      ops are named where they are created and enter the op list only in step 6
//   4. fill_decode_tail: the final 1x1 convs, folded into the decode kernels (HeadLevel), with the checks on widths and reg_max
//   5. sparse_box_applies / plan_sparse_box: whether, and how, the box layers run at the score gate's candidates only
//   6. emit_head_stages: the levels of a stage as one grouped launch per kernel configuration
//   7. set_feat_levels: the Detect inputs, for obj_feats
#include "detector.hpp"

#include <algorithm>

namespace gtx {

namespace {

bool all_multiples_of(int m, std::initializer_list<int> widths) {
  return std::all_of(widths.begin(), widths.end(), [m](int w) { return w % m == 0; });
}

// The tile rule of a grouped stage, whose members all run one kernel instantiation: K chunk 32 only if every member's Cin is a
// multiple of 32 (cin_x32; yolov8 n / m / x have widths that are multiples of 16 only), else 16; cout tile 64 only if every
// member's Cout is a multiple of 64, else 32. Only the fp16 kernels take a K chunk from outside.
HeadConvOpts head_tile(int fmt, bool cin_x32, std::initializer_list<int> couts, bool plain = false) {
  return HeadConvOpts{fmt == DT_F16 ? (cin_x32 ? 32 : 16) : 0, all_multiples_of(64, couts) ? 64 : 32, plain};
}

// Tensor b's rows behind a's: the weights / bias of two sibling convs as one conv's
HostTensor stacked(const HostTensor& a, const HostTensor& b) {
  HostTensor t = a;
  t.shape[0] += b.shape[0];
  t.data.insert(t.data.end(), b.data.begin(), b.data.end());
  return t;
}

// o joins the launch of `stage` that runs its kernel and has room, or opens the stage's next one ("<name>", "<name>.1", ...)
void group_op(std::vector<Op>& stage, const std::string& name, const Op& o) {
  for (Op& g : stage)
    if (same_kernel(g.cfg, o.cfg) && g.grp.count < kMaxGroup) { g.grp.p[g.grp.count++] = o.grp.p[0]; return; }
  Op g;
  g.kind = Op::CONV;
  g.name = stage.empty() ? name : name + "." + std::to_string(stage.size());
  g.family = conv_kernel_name(o.cfg);
  g.cfg = o.cfg;
  g.grp.p[g.grp.count++] = o.grp.p[0];
  stage.push_back(g);
}

}  // namespace

// v10Detect holds Detect's layers twice: cv2 / cv3 (one-to-many, followed by NMS) and one2one_cv2 / one2one_cv3 (followed by the
// top-300 cut, v10_select.hip). gtx_det_config.end2end picks the pair; the other pair's tensors are not read.
std::pair<std::string, std::string> Detector::choose_head_pair() {
  const bool has_o2o = has(det_pfx_ + ".one2one_cv2.0.0.conv.weight");
  end2end_ = cfg_.end2end != 0;
  GTX_CHECK(!end2end_ || has_o2o, "end2end: the checkpoint has no one-to-one head (%s.one2one_cv2 / one2one_cv3): only a YOLOv10 or YOLO26 file has", det_pfx_.c_str());
  GTX_CHECK(!end2end_ || !cfg_.obj_feats, "end2end: obj_feats (ReID `model: auto`) is not implemented for the one-to-one head");
  const std::string box_br = end2end_ ? ".one2one_cv2." : ".cv2.", cls_br = end2end_ ? ".one2one_cv3." : ".cv3.";
  GTX_CHECK(has(det_pfx_ + box_br + "0.0.conv.weight") && has(det_pfx_ + cls_br + "0.2.weight"),
            "%s: the checkpoint holds no %s / %s tensors (a fused YOLOv10 / YOLO26 export keeps the one-to-one head only: run it with end2end)", det_pfx_.c_str(),
            box_br.substr(1, box_br.size() - 2).c_str(), cls_br.substr(1, cls_br.size() - 2).c_str());
  return {box_br, cls_br};
}

// One Conv op of the head from the tensors "<name>.*"; out_slice: where it writes (null: a view of its own)
HeadLayer Detector::head_conv(const std::string& name, const View& x, const HeadConvOpts& o, const View* out_slice) {
  ConvArgs a;
  a.out_slice = out_slice;
  a.plain_out = fmt_ == DT_F32S && o.plain;
  a.force_kc = o.kc; a.force_bn = o.bn;
  std::vector<Op> one;
  const View out = emit_named_conv(one, name, x, a);
  return HeadLayer{one.back(), out};
}

// One DWConv (3x3, SiLU) of the head. The trunk emits into the op list: the op is taken back here, where it was created.
HeadLayer Detector::head_dwconv(const std::string& name, const View& x) {
  const View out = trunk_.dwconv(name, x, 1);
  HeadLayer layer{ops_.back(), out};
  ops_.pop_back();
  return layer;
}

// yolov8.yaml's Detect level: stage 1 fuses the sibling convs cv2[l][0] and cv3[l][0] (same input) into one conv by stacking
// their output channels; stage 2 runs cv2[l][1] and cv3[l][1] on its channel slices and writes the two halves of `feat`.
LevelHead Detector::build_plain_level(int l, const std::string& b2, const std::string& b3, const View& x, bool in_x32) {
  const HostTensor &w20 = tensor(b2 + ".0.conv.weight"), &w30 = tensor(b3 + ".0.conv.weight");
  const int cb = (int)w20.shape[0], cc = (int)w30.shape[0];
  GTX_CHECK((int)w20.shape[1] == x.c && (int)w30.shape[1] == x.c, "Detect level %d input channels", l);
  const std::string s1 = "__head" + std::to_string(l) + ".s1";
  tensors_[s1 + ".weight"] = stacked(w20, w30);
  tensors_[s1 + ".bias"] = stacked(tensor(b2 + ".0.conv.bias"), tensor(b3 + ".0.conv.bias"));
  LevelHead h;
  const HeadLayer st1 = head_conv(s1, x, head_tile(fmt_, in_x32, {cb + cc}));
  h.box1 = st1.op;
  h.feat = new_view(st1.out.h, st1.out.w, cb + cc);
  const View fb = h.feat.slice(0, cb), fc = h.feat.slice(cb, cc);
  const HeadConvOpts t2 = head_tile(fmt_, all_multiples_of(32, {cb, cc}), {cb, cc}, true);
  h.box2 = head_conv(b2 + ".1.conv", st1.out.slice(0, cb), t2, &fb).op;
  h.cls2 = head_conv(b3 + ".1.conv", st1.out.slice(cb, cc), t2, &fc).op;
  h.feat.plain = fmt_ == DT_F32S;
  return h;
}

// yolo11.yaml's Detect level (YOLOv10's and YOLO26's too): the box branch as above but on its own -- cv2[l][0] is a launch of one
// 64-cout tile, the sparse box branch's image -- and a class branch of DWConv 3x3 + Conv 1x1, twice.
LevelHead Detector::build_dw_cls_level(int l, const std::string& b2, const std::string& b3, const View& x, bool in_x32) {
  const HostTensor& w20 = tensor(b2 + ".0.conv.weight");
  const int cb = (int)w20.shape[0], cc = (int)tensor(b3 + ".1.1.conv.weight").shape[0];
  GTX_CHECK((int)w20.shape[1] == x.c, "Detect level %d input channels", l);
  LevelHead h;
  h.dw_cls = true;
  h.feat = new_view(x.h, x.w, cb + cc);
  const View fb = h.feat.slice(0, cb), fc = h.feat.slice(cb, cc);
  const HeadLayer box1 = head_conv(b2 + ".0.conv", x, head_tile(fmt_, in_x32, {cb}));
  h.box1 = box1.op;
  h.box2 = head_conv(b2 + ".1.conv", box1.out, head_tile(fmt_, cb % 32 == 0, {cb}, true), &fb).op;
  const HeadLayer dw_a = head_dwconv(b3 + ".0.0.conv", x);
  const HeadLayer pw_a = head_conv(b3 + ".0.1.conv", dw_a.out, head_tile(fmt_, in_x32, {cc}));
  const HeadLayer dw_b = head_dwconv(b3 + ".1.0.conv", pw_a.out);
  h.cls2 = head_conv(b3 + ".1.1.conv", dw_b.out, head_tile(fmt_, cc % 32 == 0, {cc}, true), &fc).op;
  h.dw_a = dw_a.op; h.pw_a = pw_a.op; h.dw_b = dw_b.op;
  h.feat.plain = fmt_ == DT_F32S;
  return h;
}

// The decode kernels' side of level l: its map, stride and first anchor, and the final 1x1 convs cv2[l][2] / cv3[l][2], which
// are folded into them (the box one only runs for anchors that pass the score gate).
void Detector::fill_decode_tail(int l, const std::string& b2, const std::string& b3, const LevelHead& h, float stride, int anchor_begin) {
  const int cb = h.box2.grp.p[0].Cout, cc = h.cls2.grp.p[0].Cout;
  const HostTensor &wb = tensor(b2 + ".2.weight"), &wc = tensor(b3 + ".2.weight");
  // reg_max off the last box convolution's rows: 4 x 16 DFL bins, or yolo26.yaml's four distances (reg_max = 1)
  const int box_out = (int)wb.shape[0];
  GTX_CHECK((box_out == 64 || box_out == 4) && (int)wb.shape[1] == cb, "Detect box head must have 4*16 outputs, or 4 (reg_max = 1); it has %d", box_out);
  GTX_CHECK(l == 0 || head_.reg_max == box_out / 4, "Detect box branch: reg_max differs between levels");
  head_.reg_max = box_out / 4;
  GTX_CHECK(cb <= 128 && cc % 8 == 0, "Detect head widths cb=%d cc=%d are outside what the decode kernels support", cb, cc);
  GTX_CHECK(l == 0 || cb == head_.lv[0].cb, "Detect box branch width differs between levels");
  GTX_CHECK((int)wc.shape[0] == cfg_.nc && (int)wc.shape[1] == cc, "Detect cls head has %d outputs, nc=%d", (int)wc.shape[0], cfg_.nc);
  HeadLevel& L = head_.lv[l];
  L.feat = h.feat.ptr; L.h = h.feat.h; L.w = h.feat.w; L.cstride = h.feat.cstride; L.cb = cb; L.cc = cc;
  L.stride = stride; L.anchor_begin = anchor_begin;
  std::vector<float> wbt((size_t)cb * box_out);    // [cb][64]: the decode wave reads one output per lane; reg_max = 1: [cb][4]
  for (int o = 0; o < box_out; ++o)
    for (int k = 0; k < cb; ++k) wbt[(size_t)k * box_out + o] = wb.data[(size_t)o * cb + k];
  L.wb = upload(wbt); L.bb = upload(tensor(b2 + ".2.bias").data);
  L.wc = upload(wc.data); L.bc = upload(tensor(b3 + ".2.bias").data);
  layer_views_[det_pfx_ + ".feat" + std::to_string(l)] = h.feat;
}

// The sparse box branch needs the 16x16x32 kernel's image of both box layers (32-channel chunks, one 64-cout box tile) on every
// level: decided for all levels at once. GTX_SPARSE_BOX=0: off.
bool Detector::sparse_box_applies(const std::vector<LevelHead>& lv) const {
  bool on = fmt_ == DT_F32S && env_flag("GTX_SPARSE_BOX", true);
  for (size_t l = 0; l < lv.size(); ++l) {
    const Op &b1 = lv[l].box1, &b2 = lv[l].box2;
    on = on && head_.lv[l].cb == 64 && b1.cfg.variant == ConvForm::K32 && b1.cfg.bn == 64 && b2.cfg.variant == ConvForm::K32 && b1.grp.p[0].Cin % 32 == 0;
  }
  return on;
}

// Sparse box branch (head_sparse.hip): the box half of stage 1 (cout tile 0 of the stacked image) and cv2[l][1] are evaluated at
// the candidate anchors only, after the score gate. Fills sparse_ and keeps the dense box layers (dense_box_ops_) for the debug
// read-backs and the overflow case; stage 1 keeps its class half (cout tiles 1..): same packed image, same scale.
void Detector::plan_sparse_box(std::vector<LevelHead>& lv) {
  std::vector<Op> d1, d2;
  for (size_t l = 0; l < lv.size(); ++l) {
    LevelHead& h = lv[l];
    const HeadLevel& L = head_.lv[l];
    const ConvProblem full = h.box1.grp.p[0], &p2 = h.box2.grp.p[0];
    GTX_CHECK(full.bias && p2.bias && p2.Cin == 64 && p2.Cout == 64, "sparse box branch: unexpected Detect box layers");
    SparseBoxLevel& S = sparse_.lv[l];
    S.in = full.in; S.H = full.H; S.W = full.W; S.cstride = full.in_cstride; S.coff = full.in_coff; S.cin = full.Cin;
    S.w1 = full.wpack; S.b1 = full.bias; S.sc1 = full.acc_scale;
    S.w2 = p2.wpack; S.b2 = p2.bias; S.sc2 = p2.acc_scale;
    S.wb = L.wb; S.bb = L.bb; S.stride = L.stride; S.anchor_begin = L.anchor_begin;
    Op box_tile = h.box1;                          // the box tile alone
    box_tile.grp.p[0].Cout = L.cb;
    group_op(d1, det_pfx_ + ".box1", box_tile);
    group_op(d2, det_pfx_ + ".box2", h.box2);
    h.box2_in_pass = false; h.box1_in_pass = !h.dw_cls;   // the depthwise head's stage 1 holds no class tile
    if (h.dw_cls) continue;
    ConvProblem& p = h.box1.grp.p[0];              // the class tiles alone
    p.wpack = static_cast<const char*>(full.wpack) + (size_t)(full.Cin / h.box1.cfg.kc) * 9 * 64 * 128;   // past one 64-cout tile of the packed image
    p.bias = full.bias + 64; p.Cout = L.cc; p.out_coff = full.out_coff + L.cb;
  }
  sparse_.n_levels = (int)lv.size(); sparse_.reg_max = head_.reg_max;
  dense_box_ops_ = d1;
  dense_box_ops_.insert(dense_box_ops_.end(), d2.begin(), d2.end());
}

// The levels (three, four with P2) go out as one grouped launch per stage and kernel configuration: the levels of a stage share a
// launch when they share the kernel. A stage's depthwise layers go in front of the launches that read them.
void Detector::emit_head_stages(const std::vector<LevelHead>& lv) {
  std::vector<Op> st1, st2;
  for (const LevelHead& h : lv) {
    if (h.dw_cls) group_op(st1, det_pfx_ + ".stage1", h.pw_a);
    if (h.box1_in_pass) group_op(st1, det_pfx_ + ".stage1", h.box1);
    if (h.box2_in_pass) group_op(st2, det_pfx_ + ".stage2", h.box2);
    group_op(st2, det_pfx_ + ".stage2", h.cls2);
  }
  for (const LevelHead& h : lv) if (h.dw_cls) ops_.push_back(h.dw_a);
  ops_.insert(ops_.end(), st1.begin(), st1.end());
  for (const LevelHead& h : lv) if (h.dw_cls) ops_.push_back(h.dw_b);
  ops_.insert(ops_.end(), st2.begin(), st2.end());
}

// `with_reid: true, model: auto`: the Detect layer's inputs, read after NMS at the kept boxes' anchors
void Detector::set_feat_levels(const std::vector<View>& lvl_in) {
  feat_levels_ = FeatLevels{};
  if (!cfg_.obj_feats) return;
  const int nl = (int)lvl_in.size();
  feat_levels_.n_levels = nl; feat_levels_.dim = lvl_in[0].c;
  for (int l = 1; l < nl; ++l) feat_levels_.dim = std::min(feat_levels_.dim, lvl_in[l].c);
  for (int l = 0; l < nl; ++l) {
    feat_levels_.feat[l] = lvl_in[l].ptr; feat_levels_.h[l] = lvl_in[l].h; feat_levels_.w[l] = lvl_in[l].w;
    feat_levels_.cstride[l] = lvl_in[l].cstride; feat_levels_.coff[l] = lvl_in[l].coff; feat_levels_.c[l] = lvl_in[l].c;
    feat_levels_.anchor_begin[l] = head_.lv[l].anchor_begin;
    GTX_CHECK(lvl_in[l].c % feat_levels_.dim == 0, "obj_feats: Detect input %d has %d channels, not a multiple of %d", l, lvl_in[l].c, feat_levels_.dim);
  }
}

void Detector::build_graph() {
  img_ = new_view(lb_.net_h, lb_.net_w, 4);
  alloc_sat_flag();
  const YoloTrunk::Levels trunk = trunk_.build(img_);   // trunk.in: the Detect layer's inputs, finest level first
  det_pfx_ = trunk.det_pfx;
  const int nl = (int)trunk.in.size();
  GTX_CHECK(nl <= kMaxLevels, "internal: %d Detect levels", nl);
  const std::pair<std::string, std::string> br = choose_head_pair();
  head_ = HeadParams{};
  head_.n_levels = nl; head_.nc = cfg_.nc; head_.conf = cfg_.conf;
  head_.class_mask[0] = head_.class_mask[1] = cfg_.n_classes == 0 ? ~0ull : 0ull;
  for (int i = 0; i < cfg_.n_classes; ++i)
    if (cfg_.classes[i] >= 0 && cfg_.classes[i] < 128) head_.class_mask[cfg_.classes[i] >> 6] |= 1ull << (cfg_.classes[i] & 63);
  bool in_x32 = true;                              // stage 1 of every level shares one K chunk
  for (const View& x : trunk.in) in_x32 = in_x32 && x.c % 32 == 0;
  std::vector<LevelHead> lv;
  int anchor = 0;
  for (int l = 0; l < nl; ++l) {
    const std::string b2 = det_pfx_ + br.first + std::to_string(l), b3 = det_pfx_ + br.second + std::to_string(l);
    lv.push_back(trunk.dw_cls ? build_dw_cls_level(l, b2, b3, trunk.in[l], in_x32) : build_plain_level(l, b2, b3, trunk.in[l], in_x32));
    fill_decode_tail(l, b2, b3, lv[l], trunk.strides[l], anchor);
    anchor += lv[l].feat.h * lv[l].feat.w;
  }
  head_.n_anchors = anchor;
  GTX_CHECK(end2end_ || anchor <= nms_max_anchors(), "%d anchors per image: the NMS kernels order at most %d (ties between candidates go to the lower anchor)", anchor,
            nms_max_anchors());
  sparse_ = SparseBox{};
  sparse_on_ = sparse_box_applies(lv);
  if (sparse_on_) plan_sparse_box(lv);
  emit_head_stages(lv);
  set_feat_levels(trunk.in);
}

}  // namespace gtx
