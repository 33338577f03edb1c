// YOLOv8 / YOLO11 / YOLOv10 / YOLO26 (detect) graph builder + executor: the trunk (yolo_trunk.cpp walks the layer table of ultralytics' cfg/models/v8/yolov8.yaml,
// yolov8-p2.yaml or cfg/models/11/yolo11.yaml, whichever the tensor names tell) and the Detect layer on the levels, strides and prefix the
// table's Detect row gives (model.22, model.28 of the P2 graph: a fourth level at stride 4, or model.23 of YOLO11 and YOLOv10: a class branch of
// depthwise + pointwise pairs; YOLOv10's and YOLO26's one-to-one pair of branches ends in the top-300 cut of v10_select.hip instead of the NMS; YOLO26's box branch has reg_max = 1, four signed distances instead of 4 x 16 DFL bins, read off its last 1x1's row count); channel widths and bottleneck counts are read off the tensor shapes, so every scale (n/s/m/l/x) loads unchanged.
#include "detector.hpp"
#include "split_format.hpp"

#include <algorithm>
#include <cmath>

namespace gtx {

Detector::Detector(gtx_ctx* ctx, const gtx_det_config& cfg)
    : DetectorBase(ctx, cfg, cfg.half ? DT_F16 : (cfg.fp32_split ? DT_F32S : DT_F32), dtype_size(cfg.half ? DT_F16 : DT_F32),
                   cfg.half ? DT_F16 : DT_F32),
      trunk_(*this, ops_, cfg.half ? DT_F16 : DT_F32) {
  dtype_ = cfg.half ? DT_F16 : DT_F32;
  es_ = dtype_size(dtype_);
  lb_ = letterbox_geometry(cfg.frame_h, cfg.frame_w, cfg.imgsz, cfg.rect != 0, 32);
  GTX_CHECK(lb_.net_h % 32 == 0 && lb_.net_w % 32 == 0, "network input %dx%d is not stride aligned", lb_.net_h, lb_.net_w);
}

Detector::~Detector() {
  if (h_feats_) (void)hipHostFree(h_feats_);
  if (h_count_) (void)hipHostFree(h_count_);
}

std::unique_ptr<NetRuntime> Detector::make_exact() const {
  gtx_det_config c = cfg_;
  c.fp32_split = 0;
  return std::unique_ptr<NetRuntime>(new Detector(ctx_, c));
}

// One Conv op of the Detect head, with the grouped stages' K chunk / cout tile / plain output in force
View Detector::head_conv(const std::string& name, const View& x, const View* out_slice) {
  ConvArgs a;
  a.out_slice = out_slice;
  a.plain_out = fmt_ == DT_F32S && plain_out_;
  a.force_kc = force_kc_; a.force_bn = force_bn_;
  return emit_named_conv(ops_, name, x, a);
}

void Detector::build_graph() {
  const int H = lb_.net_h, W = lb_.net_w;
  img_ = new_view(H, W, 4);
  alloc_sat_flag();
  const YoloTrunk::Levels trunk = trunk_.build(img_);
  const std::vector<View>& lvl_in = trunk.in;     // the Detect layer's inputs, finest level first
  const std::vector<float>& strides = trunk.strides;
  det_pfx_ = trunk.det_pfx;
  const int nl = (int)lvl_in.size();
  GTX_CHECK(nl <= kMaxLevels, "internal: %d Detect levels", nl);
  // v10Detect holds Detect's layers twice: cv2 / cv3 (one-to-many, followed by NMS) and one2one_cv2 / one2one_cv3 (followed by the
  // top-300 cut, v10_select.hip). gtx_det_config.end2end picks the pair; the other pair's tensors are not read.
  const bool has_o2o = has(det_pfx_ + ".one2one_cv2.0.0.conv.weight");
  end2end_ = cfg_.end2end != 0;
  GTX_CHECK(!end2end_ || has_o2o, "end2end: the checkpoint has no one-to-one head (%s.one2one_cv2 / one2one_cv3): only a YOLOv10 or YOLO26 file has", det_pfx_.c_str());
  GTX_CHECK(!end2end_ || !cfg_.obj_feats, "end2end: obj_feats (ReID `model: auto`) is not implemented for the one-to-one head");
  const std::string box_br = end2end_ ? ".one2one_cv2." : ".cv2.", cls_br = end2end_ ? ".one2one_cv3." : ".cv3.";
  GTX_CHECK(has(det_pfx_ + box_br + "0.0.conv.weight") && has(det_pfx_ + cls_br + "0.2.weight"),
            "%s: the checkpoint holds no %s / %s tensors (a fused YOLOv10 / YOLO26 export keeps the one-to-one head only: run it with end2end)", det_pfx_.c_str(),
            box_br.substr(1, box_br.size() - 2).c_str(), cls_br.substr(1, cls_br.size() - 2).c_str());

  // ---- Detect (model.22, or model.28 of the P2 graph) ----
  // Stage 1 fuses the sibling convs cv2[l][0] and cv3[l][0] (same input) into one conv by
  // stacking their output channels; stage 2 runs cv2[l][1] and cv3[l][1] on channel slices.
  // The levels (three, four with P2) go out as one grouped launch per stage. The final 1x1 convs are folded
  // into the decode kernels (the box one only runs for anchors that pass the score gate).
  std::vector<Op> st1, st2;
  const bool dw_cls = trunk.dw_cls;
  std::vector<Op> dw_a, pw_a, dw_b;                // yolo11.yaml: per level, the class branch's DWConv / 1x1 Conv / DWConv in front of its last 1x1
  head_ = HeadParams{};
  head_.n_levels = nl;
  head_.nc = cfg_.nc;
  head_.conf = cfg_.conf;
  head_.class_mask[0] = head_.class_mask[1] = cfg_.n_classes == 0 ? ~0ull : 0ull;
  for (int i = 0; i < cfg_.n_classes; ++i)
    if (cfg_.classes[i] >= 0 && cfg_.classes[i] < 128) head_.class_mask[cfg_.classes[i] >> 6] |= 1ull << (cfg_.classes[i] & 63);
  int anchor = 0;
  for (int l = 0; l < nl; ++l) {
    const std::string b2 = det_pfx_ + box_br + std::to_string(l), b3 = det_pfx_ + cls_br + std::to_string(l);
    const HostTensor &w20 = tensor(b2 + ".0.conv.weight"), &w30 = tensor(b3 + (dw_cls ? ".1.1.conv.weight" : ".0.conv.weight"));
    const int cb = (int)w20.shape[0], cc = (int)w30.shape[0], cin = (int)w20.shape[1];
    GTX_CHECK(cin == lvl_in[l].c && (dw_cls || (int)w30.shape[1] == cin), "Detect level %d input channels", l);
    Op o1, o2, o3;
    View h2;
    if (dw_cls) {
      // yolo11.yaml's Detect: the box branch as above on its own (cv2[l][0] is a launch of one 64-cout tile, the sparse box branch's
      // image); the class branch is DWConv 3x3 + Conv 1x1 twice. Six ops per level, regrouped by stage below.
      const size_t mark = ops_.size();
      bool k32 = true;
      for (int q = 0; q < nl; ++q) k32 = k32 && lvl_in[q].c % 32 == 0;
      h2 = new_view(lvl_in[l].h, lvl_in[l].w, cb + cc);
      View h2b = h2.slice(0, cb), h2c = h2.slice(cb, cc);
      force_kc_ = fmt_ == DT_F16 ? (k32 ? 32 : 16) : 0;
      force_bn_ = cb % 64 == 0 ? 64 : 32;
      const View h1b = head_conv(b2 + ".0.conv", lvl_in[l], nullptr);
      force_kc_ = fmt_ == DT_F16 ? (cb % 32 == 0 ? 32 : 16) : 0;
      plain_out_ = true;
      head_conv(b2 + ".1.conv", h1b, &h2b);
      plain_out_ = false;
      const View d0 = trunk_.dwconv(b3 + ".0.0.conv", lvl_in[l], 1);
      force_kc_ = fmt_ == DT_F16 ? (k32 ? 32 : 16) : 0;
      force_bn_ = cc % 64 == 0 ? 64 : 32;
      const View p0 = head_conv(b3 + ".0.1.conv", d0, nullptr);
      const View d1v = trunk_.dwconv(b3 + ".1.0.conv", p0, 1);
      force_kc_ = fmt_ == DT_F16 ? (cc % 32 == 0 ? 32 : 16) : 0;
      plain_out_ = true;
      head_conv(b3 + ".1.1.conv", d1v, &h2c);
      plain_out_ = false;
      h2.plain = fmt_ == DT_F32S;
      force_kc_ = force_bn_ = 0;
      GTX_CHECK(ops_.size() == mark + 6, "internal: head op count");
      o1 = ops_[mark]; o2 = ops_[mark + 1]; o3 = ops_[mark + 5];
      dw_a.push_back(ops_[mark + 2]); pw_a.push_back(ops_[mark + 3]); dw_b.push_back(ops_[mark + 4]);
      ops_.resize(mark);
    } else {
    // stacked stage-1 weights / bias
    HostTensor ws;
    ws.shape = {cb + cc, cin, 3, 3};
    ws.data = w20.data;
    ws.data.insert(ws.data.end(), w30.data.begin(), w30.data.end());
    tensors_["__head" + std::to_string(l) + ".s1.weight"] = ws;
    HostTensor bs;
    bs.shape = {cb + cc};
    bs.data = tensor(b2 + ".0.conv.bias").data;
    const auto& b30 = tensor(b3 + ".0.conv.bias").data;
    bs.data.insert(bs.data.end(), b30.begin(), b30.end());
    tensors_["__head" + std::to_string(l) + ".s1.bias"] = bs;
    const size_t mark = ops_.size();
    // The levels run as grouped launches: one K chunk and one cout tile for all members of a stage. Widths that
    // are multiples of 16 only (yolov8 n / m / x) take the 16-channel chunk; a stage with a member whose Cout is not a
    // multiple of 64 takes the 32-cout tile.
    bool k32 = true;
    for (int q = 0; q < nl; ++q) k32 = k32 && lvl_in[q].c % 32 == 0;
    force_kc_ = fmt_ == DT_F16 ? (k32 ? 32 : 16) : 0;
    force_bn_ = (cb + cc) % 64 == 0 ? 64 : 32;
    View h1 = head_conv("__head" + std::to_string(l) + ".s1", lvl_in[l], nullptr);
    View h2v = new_view(h1.h, h1.w, cb + cc);
    View h1b = h1.slice(0, cb), h1c = h1.slice(cb, cc), h2b = h2v.slice(0, cb), h2c = h2v.slice(cb, cc);
    force_kc_ = fmt_ == DT_F16 ? ((cb % 32 == 0 && cc % 32 == 0) ? 32 : 16) : 0;
    force_bn_ = (cb % 64 == 0 && cc % 64 == 0) ? 64 : 32;
    plain_out_ = true;            // the decode kernels read these two as plain fp32
    head_conv(b2 + ".1.conv", h1b, &h2b);
    head_conv(b3 + ".1.conv", h1c, &h2c);
    plain_out_ = false;
    h2v.plain = fmt_ == DT_F32S;
    force_kc_ = force_bn_ = 0;
    // move the three freshly built single-problem ops into the grouped stage ops: one grouped launch per stage and kernel
    // configuration (the levels of a stage share a launch when they share the kernel)
    GTX_CHECK(ops_.size() == mark + 3, "internal: head op count");
    o1 = ops_[mark]; o2 = ops_[mark + 1]; o3 = ops_[mark + 2];
    ops_.resize(mark);
    h2 = h2v;
    }
    // Sparse box branch (head_sparse.hip): the box half of stage 1 (cout tile 0 of the stacked image) and cv2[l][1] are evaluated
    // at the candidate anchors only, after the score gate; stage 1 keeps its class half (cout tiles 1..), same packed image,
    // same scale. Needs the 16x16x32 kernel's image (32-channel chunks, one 64-cout box tile); decided for all levels at once.
    if (l == 0) {
      sparse_on_ = fmt_ == DT_F32S && env_flag("GTX_SPARSE_BOX", true);
      sparse_ = SparseBox{};
      dense_box_ops_.clear();
    }
    sparse_on_ = sparse_on_ && cb == 64 && o1.cfg.variant == ConvForm::K32 && o1.cfg.bn == 64 && o2.cfg.variant == ConvForm::K32 && cin % 32 == 0;
    head_ops_[l][0] = o1; head_ops_[l][1] = o2; head_ops_[l][2] = o3;

    HeadLevel& L = head_.lv[l];
    L.feat = h2.ptr; L.h = h2.h; L.w = h2.w; L.cstride = h2.cstride; L.cb = cb; L.cc = cc;
    L.stride = strides[l];
    L.anchor_begin = anchor;
    anchor += h2.h * h2.w;
    auto upload = [&](const std::vector<float>& v) {
      float* d = (float*)alloc(v.size() * sizeof(float));
      GTX_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
      return d;
    };
    const HostTensor &wb = tensor(b2 + ".2.weight"), &wc = tensor(b3 + ".2.weight");
    // reg_max off the last box convolution's rows: 4 x 16 DFL bins, or yolo26.yaml's four distances (reg_max = 1)
    const int box_out = (int)wb.shape[0];
    GTX_CHECK((box_out == 64 || box_out == 4) && (int)wb.shape[1] == cb, "Detect box head must have 4*16 outputs, or 4 (reg_max = 1); it has %d", box_out);
    GTX_CHECK(l == 0 || head_.reg_max == box_out / 4, "Detect box branch: reg_max differs between levels");
    head_.reg_max = box_out / 4;
    GTX_CHECK(cb <= 128 && cc % 8 == 0, "Detect head widths cb=%d cc=%d are outside what the decode kernels support", cb, cc);
    GTX_CHECK(l == 0 || cb == head_.lv[0].cb, "Detect box branch width differs between levels");
    GTX_CHECK((int)wc.shape[0] == cfg_.nc && (int)wc.shape[1] == cc, "Detect cls head has %d outputs, nc=%d", (int)wc.shape[0], cfg_.nc);
    {
      std::vector<float> wbt((size_t)cb * box_out);  // [cb][64]: the decode wave reads one output per lane; reg_max = 1: [cb][4]
      for (int o = 0; o < box_out; ++o)
        for (int k = 0; k < cb; ++k) wbt[(size_t)k * box_out + o] = wb.data[(size_t)o * cb + k];
      L.wb = upload(wbt);
    }
    L.bb = upload(tensor(b2 + ".2.bias").data);
    L.wc = upload(wc.data); L.bc = upload(tensor(b3 + ".2.bias").data);
    layer_views_[det_pfx_ + ".feat" + std::to_string(l)] = h2;
  }
  head_.n_anchors = anchor;
  GTX_CHECK(end2end_ || anchor <= nms_max_anchors(), "%d anchors per image: the NMS kernels order at most %d (ties between candidates go to the lower anchor)", anchor,
            nms_max_anchors());
  {
    auto same = [](const ConvConfig& a, const ConvConfig& b) {
      return a.dtype == b.dtype && a.ks == b.ks && a.stride == b.stride && a.bn == b.bn && a.kc == b.kc &&
             a.variant == b.variant && a.th == b.th && a.tw == b.tw;
    };
    auto add = [&](std::vector<Op>& stage, const char* name, const Op& o) {
      for (Op& g : stage)
        if (same(g.cfg, o.cfg) && g.grp.count < kMaxGroup) { g.grp.p[g.grp.count++] = o.grp.p[0]; return; }
      Op g;
      g.kind = Op::CONV;
      g.name = stage.empty() ? std::string(name) : std::string(name) + "." + std::to_string(stage.size());
      g.cfg = o.cfg;
      g.grp.p[g.grp.count++] = o.grp.p[0];
      stage.push_back(g);
    };
    std::vector<Op> d1, d2;                          // the dense box layers, kept for the debug read-backs and the overflow case
    for (int l = 0; l < nl; ++l) {
      Op o1 = head_ops_[l][0];
      const Op &o2 = head_ops_[l][1], &o3 = head_ops_[l][2];
      if (sparse_on_) {
        const ConvProblem full = o1.grp.p[0];
        const int cb = head_.lv[l].cb, cc = head_.lv[l].cc;
        const size_t tile_bytes = (size_t)(full.Cin / o1.cfg.kc) * 9 * 64 * 128;   // one 64-cout tile of the packed image
        SparseBoxLevel& S = sparse_.lv[l];
        S.in = full.in; S.H = full.H; S.W = full.W; S.cstride = full.in_cstride; S.coff = full.in_coff; S.cin = full.Cin;
        S.w1 = full.wpack; S.b1 = full.bias; S.sc1 = full.acc_scale;
        S.w2 = o2.grp.p[0].wpack; S.b2 = o2.grp.p[0].bias; S.sc2 = o2.grp.p[0].acc_scale;
        S.anchor_begin = head_.lv[l].anchor_begin;
        S.wb = head_.lv[l].wb; S.bb = head_.lv[l].bb; S.stride = head_.lv[l].stride;
        GTX_CHECK(full.bias && o2.grp.p[0].bias && o2.grp.p[0].Cin == 64 && o2.grp.p[0].Cout == 64, "sparse box branch: unexpected Detect box layers");
        Op box1 = o1;                                // the box tile alone
        box1.grp.p[0].Cout = cb;
        add(d1, (det_pfx_ + ".box1").c_str(), box1);
        add(d2, (det_pfx_ + ".box2").c_str(), o2);
        if (dw_cls) {                                // stage 1 holds no class tile: the class branch's own 1x1 layers
          add(st1, (det_pfx_ + ".stage1").c_str(), pw_a[l]);
          add(st2, (det_pfx_ + ".stage2").c_str(), o3);
          continue;
        }
        ConvProblem& p = o1.grp.p[0];                // the class tiles alone
        p.wpack = static_cast<const char*>(full.wpack) + tile_bytes;
        p.bias = full.bias + 64;
        p.Cout = cc;
        p.out_coff = full.out_coff + cb;
        add(st1, (det_pfx_ + ".stage1").c_str(), o1);
        add(st2, (det_pfx_ + ".stage2").c_str(), o3);
      } else {
        if (dw_cls) add(st1, (det_pfx_ + ".stage1").c_str(), pw_a[l]);
        add(st1, (det_pfx_ + ".stage1").c_str(), o1);
        add(st2, (det_pfx_ + ".stage2").c_str(), o2);
        add(st2, (det_pfx_ + ".stage2").c_str(), o3);
      }
    }
    if (sparse_on_) {
      sparse_.n_levels = nl;
      sparse_.reg_max = head_.reg_max;
      for (std::vector<Op>* stage : {&d1, &d2})
        for (Op& g : *stage) { g.family = conv_kernel_name(g.cfg); dense_box_ops_.push_back(g); }
    }
  }
  feat_levels_ = FeatLevels{};
  if (cfg_.obj_feats) {                           // `with_reid: true, model: auto`: the Detect layer's inputs, read after NMS
    feat_levels_.n_levels = nl;
    feat_levels_.dim = lvl_in[0].c;
    for (int l = 1; l < nl; ++l) feat_levels_.dim = std::min(feat_levels_.dim, lvl_in[l].c);
    for (int l = 0; l < nl; ++l) {
      feat_levels_.feat[l] = lvl_in[l].ptr; feat_levels_.h[l] = lvl_in[l].h; feat_levels_.w[l] = lvl_in[l].w;
      feat_levels_.cstride[l] = lvl_in[l].cstride; feat_levels_.coff[l] = lvl_in[l].coff; feat_levels_.c[l] = lvl_in[l].c;
      feat_levels_.anchor_begin[l] = head_.lv[l].anchor_begin;
      GTX_CHECK(lvl_in[l].c % feat_levels_.dim == 0, "obj_feats: Detect input %d has %d channels, not a multiple of %d", l, lvl_in[l].c, feat_levels_.dim);
    }
  }
  for (std::vector<Op>* stage : {&st1, &st2}) {
    for (const Op& d : stage == &st1 ? dw_a : dw_b) ops_.push_back(d);   // the depthwise layers a stage's 1x1 launches read
    for (Op& g : *stage) {
      g.family = conv_kernel_name(g.cfg);
      ops_.push_back(g);
    }
  }
}

void Detector::set_batch(int nb) {
  if (nb == cur_nb_) return;
  set_batch_ops(ops_, nb, es_, pad_skip_on_);
  cur_nb_ = nb;
}

// Rows of every activation tensor that can depend on the frame. The letterbox puts the resized frame in rows [top, top + new_h)
// of the network input and a constant colour everywhere else (ultralytics LetterBox, default.yaml `rect: false`: 420 + 420 of
// 1920 rows for a 16:9 frame); a convolution's output row outside the reach of those rows sees the same inputs for every
// frame, so its value is a constant of the checkpoint. Those rows are computed once (prime_pad_skip, at finalize) and the
// launches of every later pass cover the other tile rows only -- the buffers keep the constants, the results are the full
// launches' bit for bit. The interval grows with every 3x3 layer and covers the whole map from the SPPF on; the gain is in the
// backbone's large maps. GTX_PAD_SKIP=0: off.
void Detector::plan_pad_skip() {
  pad_skip_rows_ = pad_skip_total_ = 0;
  struct Rows { int lo, hi; };
  std::map<const void*, Rows> dep;                   // buffer -> frame-dependent rows; a buffer that is not here depends on the frame everywhere
  std::set<const void*> full;                        // ... and these stay that way whatever is written to them later
  // A region two different launches write (a scratch buffer reused by two layers) cannot keep either's constants: whoever
  // writes it computes every row. Writers per buffer as channel ranges.
  struct Writer { int c0, c1; Op* op; int member; };
  std::map<const void*, std::vector<Writer>> writers;
  auto second_writer = [&](const void* p, int c0, int c1, Op* op, int member) {
    bool hit = false;
    for (Writer& w : writers[p])
      if (c0 < w.c1 && w.c0 < c1) {
        hit = true;
        if (w.op->ty_count[w.member] > 0) {            // the earlier writer had been given a row range: take it back
          const ConvProblem& q = w.op->grp.p[w.member];
          pad_skip_rows_ -= (q.Ho + w.op->cfg.th - 1) / w.op->cfg.th - w.op->ty_count[w.member];
          w.op->ty_first[w.member] = w.op->ty_count[w.member] = 0;
        }
      }
    writers[p].push_back(Writer{c0, c1, op, member});
    return hit;
  };
  dep[img_.ptr] = Rows{lb_.top, lb_.top + lb_.new_h};
  auto through = [](Rows r, int k, int s, int h_out) {   // rows of a k x k / stride s / pad k/2 layer's output that see input rows [lo, hi)
    const int p = k / 2;
    const int num = r.lo + p - k + 1;                      // y >= num / s
    const int lo = num <= 0 ? 0 : (num + s - 1) / s;
    const int hi = (r.hi - 1 + p) / s + 1;
    return Rows{lo, std::min(h_out, hi)};
  };
  auto unite = [](Rows a, Rows b) { return Rows{std::min(a.lo, b.lo), std::max(a.hi, b.hi)}; };
  auto get = [&](const void* p, Rows& r) {
    auto it = dep.find(p);
    if (it == dep.end()) return false;
    r = it->second;
    return true;
  };
  auto put = [&](const void* p, bool known, Rows r) {
    if (!known) { dep.erase(p); full.insert(p); return; }
    if (full.count(p)) return;
    auto it = dep.find(p);
    if (it == dep.end()) dep[p] = r; else it->second = unite(it->second, r);   // another slice of a concat buffer may reach further
  };
  for (Op& op : ops_) {
    if (op.kind == Op::STEM) {
      Rows in{0, 0};
      const bool known = get(op.in.ptr, in);
      put(op.out.ptr, known, through(in, 3, 2, op.out.h));
      continue;
    }
    if (op.kind != Op::CONV) { put(op.out.ptr, false, Rows{0, 0}); continue; }   // pools / upsampling: deep in the network
    for (int i = 0; i < op.grp.count; ++i) {
      const ConvProblem& p = op.grp.p[i];
      op.ty_first[i] = op.ty_count[i] = 0;
      Rows in{0, p.H};
      bool known;
      if (p.front_img) {
        Rows img{0, 0};
        known = get(p.front_img, img);
        if (known) in = through(img, 3, 2, p.H);
      } else {
        known = get(p.in, in) && p.c_split == 0;       // a second, upsampled source: neck layers, all rows
      }
      Rows out = through(in, op.cfg.ks, op.cfg.stride, p.Ho);
      if (known && p.res) {
        Rows r{0, 0};
        known = get(p.res, r);
        if (known) out = unite(out, r);
      }
      const int tiles = (p.Ho + op.cfg.th - 1) / op.cfg.th;
      pad_skip_total_ += tiles;
      if (second_writer(p.out, p.out_coff, p.out_coff + p.Cout, &op, i)) known = false;
      put(p.out, known, out);
      if (!known) continue;
      const int t0 = out.lo / op.cfg.th, t1 = std::min(tiles, (out.hi + op.cfg.th - 1) / op.cfg.th);
      if (t1 - t0 < tiles && t1 > t0) {
        op.ty_first[i] = t0;
        op.ty_count[i] = t1 - t0;
        pad_skip_rows_ += tiles - (t1 - t0);
      }
    }
  }
}

// One full pass over every batch slot on a blank frame: the rows the later launches skip now hold their constants.
void Detector::prime_pad_skip() {
  if (pad_skip_rows_ == 0) return;
  const int N = cfg_.max_batch;
  hipStream_t s = ctx_->stream;
  DevBuf blank;
  blank.alloc((size_t)N * cfg_.frame_h * cfg_.frame_w * 3);
  GTX_HIP(hipMemsetAsync(blank.p, 0, blank.bytes, s));
  pad_skip_on_ = false;
  cur_nb_ = 0;
  set_batch(N);
  launch_preprocess(dtype_, (const uint8_t*)blank.p, N, lb_, img_.ptr, nullptr, cfg_.frame_h / 2, cfg_.frame_w / 2, s);
  for (const Op& op : ops_) run_op(op, N, s);
  int sat = 0;
  if (sat_dev_) GTX_HIP(hipMemcpyAsync(&sat, sat_dev_, sizeof(int), hipMemcpyDeviceToHost, s));
  GTX_HIP(hipStreamSynchronize(s));
  cur_nb_ = 0;
  if (sat_dev_) GTX_HIP(hipMemsetAsync(sat_dev_, 0, sizeof(int), s));
  if (sat) {
    // A constant of the padding rows lies beyond fp16's range: it was clamped on its way into the pair format. With the rows
    // left out of the later launches no pass would raise the flag for them again, so the skipping stays off for this detector:
    // every pass computes (and checks) every row, and the first one falls back to the exact-fp32 kernels (collect()).
    pad_skip_on_ = false;
    pad_skip_rows_ = 0;
    for (Op& op : ops_)
      for (int i = 0; i < kMaxGroup; ++i) op.ty_first[i] = op.ty_count[i] = 0;
    return;
  }
  pad_skip_on_ = true;
}

void Detector::finalize() {
  GTX_CHECK(!finalized_, "finalize called twice");
  GTX_HIP(hipSetDevice(ctx_->device));
  build_graph();
  trunk_.fuse();
  const int N = cfg_.max_batch;
  alloc_outputs();
  // NMS workspace. Candidate capacity = every anchor; sort/NMS capacity = ultralytics max_nms.
  nms_ = NmsBuffers{};
  nms_.cap = head_.n_anchors;
  nms_.nms_cap = 30016;  // >= max_nms (30000), multiple of 64
  nms_.max_det = cfg_.max_det;
  nms_.count = (int*)alloc(sizeof(int) * N);
  nms_.cand_score = (float*)alloc(sizeof(float) * N * nms_.cap);
  nms_.cand_anchor = (int*)alloc(sizeof(int) * N * nms_.cap);
  nms_.cand_cls = (int*)alloc(sizeof(int) * N * nms_.cap);
  nms_.cand_box = (float*)alloc(sizeof(float) * 4 * N * nms_.cap);
  if (!end2end_) {                                   // the sort / mask workspace of the NMS kernels (113 MB per batch slot): the one-to-one head runs none of them
    nms_.sorted_n = (int*)alloc(sizeof(int) * N);
    nms_.s_box = (float*)alloc(sizeof(float) * 4 * N * nms_.nms_cap);
    nms_.s_score = (float*)alloc(sizeof(float) * N * nms_.nms_cap);
    nms_.s_cls = (int*)alloc(sizeof(int) * N * nms_.nms_cap);
    nms_.mask = (unsigned long long*)alloc(sizeof(unsigned long long) * N * (size_t)nms_.nms_cap * (nms_.nms_cap / 64));
  }
  nms_.out_n = (int*)alloc(sizeof(int) * N);
  nms_.out_rows = (float*)alloc(sizeof(float) * 6 * N * cfg_.max_det);
  nms_.s_anchor = nms_.out_anchor = nullptr;
  if (cfg_.obj_feats) {
    nms_.s_anchor = (int*)alloc(sizeof(int) * N * nms_.nms_cap);
    nms_.out_anchor = (int*)alloc(sizeof(int) * N * cfg_.max_det);
    d_feats_ = (float*)alloc(sizeof(float) * N * cfg_.max_det * feat_levels_.dim);
    GTX_HIP(hipHostMalloc((void**)&h_feats_, sizeof(float) * N * cfg_.max_det * feat_levels_.dim));
  }
  if (sparse_on_ && !end2end_) {
    sparse_.cap = kSparseCap;
    sparse_.sat_flag = sat_dev_;
    nms_.lvl_cap = kSparseCap;
    nms_.lvl_count = (int*)alloc(sizeof(int) * N * kMaxLevels);
    nms_.lvl_list = (int*)alloc(sizeof(int) * N * kMaxLevels * kSparseCap);
  }
  if (end2end_) {
    // the one-to-one head: nms_ holds the gate's candidates (one per anchor at most); sel_ the entries v10_select keeps, with the
    // result buffers; the box branch runs on sel_'s entries only
    sel_ = nms_;
    sel_.cap = kSelCap;
    sel_.count = (int*)alloc(sizeof(int) * N);
    sel_.cand_score = (float*)alloc(sizeof(float) * N * kSelCap);
    sel_.cand_anchor = (int*)alloc(sizeof(int) * N * kSelCap);
    sel_.cand_cls = (int*)alloc(sizeof(int) * N * kSelCap);
    sel_.cand_box = (float*)alloc(sizeof(float) * 4 * N * kSelCap);
    sel_.lvl_count = sel_.lvl_list = nullptr;
    sel_.lvl_cap = 0;
    if (sparse_on_) {
      sparse_.cap = kSelCap;
      sparse_.sat_flag = sat_dev_;
      sel_.lvl_cap = kSelCap;
      sel_.lvl_count = (int*)alloc(sizeof(int) * N * kMaxLevels);
      sel_.lvl_list = (int*)alloc(sizeof(int) * N * kMaxLevels * kSelCap);
    }
    v10_scores_ = (float*)alloc(sizeof(float) * N * kV10Keep * cfg_.nc);
  }
  GTX_HIP(hipHostMalloc((void**)&h_count_, sizeof(int) * N));
  drop_tensors_unless_fallback();
  if (env_flag("GTX_PAD_SKIP", true)) {
    plan_pad_skip();
    prime_pad_skip();
  }
  set_batch(1);
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  finalized_ = true;
}

void Detector::run_op(const Op& op, int nb, hipStream_t s) { trunk_.run_op(op, nb, s); }

void Detector::run_post(int nb, hipStream_t s) {
  if (end2end_) {                                  // no NMS: gate -> the two-stage top-300 cut -> the box branch at the entries kept -> rows
    HeadParams gate = head_;
    gate.class_mask[0] = gate.class_mask[1] = ~0ull;   // `classes` is applied to the rows the cut keeps, not in front of it
    launch_head_gate(dtype_, gate, nb, nms_, s);
    launch_v10_select(dtype_, head_, nb, nms_, sel_, v10_scores_, s);
    if (sparse_on_) {
      launch_head_sparse_box(sparse_, nb, sel_, s);
      dense_head_valid_ = false;
    } else {
      launch_head_boxes(dtype_, head_, nb, sel_, s);
    }
    launch_v10_rows(sel_, head_.class_mask, nb, lb_, s);
    GTX_HIP(hipMemcpyAsync(h_count_, nms_.count, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
    GTX_HIP(hipMemcpyAsync(h_out_n_, sel_.out_n, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
    GTX_HIP(hipMemcpyAsync(h_out_rows_, sel_.out_rows, sizeof(float) * 6 * nb * cfg_.max_det, hipMemcpyDeviceToHost, s));
    if (sat_dev_) GTX_HIP(hipMemcpyAsync(h_sat_, sat_dev_, sizeof(int), hipMemcpyDeviceToHost, s));
    return;
  }
  if (sparse_on_) {                                // score gate -> the box branch at the candidates -> their boxes
    launch_head_gate(dtype_, head_, nb, nms_, s);
    launch_head_sparse_box(sparse_, nb, nms_, s);    // the box branch at the candidates and their boxes
    dense_head_valid_ = false;
  } else {
    launch_head_candidates(dtype_, head_, nb, nms_, s);
  }
  // the candidate counts come back with the results: collect() runs what this pass leaves out for a batch that needs it (the
  // general NMS kernels for > 4096 candidates in an image, the dense box layers for > kSparseCap)
  GTX_HIP(hipMemcpyAsync(h_count_, nms_.count, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
  launch_nms(nms_, nb, cfg_.iou, cfg_.agnostic_nms != 0, 30000, lb_, s, 1);
  GTX_HIP(hipMemcpyAsync(h_out_n_, nms_.out_n, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipMemcpyAsync(h_out_rows_, nms_.out_rows, sizeof(float) * 6 * nb * cfg_.max_det, hipMemcpyDeviceToHost, s));
  if (sat_dev_) GTX_HIP(hipMemcpyAsync(h_sat_, sat_dev_, sizeof(int), hipMemcpyDeviceToHost, s));
  if (cfg_.obj_feats) {
    launch_obj_feats(fmt_, feat_levels_, nb, nms_, d_feats_, s);
    GTX_HIP(hipMemcpyAsync(h_feats_, d_feats_, sizeof(float) * nb * cfg_.max_det * feat_levels_.dim, hipMemcpyDeviceToHost, s));
  }
}

// The dense box layers of the Detect head on the activations of the pass that ran last (sparse mode leaves them out of the
// forward): for the debug read-backs and for a batch with more candidates than the sparse buffer holds.
void Detector::run_dense_box(hipStream_t s) {
  if (!sparse_on_ || dense_head_valid_) return;
  GTX_CHECK(cur_nb_ > 0, "no forward pass has run yet");
  for (Op o : dense_box_ops_) {
    for (int i = 0; i < o.grp.count; ++i) o.grp.p[i].N = cur_nb_;
    conv_group_finalize(o.grp, o.cfg);
    run_op(o, cur_nb_, s);
  }
  dense_head_valid_ = true;
}

// What the pass left out for the common case: the general NMS kernels for > 4096 candidates in an image, the dense box layers and
// every candidate's box for > kSparseCap; then the appearance vectors out of the pinned buffer before the next pass lands in it.
void Detector::after_pass(int nb) {
  // The one-to-one head leaves nothing out of its pass, so there is no overflow case to finish here: the gate's buffer (nms_.cap =
  // n_anchors) takes one candidate per anchor at most, head_candidates_kernel writes no more, and v10_select hands the box branch at
  // most kV10Keep = 300 entries of sel_'s 304 (cap and lvl_cap) -- the sparse buffer cannot fill, whatever conf is
  // (tests/test_yolov10_gpu.py::test_every_anchor_a_candidate). No NMS runs either, so there is no large-NMS re-run.
  if (end2end_) return;
  bool over = false, big = false;
  for (int b = 0; b < nb; ++b) {
    over = over || (sparse_on_ && h_count_[b] > kSparseCap);                 // more candidates than the sparse buffer holds
    big = big || !nms_small_covers(std::min(h_count_[b], nms_.cap), nms_.max_det);   // ... than the single-workgroup NMS takes
  }
  if (over || big) {
    hipStream_t s = ctx_->stream;
    NmsBuffers dense = nms_;
    if (over) {                                      // the dense box layers, then every candidate's box again
      run_dense_box(s);
      launch_head_boxes(dtype_, head_, nb, dense, s);
      ++sparse_overflows_;
    }
    launch_nms(dense, nb, cfg_.iou, cfg_.agnostic_nms != 0, 30000, lb_, s, over ? 0 : 2);
    GTX_HIP(hipMemcpyAsync(h_out_n_, nms_.out_n, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
    GTX_HIP(hipMemcpyAsync(h_out_rows_, nms_.out_rows, sizeof(float) * 6 * nb * cfg_.max_det, hipMemcpyDeviceToHost, s));
    if (cfg_.obj_feats) {
      launch_obj_feats(fmt_, feat_levels_, nb, nms_, d_feats_, s);
      GTX_HIP(hipMemcpyAsync(h_feats_, d_feats_, sizeof(float) * nb * cfg_.max_det * feat_levels_.dim, hipMemcpyDeviceToHost, s));
    }
    record_post_end(s);                              // the postprocess figure now includes the re-run
    GTX_HIP(hipStreamSynchronize(s));
  }
  if (cfg_.obj_feats) {
    c_feat_n_.assign(cfg_.max_batch, 0);
    c_feats_.resize((size_t)cfg_.max_batch * cfg_.max_det * feat_levels_.dim);
    for (int b = 0; b < nb; ++b) {
      c_feat_n_[b] = h_out_n_[b];
      const size_t o = (size_t)b * cfg_.max_det * feat_levels_.dim;
      memcpy(c_feats_.data() + o, h_feats_ + o, sizeof(float) * h_out_n_[b] * feat_levels_.dim);
    }
  }
}

void Detector::features(int b, float* out, int cap, int* n, int* dim) const {
  GTX_CHECK(cfg_.obj_feats && h_feats_, "features: the detector was created without gtx_det_config.obj_feats");
  GTX_CHECK(b >= 0 && b < cfg_.max_batch, "features: image %d of %d", b, cfg_.max_batch);
  const int cnt = std::min(b < (int)c_feat_n_.size() ? c_feat_n_[b] : 0, cap);
  if (n) *n = cnt;
  if (dim) *dim = feat_levels_.dim;
  if (out && cnt > 0) memcpy(out, c_feats_.data() + (size_t)b * cfg_.max_det * feat_levels_.dim, sizeof(float) * cnt * feat_levels_.dim);
}

void Detector::raw_output(int b, float* out, int* n_anchors, bool logits) {
  GTX_CHECK(finalized_ && cur_nb_ > 0 && b >= 0 && b < cur_nb_, "raw_output: no forward pass for slot %d", b);
  const size_t per = (size_t)head_.n_anchors * (4 + head_.nc);
  if (raw_.bytes < per * cur_nb_ * sizeof(float)) raw_.alloc(per * cur_nb_ * sizeof(float));
  GTX_CHECK(!in_flight_, "raw_output while a batch is in flight: call collect first");
  run_dense_box(ctx_->stream);                     // the full decode reads every anchor's box features
  launch_head_raw(dtype_, head_, cur_nb_, raw_.as<float>(), logits, ctx_->stream);
  GTX_HIP(hipMemcpyAsync(out, raw_.as<float>() + per * b, per * sizeof(float), hipMemcpyDeviceToHost, ctx_->stream));
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  if (n_anchors) *n_anchors = head_.n_anchors;
}

void Detector::layer_output(int b, const std::string& layer, float* out, int* h, int* w, int* c) {
  // Not while a pass is in flight: the stand-alone launches of the hidden layers would queue behind it and overwrite the
  // buffers it shares with them.
  GTX_CHECK(!(out && in_flight_), "layer_output while a batch is in flight: call collect first");
  auto it = layer_views_.find(layer);
  if (it == layer_views_.end()) fail(-1, "unknown layer '%s'", layer.c_str());
  const View& v = it->second;
  if (out && sparse_on_ && cur_nb_ > 0 && (layer.rfind(det_pfx_ + ".", 0) == 0 || layer.rfind("__head", 0) == 0)) {
    GTX_HIP(hipSetDevice(ctx_->device));
    run_dense_box(ctx_->stream);                   // the head's box layers are not part of the forward in sparse mode
    GTX_HIP(hipStreamSynchronize(ctx_->stream));
  }
  if (out) trunk_.recompute_hidden(layer, cur_nb_, ctx_->stream);   // the stem's output, model.1's: not written by the fused front
  if (h) *h = v.h;
  if (w) *w = v.w;
  if (c) *c = v.c;
  if (!out) return;
  GTX_CHECK(b >= 0 && b < cfg_.max_batch, "bad batch slot");
  GTX_CHECK(!trunk_.hidden(v.ptr), "layer_output('%s'): the layer's buffer was not re-created", layer.c_str());
  read_view(v, b, out);
}

}  // namespace gtx
