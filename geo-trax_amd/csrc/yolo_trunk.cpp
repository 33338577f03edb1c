// YoloTrunk (yolo_trunk.hpp): the backbone + neck of the YOLO detectors, built by one walk (build()) over a layer table that restates
// the family's model yaml row by row: ultralytics' cfg/models/v8/yolov8.yaml (kYolov8: Detect = model.22; YOLOv8-RTDETR puts its
// decoder there; rows 0-8 are the YOLOv8-cls backbone of the ReID embedder), v8/yolov8-p2.yaml (kYolov8P2: one more stage at stride 4,
// Detect = model.28) and 11/yolo11.yaml (kYolo11: C3k2 blocks, C2PSA = model.10, Detect = model.23). Channel widths, bottleneck counts
// and c3k-or-not are read off the tensor shapes, so every scale (n/s/m/l/x) loads unchanged. A new family is one more table and one
// more rule in choose_graph(); a new module is one more case in build(). v10/yolov10.yaml is kYolo10 (SCDown, PSA = model.10, C2fCIB, v10Detect = model.23),
// v9/yolov9{t,s,m,c}.yaml kYolo9 (ELAN1 / RepNCSPELAN4, AConv / ADown behind pool_down.hip's launch, SPPELAN = model.9, Detect = model.22). The two classification graphs of the ReID embedder are
// prefixes of these tables: yolov8-cls.yaml = kYolov8's rows 0-8, 11/yolo11-cls.yaml = kYolo11's rows 0-8 + C2PSA as model.9 (kYolo11Cls).
// 26/yolo26.yaml is kYolo26: kYolo11's rows with SPPF's linear cv1 + residual at model.9 and the C3k2 with attention at model.22.
// 12/yolo12.yaml is kYolo12: A2C2f blocks (area attention in the backbone, C3k members in the neck), no SPPF, Detect = model.21.
// v5/yolov5.yaml with the anchor-free Detect (the yolov5*u files) is kYolov5u: a 6x6 stem (stem6.hip), C3 blocks, 1x1 Convs in the neck, Detect = model.24.
#include "yolo_trunk.hpp"
#include "area_attn.hpp"
#include "pool_down.hpp"
#include "rtdetr_kernels.hpp"
#include "split_format.hpp"
#include "stem6.hpp"

#include <algorithm>

namespace gtx {

namespace {
using namespace tables;
}  // namespace

TrunkGraph YoloTrunk::cls_backbone() { return TrunkGraph{kYolov8, kClsBackboneRows, false}; }

// The classifier's yaml by its tensor names: an attention block at model.9 and no Detect at model.23 is yolo11-cls.yaml
TrunkGraph YoloTrunk::choose_cls_graph() const {
  if (net_.has("model.9.m.0.attn.qkv.conv.weight") && !net_.has("model.23.cv2.0.0.conv.weight")) return graph_of(kYolo11Cls, false);
  return cls_backbone();
}

// Which yaml the tensors were built from, told apart by their names like the reference's model yaml does
TrunkGraph YoloTrunk::choose_graph() const {
  // yolov5.yaml: a 6x6 stem and YOLOv8's Detect at model.24 -- no other yaml has either
  if (net_.has("model.0.conv.weight") && net_.tensor("model.0.conv.weight").shape.size() == 4 && net_.tensor("model.0.conv.weight").shape[2] == 6 &&
      net_.has("model.24.cv2.0.0.conv.weight"))
    return graph_of(kYolov5u, false);
  // yolo12.yaml: an A2C2f's ABlocks (a Sequential of two inside m.{k}) at model.6 and YOLO11's Detect at model.21 -- no other yaml has either
  if (net_.has("model.6.m.0.0.attn.qkv.conv.weight") && net_.has("model.21.cv3.0.0.0.conv.weight")) return graph_of(kYolo12, true);
  // yolov10.yaml: PSA's attention directly under model.10, SCDown's depthwise model.5.cv2 and a one-to-one head at model.23
  if (net_.has("model.10.attn.qkv.conv.weight") && net_.has("model.5.cv2.conv.weight") && net_.has("model.23.one2one_cv2.0.0.conv.weight"))
    return graph_of(kYolo10, true);
  // yolo26.yaml: yolo11.yaml's names plus the attention inside model.22's C3k2 and a one-to-one head at model.23
  if (net_.has("model.10.m.0.attn.qkv.conv.weight") && net_.has("model.22.m.0.1.attn.qkv.conv.weight") && net_.has("model.23.one2one_cv2.0.0.conv.weight"))
    return graph_of(kYolo26, true);
  // yolo11.yaml: C2PSA at model.10 and Detect (depthwise class branch) at model.23 -- names no YOLOv8 file has
  if (net_.has("model.10.m.0.attn.qkv.conv.weight") && net_.has("model.23.cv3.0.0.0.conv.weight")) return graph_of(kYolo11, true);
  // yolov9.yaml: a RepNCSPELAN4's RepCSP (a Sequential inside the block) and SPPELAN's cv5 at model.9, Detect = model.22
  if (net_.has("model.9.cv5.conv.weight") && net_.has("model.4.cv2.0.cv1.conv.weight") && net_.has("model.22.cv2.0.0.conv.weight")) return graph_of(kYolo9, false);
  // yolov8-p2.yaml: Detect = model.28 on four levels; else yolov8.yaml (Detect, or YOLOv8-RTDETR's decoder, = model.22)
  return net_.has("model.28.cv2.0.0.conv.weight") ? graph_of(kYolov8P2, false) : graph_of(kYolov8, false);
}

View YoloTrunk::conv(const std::string& name, const View& x, int stride, const View* out_slice, const View* residual, const View* up_src) {
  GTX_CHECK(net_.format() != DT_F32S || !up_src || !up_src->plain, "%s: a plain fp32 tensor cannot feed a split convolution", name.c_str());
  NetRuntime::ConvArgs a;
  a.stride = stride; a.act = 1; a.out_slice = out_slice; a.residual = residual;
  // The fused post / front stages (fuse_front, fuse_stem) are stages of the 32x32x16 kernel and read its 16-channel-chunk weight
  // image. The one layer they can attach to -- model.1 with all its couts in one tile, YOLOv8 n / s -- keeps that kernel while
  // either fusion is enabled; conv_pick_config leaves a pinned K chunk alone.
  if (net_.format() == DT_F32S && stride == 2 && name == "model.1.conv" && net_.tensor(name + ".weight").shape[0] <= 64 &&
      (env_flag("GTX_FUSE_FRONT", true) || env_flag("GTX_FUSE_STEM", true)))
    a.force_kc = 16;
  const View out = net_.emit_named_conv(ops_, name, x, a);
  if (up_src) read_upsampled(ops_.back(), x, *up_src);
  return out;
}

// The conv op just emitted on x reads x's leading up_src.c channels from up_src, upsampled 2x, instead (ConvProblem::in2)
void YoloTrunk::read_upsampled(Op& op, const View& x, const View& up_src) {
  GTX_CHECK(op.cfg.ks == 1 && op.cfg.stride == 1 && op.cfg.variant == ConvForm::Split && up_src.h * 2 == x.h && up_src.w * 2 == x.w && up_src.c < x.c,
            "%s: upsampled source does not fit", op.name.c_str());
  ConvProblem& p = op.grp.p[0];
  p.in2 = up_src.ptr; p.in2_cstride = up_src.cstride; p.in2_coff = up_src.coff; p.c_split = up_src.c;
  op.family = conv_kernel_name(op.cfg);
}

void YoloTrunk::upsample(const std::string& name, const View& src, const View& dst) {
  GTX_CHECK(dst.h == 2 * src.h && dst.w == 2 * src.w && dst.c == src.c, "%s: a %dx%dx%d map does not upsample into %dx%dx%d", name.c_str(), src.w, src.h, src.c, dst.w, dst.h, dst.c);
  Op op;
  op.kind = Op::UPSAMPLE;
  op.name = name;
  op.family = "upsample2x_kernel";
  op.in = src;
  op.out = dst;
  ops_.push_back(op);
}

// ---- SPPF: cv1 -> 3 cascaded pools -> cv2, written into `out` (its slice of the Concat that lists it, or a view of its own)
// linear_res (yolo26.yaml's SPPF(shortcut)): cv1 has no activation, and x joins cv2's output in its epilogue, after the activation
void YoloTrunk::sppf(const std::string& pfx, const View& x, const View& out, const char* last, bool linear_res) {
  const int cm = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0];
  View sp = net_.new_view(x.h, x.w, 4 * cm);
  View sp0 = sp.slice(0, cm);
  if (linear_res) conv_act(pfx + ".cv1.conv", x, 0, &sp0, nullptr);
  else conv(pfx + ".cv1.conv", x, 1, &sp0, nullptr);
  Op op;
  op.kind = Op::POOL;
  op.name = pfx + ".m";
  op.family = "sppf_pool_kernel";
  op.in = sp0;
  op.out = sp;
  ops_.push_back(op);
  GTX_CHECK(!linear_res || x.c == out.c, "%s: the residual has %d channels, the output %d", pfx.c_str(), x.c, out.c);
  conv(pfx + last, sp, 1, &out, linear_res ? &x : nullptr);
  net_.set_layer_view(pfx, out);
}

// One stride-1 Conv op with the given activation (0 none, 1 SiLU). The convolution kernels take channel counts that are
// multiples of 16: a narrower layer (the 8-channel hidden layer of scale n's model.2 bottleneck) gets zero output channels
// appended -- SiLU(0) = 0 -- and its consumer zero input weights for them, which changes no sum. A padded layer may write a slice and
// take a residual of its padded width (the residual's padding channels hold zeros, so the output's do); in_seg: the input is a concat
// of such padded maps, in_seg real channels in each (YOLOv9-t's 24-channel RepCSP hidden maps).
View YoloTrunk::conv_act(const std::string& name, const View& x, int act, const View* out_slice, const View* residual, int in_seg) {
  const HostTensor& w = net_.tensor(name + ".weight");
  GTX_CHECK(w.shape.size() == 4 && w.shape[2] == w.shape[3], "%s: expected OIHW square kernel", name.c_str());
  const int cout = (int)w.shape[0], cin = (int)w.shape[1], ks = (int)w.shape[2], taps = ks * ks;
  const int cout_p = (cout + 15) / 16 * 16, cin_p = x.c;
  NetRuntime::ConvArgs a;
  a.act = act; a.out_slice = out_slice; a.residual = residual;
  if (cout_p == cout && cin_p == cin) return net_.emit_named_conv(ops_, name, x, a);
  GTX_CHECK(cin_p >= cin && (cout_p == cout || ((!out_slice || out_slice->c == cout_p) && (!residual || residual->c == cout_p))),
            "%s: %d -> %d channels cannot be padded here", name.c_str(), cin, cout);
  const int seg_p = in_seg > 0 ? (in_seg + 15) / 16 * 16 : 0;
  GTX_CHECK(in_seg <= 0 || (cin % in_seg == 0 && cin_p == cin / in_seg * seg_p), "%s: %d input channels are not padded segments of %d", name.c_str(), cin_p, in_seg);
  std::vector<float> wp((size_t)cout_p * cin_p * taps, 0.f), bp(cout_p, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int i = 0; i < cin; ++i) {
      const int ip = in_seg > 0 ? i / in_seg * seg_p + i % in_seg : i;
      for (int t = 0; t < taps; ++t) wp[((size_t)o * cin_p + ip) * taps + t] = w.data[((size_t)o * cin + i) * taps + t];
    }
  if (const float* b = net_.bias_of(name, cout)) std::copy(b, b + cout, bp.begin());
  return net_.emit_conv(ops_, name, wp.data(), cout_p, cin_p, ks, bp.data(), x, a);
}

// Bottleneck(c, c, shortcut, k = (3, 3), e): src -> dst (+ src); the hidden width is read off cv1 (c in C2f and C3k, c / 2 in C3k2)
View YoloTrunk::bottleneck(const std::string& m, const View& src, const View& dst, bool shortcut) {
  // a buffer of its own per bottleneck: rows that no launch rewrites (plan_pad_skip) must keep ONE producer's values
  const View tmp = conv_act(m + ".cv1.conv", src, 1, nullptr, nullptr);
  return conv_act(m + ".cv2.conv", tmp, 1, &dst, shortcut ? &src : nullptr);
}

// C3k: cv3(cat(m(cv1(x)), cv2(x))), m = Bottlenecks of full hidden width. YOLOv9's RepCSP is the same block (its RepConv arrives fused:
// one 3x3). A hidden width that is no multiple of 16 (RepCSP's 24 channels in yolov9t) is carried zero-padded: chp channels per map.
View YoloTrunk::c3k(const std::string& m, const View& src, const View& dst, bool shortcut) {
  const int ch = (int)net_.tensor(m + ".cv1.conv.weight").shape[0], chp = (ch + 15) / 16 * 16;
  int n = 0;
  while (net_.has(m + ".m." + std::to_string(n) + ".cv1.conv.weight")) ++n;
  View cat = net_.new_view(src.h, src.w, 2 * chp);
  View left = cat.slice(0, chp), right = cat.slice(chp, chp);
  View y = n == 0 ? left : net_.new_view(src.h, src.w, chp);
  conv_act(m + ".cv1.conv", src, 1, &y, nullptr);
  for (int j = 0; j < n; ++j) {
    View nxt = j + 1 == n ? left : net_.new_view(src.h, src.w, chp);
    bottleneck(m + ".m." + std::to_string(j), y, nxt, shortcut);
    y = nxt;
  }
  conv_act(m + ".cv2.conv", src, 1, &right, nullptr);
  return conv_act(m + ".cv3.conv", cat, 1, &dst, nullptr, chp != ch ? ch : 0);
}

// C3(c1, c2, n, shortcut, e = 0.5) of yolov5.yaml: cv3(cat(m(cv1 x), cv2 x)), cv1 and cv2 both 1x1 on the block's input, m = n
// Bottleneck(c_, c_, shortcut, k = (1x1, 3x3), e = 1.0). cv1 and cv2 run as ONE 1x1 launch over their weights stacked [cv2 | cv1] into
// channels [c_, 3 c_) of a 3 c_-wide buffer; the bottlenecks chain from cv1's slice and the last one writes channels [0, c_), so that
// cv3 reads its concat [m | cv2 x] in place as the buffer's first 2 c_ channels and no slice has two writers (plan_pad_skip).
View YoloTrunk::c3(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src) {
  const HostTensor &w1 = net_.tensor(pfx + ".cv1.conv.weight"), &w2 = net_.tensor(pfx + ".cv2.conv.weight");
  const int c = (int)w1.shape[0], cin = (int)w1.shape[1];
  int n = 0;
  while (net_.has(pfx + ".m." + std::to_string(n) + ".cv1.conv.weight")) ++n;
  GTX_CHECK(n > 0 && c % 16 == 0 && w1.shape.size() == 4 && w1.shape == w2.shape && w1.shape[2] == 1 && w1.shape[3] == 1 && cin == x.c,
            "%s: cv1 / cv2 must be 1x1 convolutions of one shape on %d channels, with bottlenecks behind cv1", pfx.c_str(), x.c);
  std::vector<float> ws((size_t)2 * c * cin), bs(2 * c, 0.f);
  std::copy(w2.data.begin(), w2.data.end(), ws.begin());
  std::copy(w1.data.begin(), w1.data.end(), ws.begin() + (size_t)c * cin);
  if (const float* b = net_.bias_of(pfx + ".cv2.conv", c)) std::copy(b, b + c, bs.begin());
  if (const float* b = net_.bias_of(pfx + ".cv1.conv", c)) std::copy(b, b + c, bs.begin() + c);
  View buf = net_.new_view(x.h, x.w, 3 * c);
  const View both = buf.slice(c, 2 * c), left = buf.slice(0, c);
  NetRuntime::ConvArgs a;
  a.act = 1; a.out_slice = &both;
  net_.emit_conv(ops_, pfx + ".cv2|cv1.conv", ws.data(), 2 * c, cin, 1, bs.data(), x, a);
  if (up_src) read_upsampled(ops_.back(), x, *up_src);
  net_.set_layer_view(pfx + ".cv1.conv", buf.slice(2 * c, c));
  net_.set_layer_view(pfx + ".cv2.conv", buf.slice(c, c));
  View y = buf.slice(2 * c, c);
  for (int j = 0; j < n; ++j) {
    const View nxt = j + 1 == n ? left : net_.new_view(x.h, x.w, c);
    bottleneck(pfx + ".m." + std::to_string(j), y, nxt, shortcut);
    y = nxt;
  }
  const View out = conv(pfx + ".cv3.conv", buf.slice(0, 2 * c), 1, out_slice, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

// ELAN1 / RepNCSPELAN4(c1, c2, c3, c4, n): cv1 -> two chunks of c3 / 2; cv2 on the second chunk, cv3 on cv2's output, each a
// Sequential(RepCSP, Conv3x3) (ELAN1: a plain Conv3x3); cv4 on the concatenation of the four. Chunks and concat are channel offsets
// into one buffer, as in C2f.
View YoloTrunk::elan(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src) {
  const bool rep = net_.has(pfx + ".cv2.0.cv1.conv.weight");
  const int c3 = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0], half = c3 / 2;
  const int c4 = (int)net_.tensor(pfx + (rep ? ".cv2.1.conv.weight" : ".cv2.conv.weight")).shape[0];
  GTX_CHECK(c3 % 16 == 0 && c4 % 8 == 0, "%s: chunks of %d and branches of %d channels", pfx.c_str(), half, c4);
  View cat = net_.new_view(x.h, x.w, c3 + 2 * c4);
  View first = cat.slice(0, c3);
  conv(pfx + ".cv1.conv", x, 1, &first, nullptr, up_src);
  View src = cat.slice(half, half);
  for (int k = 0; k < 2; ++k) {
    const std::string b = pfx + (k == 0 ? ".cv2" : ".cv3");
    View dst = cat.slice(c3 + k * c4, c4);
    if (rep) {
      const View mid = net_.new_view(x.h, x.w, c4);
      c3k(b + ".0", src, mid, shortcut);
      conv_act(b + ".1.conv", mid, 1, &dst, nullptr);
    } else {
      conv_act(b + ".conv", src, 1, &dst, nullptr);
    }
    src = dst;
  }
  View out = conv(pfx + ".cv4.conv", cat, 1, out_slice, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

// AConv(c1, c2): cv1(avg_pool2d(x, 2, 1)), cv1 = Conv 3x3 stride 2. ADown(c1, c2), told by its cv2: the same average, then cv1 on the
// first half of the channels and cv2 = Conv 1x1 on max_pool2d(3, 2, 1) of the second half, concatenated. One pool_down launch writes
// what the convolutions read: the average at x's size with a zero last row and column (the even-sized stride-2 kernels then form
// Conv2d(3, 2, 1)'s sums on the odd-sized map), the maximum at half of it.
View YoloTrunk::adown(const std::string& pfx, const View& x, const View* out_slice) {
  const bool two = net_.has(pfx + ".cv2.conv.weight");
  GTX_CHECK(x.h % 2 == 0 && x.w % 2 == 0 && x.c % 16 == 0, "%s: a %dx%d map of %d channels", pfx.c_str(), x.w, x.h, x.c);
  const int ca = two ? x.c / 2 : x.c;
  const View avg = net_.new_view(x.h, x.w, ca);
  View mx;
  if (two) mx = net_.new_view(x.h / 2, x.w / 2, x.c - ca);
  Op op;
  op.kind = Op::POOLDOWN;
  op.name = pfx + ".pool";
  op.family = "pool_down_kernel";
  op.in = x; op.out = avg; op.out2 = mx;
  ops_.push_back(op);
  net_.set_layer_view(pfx + ".pool", avg);
  if (!two) {
    const View out = conv(pfx + ".cv1.conv", avg, 2, out_slice, nullptr);
    net_.set_layer_view(pfx, out);
    return out;
  }
  net_.set_layer_view(pfx + ".maxpool", mx);
  const int c = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0];
  const View out = out_slice ? *out_slice : net_.new_view(x.h / 2, x.w / 2, 2 * c);
  const View a = out.slice(0, c), b = out.slice(c, c);
  conv(pfx + ".cv1.conv", avg, 2, &a, nullptr);
  conv(pfx + ".cv2.conv", mx, 1, &b, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

// C2f / C3k2: cv1 -> a | b, n blocks m.{k} chained from b with every output appended, cv2 on the concatenation. m.{k} is a Bottleneck
// (C2f: full hidden width; C3k2 with c3k = False: half of it), a C3k (C3k2 with c3k = True: the block has a cv3) or, in yolo26.yaml's
// C3k2 with attention, Sequential(Bottleneck of half width, PSABlock): m.{k}.0.cv1 / cv2, then C2PSA's block on m.{k}.1.*.
View YoloTrunk::c2f(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src) {
  const int c = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0] / 2;
  int n = 0;
  while (net_.has(pfx + ".m." + std::to_string(n) + ".cv1.conv.weight") || net_.has(pfx + ".m." + std::to_string(n) + ".cv1.0.conv.weight") ||
         net_.has(pfx + ".m." + std::to_string(n) + ".0.cv1.conv.weight"))
    ++n;
  View cat = net_.new_view(x.h, x.w, (2 + n) * c);
  View first = cat.slice(0, 2 * c);
  conv(pfx + ".cv1.conv", x, 1, &first, nullptr, up_src);
  for (int k = 0; k < n; ++k) {
    const std::string m = pfx + ".m." + std::to_string(k);
    View src = cat.slice((1 + k) * c, c), dst = cat.slice((2 + k) * c, c);
    if (net_.has(m + ".0.cv1.conv.weight") && net_.has(m + ".1.attn.qkv.conv.weight")) {        // C3k2 with attention (yolo26.yaml): Bottleneck, then PSABlock
      GTX_CHECK(c % 64 == 0, "%s: %d hidden channels are not whole 64-wide attention heads", m.c_str(), c);
      const View mid = net_.new_view(x.h, x.w, c);
      bottleneck(m + ".0", src, mid, shortcut);
      psa_block(m + ".1", mid, dst);
    } else if (net_.has(m + ".cv1.0.conv.weight")) cib(m, src, dst, shortcut);                // C2fCIB (yolov10.yaml)
    else if (net_.has(m + ".cv3.conv.weight")) c3k(m, src, dst, shortcut);
    else bottleneck(m, src, dst, shortcut);
  }
  View out = conv(pfx + ".cv2.conv", cat, 1, out_slice, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

// PSABlock on b (c channels, c / 64 heads of key depth 32 and value width 64) -> dst: b1 = b + proj(attention(qkv(b)) + pe(v)), dst = b1 +
// ffn.1(ffn.0(b1)). The convolutions without activation take the residual in their epilogue. dst may be b's own buffer.
void YoloTrunk::psa_block(const std::string& m, const View& b, const View& dst) {
  const int c = b.c, heads = c / 64;
  const HostTensor &wq = net_.tensor(m + ".attn.qkv.conv.weight"), &wp = net_.tensor(m + ".attn.pe.conv.weight");
  GTX_CHECK(c % 64 == 0 && (int)wq.shape[0] == heads * 128 && wp.shape.size() == 4 && (int)wp.shape[0] == c && wp.shape[1] == 1 && wp.shape[2] == 3,
            "%s: attention of %d heads with key_dim 32 / head_dim 64 expected", m.c_str(), heads);
  const View qkv = conv_act(m + ".attn.qkv.conv", b, 0, nullptr, nullptr);
  View att = net_.new_view(b.h, b.w, c);
  {
    std::vector<float> bias(c, 0.f);
    if (const float* pb = net_.bias_of(m + ".attn.pe.conv", c)) std::copy(pb, pb + c, bias.begin());
    Op op;
    op.kind = Op::ATTN;
    op.name = m + ".attn";
    op.family = psa_attention_kernel_name(b.h, b.w);
    op.in = qkv; op.out = att;
    op.heads = heads;
    op.dw_w = net_.upload(dw_tap_major(wp.data.data(), c, 9)); op.dw_bias = net_.upload(bias);
    op.sat = net_.sat_flag();
    ops_.push_back(op);
    net_.set_layer_view(m + ".attn.out", att);       // softmax(q^T k) v + pe(v): what proj reads
  }
  View b1 = net_.new_view(b.h, b.w, c);
  conv_act(m + ".attn.proj.conv", att, 0, &b1, &b);
  const View f0 = conv_act(m + ".ffn.0.conv", b1, 1, nullptr, nullptr);
  conv_act(m + ".ffn.1.conv", f0, 0, &dst, &b1);
}

// C2PSA: cv1 -> a | b; per PSABlock b += proj(attention(qkv(b)) + pe(v)), b += ffn.1(ffn.0(b)); cv2 on cat(a, b). The convolutions
// without activation take the residual in their epilogue (activation first, then the residual: x + conv(x)). The last block
// writes b back into cv1's buffer, which cv2 then reads whole.
View YoloTrunk::c2psa(const std::string& pfx, const View& x, const View* out_slice, bool bare) {
  const int c = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0] / 2;
  GTX_CHECK(c % 64 == 0, "%s: %d hidden channels are not whole 64-wide attention heads", pfx.c_str(), c);
  int n = bare ? 1 : 0;
  while (!bare && net_.has(pfx + ".m." + std::to_string(n) + ".attn.qkv.conv.weight")) ++n;
  GTX_CHECK(n > 0, "%s: no PSABlock", pfx.c_str());
  View ab = conv(pfx + ".cv1.conv", x, 1, nullptr, nullptr);
  View b = ab.slice(c, c);
  for (int k = 0; k < n; ++k) {
    const View b2 = k + 1 == n ? ab.slice(c, c) : net_.new_view(x.h, x.w, c);
    psa_block(bare ? pfx : pfx + ".m." + std::to_string(k), b, b2);
    b = b2;
  }
  View out = conv(pfx + ".cv2.conv", ab, 1, out_slice, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

// ABlock(c, heads = c / 32, mlp_ratio, area) on x -> dst: x1 = x + proj(attention(qkv(x)) + pe(v)), dst = x1 + mlp.1(mlp.0(x1)). AAttn's qkv
// convolution writes per head [q 32 | k 32 | v 32]; its rows are emitted in the order [q of every head | k of every head | v of every
// head] instead (the same sums, other channel positions), so that v is a channel slice of the qkv map: the attention launch reads the
// planar layout, and `pe` -- a depthwise 7x7 without activation -- is the existing depthwise launch on that slice with the attention's
// output as its residual. mlp.0's width int(c * mlp_ratio) need not be a multiple of 16 (307 at scale l): conv_act pads it with zeros.
void YoloTrunk::ablock(const std::string& m, const View& x, const View& dst, int area) {
  const int c = x.c, heads = c / 32;
  const std::string q = m + ".attn.qkv.conv";
  const HostTensor &wq = net_.tensor(q + ".weight"), &wp = net_.tensor(m + ".attn.pe.conv.weight");
  GTX_CHECK(c % 32 == 0 && heads > 0 && wq.shape.size() == 4 && (int)wq.shape[0] == 3 * c && (int)wq.shape[1] == c && wq.shape[2] == 1 && wq.shape[3] == 1 &&
                wp.shape.size() == 4 && (int)wp.shape[0] == c && wp.shape[1] == 1 && wp.shape[2] == 7,
            "%s: area attention of %d heads of width 32 with a 7x7 pe expected", m.c_str(), heads);
  GTX_CHECK(area_attention_fits(x.h, x.w, area), "%s: a %d x %d map (%d positions) does not cut into %d equal areas", m.c_str(), x.w, x.h, x.h * x.w, area);
  std::vector<float> wpl((size_t)3 * c * c), bpl(3 * c, 0.f);
  const float* bq = net_.bias_of(q, 3 * c);
  for (int part = 0; part < 3; ++part)
    for (int h = 0; h < heads; ++h)
      for (int d = 0; d < 32; ++d) {
        const int src = h * 96 + part * 32 + d, dstrow = part * c + h * 32 + d;
        std::copy(wq.data.begin() + (size_t)src * c, wq.data.begin() + (size_t)(src + 1) * c, wpl.begin() + (size_t)dstrow * c);
        if (bq) bpl[dstrow] = bq[src];
      }
  NetRuntime::ConvArgs a;
  a.act = 0;
  const View qkv = net_.emit_conv(ops_, q, wpl.data(), 3 * c, c, 1, bpl.data(), x, a);
  View att = net_.new_view(x.h, x.w, c);
  {
    Op op;
    op.kind = Op::AREAATTN;
    op.name = m + ".attn";
    op.family = "area_attn_kernel";
    op.in = qkv; op.out = att;
    op.heads = heads; op.area = area;
    op.sat = net_.sat_flag();
    ops_.push_back(op);
    net_.set_layer_view(m + ".attn.out", att);       // softmax(q^T k) v, bands back in map order
  }
  const View v = qkv.slice(2 * c, c);
  const View sum = dwconv(m + ".attn.pe.conv", v, 0, 1, nullptr, &att);   // attention + pe(v): what proj reads
  View x1 = net_.new_view(x.h, x.w, c);
  conv_act(m + ".attn.proj.conv", sum, 0, &x1, &x);
  const View f0 = conv_act(m + ".mlp.0.conv", x1, 1, nullptr, nullptr);
  conv_act(m + ".mlp.1.conv", f0, 0, &dst, &x1);
}

// A2C2f(c1, c2, n, a2, area, residual, mlp_ratio, e = 0.5): cv1 -> y0 (c_ = c2 / 2 channels); member k maps y_k to y_{k+1} -- with a2 two
// ABlocks in sequence, without it a C3k(c_, c_, 2) --; cv2 on the concatenation of all of them. The concat is channel offsets into one
// buffer, as in C2f. With a `gamma` tensor (scales l / x: residual = True) the output is x + gamma[c] * cv2(...), one scale-add launch.
View YoloTrunk::a2c2f(const std::string& pfx, const View& x, int area, bool c3k_shortcut, const View* out_slice, const View* up_src) {
  const int c = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0];
  const bool a2 = net_.has(pfx + ".m.0.0.attn.qkv.conv.weight");
  int n = 0;
  while (net_.has(pfx + ".m." + std::to_string(n) + (a2 ? ".0.attn.qkv.conv.weight" : ".cv1.conv.weight"))) ++n;
  GTX_CHECK(n > 0 && c % 16 == 0 && (!a2 || (c % 32 == 0 && area >= 1)), "%s: %d members on %d hidden channels, area %d", pfx.c_str(), n, c, area);
  View cat = net_.new_view(x.h, x.w, (1 + n) * c);
  View first = cat.slice(0, c);
  conv(pfx + ".cv1.conv", x, 1, &first, nullptr, up_src);
  for (int k = 0; k < n; ++k) {
    const std::string m = pfx + ".m." + std::to_string(k);
    const View src = cat.slice(k * c, c), dst = cat.slice((k + 1) * c, c);
    if (a2) {
      const View mid = net_.new_view(x.h, x.w, c);
      ablock(m + ".0", src, mid, area);
      ablock(m + ".1", mid, dst, area);
      net_.set_layer_view(m, dst);
    } else {
      c3k(m, src, dst, c3k_shortcut);
    }
  }
  if (!(a2 && net_.has(pfx + ".gamma"))) {
    const View out = conv(pfx + ".cv2.conv", cat, 1, out_slice, nullptr);
    net_.set_layer_view(pfx, out);
    return out;
  }
  const HostTensor& gm = net_.tensor(pfx + ".gamma");
  const View y = conv(pfx + ".cv2.conv", cat, 1, nullptr, nullptr);
  GTX_CHECK((int)gm.data.size() == y.c && x.c == y.c && y.c % 8 == 0, "%s: gamma of %d values on %d -> %d channels", pfx.c_str(), (int)gm.data.size(), x.c, y.c);
  Op op;
  op.kind = Op::SCALEADD;
  op.name = pfx + ".gamma";
  op.family = "scale_add_kernel";
  op.in = y; op.dw_res = x;
  op.out = out_slice ? *out_slice : net_.new_view(x.h, x.w, y.c);
  op.dw_w = net_.upload(gm.data);
  op.sat = net_.sat_flag();
  ops_.push_back(op);
  net_.set_layer_view(pfx, op.out);
  return op.out;
}

View YoloTrunk::dwconv(const std::string& name, const View& x, int act, int stride, const View* out_slice, const View* residual) {
  const HostTensor& w = net_.tensor(name + ".weight");
  const int c = x.c;
  GTX_CHECK(w.shape.size() == 4 && (int)w.shape[0] == c && w.shape[1] == 1 && (w.shape[2] == 3 || w.shape[2] == 5 || w.shape[2] == 7) && w.shape[3] == w.shape[2] && c % 8 == 0,
            "%s: expected a depthwise 3x3, 5x5 or 7x7 convolution on %d channels", name.c_str(), c);
  const int k = (int)w.shape[2], taps = k * k;
  GTX_CHECK(stride == 1 || (stride == 2 && k == 3), "%s: stride %d", name.c_str(), stride);
  std::vector<float> wt = dw_tap_major(w.data.data(), c, taps), bias(c, 0.f);   // no bias tensor: zeros, the same sum
  if (const float* pb = net_.bias_of(name, c)) std::copy(pb, pb + c, bias.begin());
  const int ho = (x.h - 1) / stride + 1, wo = (x.w - 1) / stride + 1;
  Op op;
  op.kind = Op::DWCONV;
  op.name = name;
  op.family = rt_dwconv_kernel_name(k, stride, c);
  op.in = x;
  op.out = out_slice ? *out_slice : net_.new_view(ho, wo, c);
  GTX_CHECK(op.out.h == ho && op.out.w == wo && op.out.c == c, "%s: the output slice does not fit", name.c_str());
  if (residual) {
    GTX_CHECK(residual->h == ho && residual->w == wo && residual->c == c, "%s: the residual does not fit", name.c_str());
    op.dw_res = *residual;
  }
  op.dw_w = net_.upload(wt); op.dw_bias = net_.upload(bias);
  op.dw_act = act; op.dw_k = k; op.dw_stride = stride;
  op.sat = net_.sat_flag();
  ops_.push_back(op);
  net_.set_layer_view(name, op.out);
  return op.out;
}

// CIB(c, c, shortcut, e = 1.0, lk): dw3x3 -> 1x1 c -> 2c -> dw3x3 (lk: the fused RepVGGDW, one dw7x7) -> 1x1 2c -> c -> dw3x3, SiLU after
// each; src -> dst (+ src, in the last depthwise layer's epilogue after its activation)
View YoloTrunk::cib(const std::string& m, const View& src, const View& dst, bool shortcut) {
  const View d0 = dwconv(m + ".cv1.0.conv", src, 1);
  const View p1 = conv_act(m + ".cv1.1.conv", d0, 1, nullptr, nullptr);
  const View d2 = dwconv(m + ".cv1.2.conv", p1, 1);
  const View p3 = conv_act(m + ".cv1.3.conv", d2, 1, nullptr, nullptr);
  return dwconv(m + ".cv1.4.conv", p3, 1, 1, &dst, shortcut ? &src : nullptr);
}

// SCDown(c1, c2, 3, 2): cv2(cv1(x)), cv1 = 1x1 Conv + SiLU, cv2 = depthwise 3x3 stride 2 without activation
View YoloTrunk::scdown(const std::string& pfx, const View& x, const View* out_slice) {
  const View a = conv(pfx + ".cv1.conv", x, 1, nullptr, nullptr);
  const View out = dwconv(pfx + ".cv2.conv", a, 0, 2, out_slice);
  net_.set_layer_view(pfx, out);
  return out;
}

// ---- layer 0: the stem (dedicated 3-channel kernel). front: also the weights packed for fuse_stem()
View YoloTrunk::stem(const View& img, bool front) {
  const int fmt = net_.format();
  const HostTensor& w0 = net_.tensor("model.0.conv.weight");
  GTX_CHECK(w0.shape.size() == 4 && w0.shape[1] == 3 && (w0.shape[2] == 3 || w0.shape[2] == 6) && w0.shape[3] == w0.shape[2],
            "model.0 must be a 3x3 conv, or yolov5.yaml's 6x6, on 3 channels");
  if (w0.shape[2] == 6) return stem6(img);
  const int c0 = (int)w0.shape[0];
  View a0 = net_.new_view(img.h / 2, img.w / 2, c0);
  std::vector<float> w27((size_t)27 * c0);
  for (int o = 0; o < c0; ++o)
    for (int i = 0; i < 3; ++i)
      for (int y = 0; y < 3; ++y)
        for (int x = 0; x < 3; ++x)
          w27[(size_t)((y * 3 + x) * 3 + i) * c0 + o] = w0.data[(((size_t)o * 3 + i) * 3 + y) * 3 + x];
  float* dw = (float*)net_.alloc(w27.size() * sizeof(float));
  GTX_HIP(hipMemcpy(dw, w27.data(), w27.size() * sizeof(float), hipMemcpyHostToDevice));
  std::vector<float> b(c0, 0.f);
  if (net_.has("model.0.conv.bias")) b = net_.tensor("model.0.conv.bias").data;
  float* db = (float*)net_.alloc((size_t)(c0 + 31) / 32 * 32 * sizeof(float));   // zero-filled up to whole 32-channel groups (the MFMA stems read a group's bias unconditionally)
  GTX_HIP(hipMemcpy(db, b.data(), c0 * sizeof(float), hipMemcpyHostToDevice));
  auto upload_u16 = [&](const std::vector<uint16_t>& pk) {
    void* dp = net_.alloc(pk.size() * 2);
    GTX_HIP(hipMemcpy(dp, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
    return dp;
  };
  Op op;
  op.kind = Op::STEM;
  op.name = "model.0.conv";
  op.family = dtype_ == DT_F16 ? "stem_mfma_kernel" : (fmt == DT_F32S ? "stem_split_kernel" : "stem_kernel");
  op.in = img;
  op.out = a0;
  op.w27 = dw;
  op.bias = db;
  if (dtype_ == DT_F16) {
    op.wpk = upload_u16(pack_stem_weights_f16(w27.data(), c0));
  } else if (fmt == DT_F32S) {
    op.wpk = upload_u16(pack_stem_weights_split(w27.data(), c0, &op.stem_scale));
    if (front && c0 % 16 == 0) op.front_wpk = upload_u16(pack_front_weights_split(w27.data(), c0, &op.front_scale));   // fuse_stem(): whole 16-channel K chunks of model.1
  }
  ops_.push_back(op);
  net_.set_layer_view("model.0.conv", a0);
  return a0;
}

// yolov5.yaml's layer 0: Conv(3, c0, 6, 2, 2), its own kernels (stem6.hip) on weights in tap-major order [108][c0]. Nothing is packed
// for fuse_stem(): the fused front launch is built on the 27-tap stem.
View YoloTrunk::stem6(const View& img) {
  const int fmt = net_.format();
  const HostTensor& w0 = net_.tensor("model.0.conv.weight");
  const int c0 = (int)w0.shape[0];
  GTX_CHECK(c0 % 16 == 0 && c0 <= 96 && img.h >= 2 && img.w >= 2, "model.0: a 6x6 stem of %d channels on a %d x %d image", c0, img.w, img.h);
  View a0 = net_.new_view(stem6_out(img.h), stem6_out(img.w), c0);
  std::vector<float> w108((size_t)108 * c0);
  for (int o = 0; o < c0; ++o)
    for (int i = 0; i < 3; ++i)
      for (int y = 0; y < 6; ++y)
        for (int x = 0; x < 6; ++x) w108[(size_t)((y * 6 + x) * 3 + i) * c0 + o] = w0.data[(((size_t)o * 3 + i) * 6 + y) * 6 + x];
  std::vector<float> b((size_t)(c0 + 31) / 32 * 32, 0.f);     // whole 32-channel groups: the matrix-core kernels read a group's bias unconditionally
  if (const float* pb = net_.bias_of("model.0.conv", c0)) std::copy(pb, pb + c0, b.begin());
  auto upload_u16 = [&](const std::vector<uint16_t>& pk) {
    void* dp = net_.alloc(pk.size() * 2);
    GTX_HIP(hipMemcpy(dp, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
    return dp;
  };
  Op op;
  op.kind = Op::STEM;
  op.stem_k = 6;
  op.name = "model.0.conv";
  op.family = dtype_ == DT_F16 ? "stem6_mfma_kernel" : (fmt == DT_F32S ? "stem6_split_kernel" : "stem6_kernel");
  op.in = img;
  op.out = a0;
  op.w27 = net_.upload(w108);
  op.bias = net_.upload(b);
  if (dtype_ == DT_F16) op.wpk = upload_u16(pack_stem6_weights_f16(w108.data(), c0));
  else if (fmt == DT_F32S) op.wpk = upload_u16(pack_stem6_weights_split(w108.data(), c0, &op.stem_scale));
  ops_.push_back(op);
  net_.set_layer_view("model.0.conv", a0);
  return a0;
}

// The walk over a layer table, in yaml order. No Concat op exists: a row that a Concat lists writes straight into its slice of that
// Concat's buffer (members in the yaml's `from` order, widths off the tensor shapes), which the Concat's consumer reads whole.
YoloTrunk::Levels YoloTrunk::build(const View& img, const TrunkGraph& g, bool front) {
  const int n = g.n;
  auto name = [](int i) { return "model." + std::to_string(i); };
  auto cout_of = [&](const std::string& t) { return (int)net_.tensor(t + ".weight").shape[0]; };
  auto from = [&](const TrunkRow& r, int k) { return r.from[k] < 0 ? r.i + r.from[k] : r.from[k]; };   // row 0: -1, the image
  auto n_from = [](const TrunkRow& r) { int k = 0; while (k < 4 && r.from[k] != 0) ++k; return k; };

  GTX_CHECK(trunk_table_error(g.rows, n) < 0, "internal: layer table row %d", trunk_table_error(g.rows, n));
  // ---- output width of every row; the Concat (at most one) that lists it and its channel offset there
  std::vector<int> width(n, 0), cat_of(n, -1), cat_off(n, 0);
  bool fuse_up = net_.format() == DT_F32S;
  for (int i = 0; i < n; ++i) {
    const TrunkRow& r = g.rows[i];
    switch (r.mod) {
      case TrunkRow::CONV: width[i] = cout_of(name(i) + ".conv"); break;
      case TrunkRow::BLOCK: case TrunkRow::SPPF: case TrunkRow::C2PSA: case TrunkRow::SCDOWN: case TrunkRow::PSA: case TrunkRow::A2C2F: width[i] = cout_of(name(i) + ".cv2.conv"); break;
      case TrunkRow::ELAN: width[i] = cout_of(name(i) + ".cv4.conv"); break;
      case TrunkRow::C3: width[i] = cout_of(name(i) + ".cv3.conv"); break;
      case TrunkRow::ADOWN: width[i] = cout_of(name(i) + ".cv1.conv") + (net_.has(name(i) + ".cv2.conv.weight") ? cout_of(name(i) + ".cv2.conv") : 0); break;
      case TrunkRow::SPPELAN: width[i] = cout_of(name(i) + ".cv5.conv"); break;
      case TrunkRow::UPSAMPLE:
        // torch's Upsample + Concat in front of a block: the split-f16x3 path reads the low-resolution tensor in place from the
        // block's first 1x1 conv (ConvProblem::in2) when every such tensor of the graph is whole 32-channel groups (all or nothing),
        // the other arithmetics write the upsampled copy
        width[i] = width[from(r, 0)];
        fuse_up = fuse_up && width[i] % 32 == 0;
        break;
      case TrunkRow::CONCAT:
        for (int k = 0; k < n_from(r); ++k) {
          const int m = from(r, k);
          GTX_CHECK(cat_of[m] < 0, "internal: model.%d feeds two Concats (model.%d and model.%d)", m, cat_of[m], i);
          cat_of[m] = i;
          cat_off[m] = width[i];
          width[i] += width[m];
        }
        break;
      case TrunkRow::DETECT: break;
    }
  }

  // ---- the ops
  std::vector<View> out(n);         // per row; a Concat's: its whole buffer, allocated when its first member is placed
  std::vector<int> up_src(n, -1);   // per Concat under fuse_up: the row whose 2x upsampling its leading slice would hold (never written)
  View slot;
  auto place = [&](int i, int h, int w) -> const View* {   // where row i writes: null = a view of its own
    if (cat_of[i] < 0) return nullptr;
    View& c = out[cat_of[i]];
    if (!c.ptr) c = net_.new_view(h, w, width[cat_of[i]]);
    GTX_CHECK(c.h == h && c.w == w, "model.%d: %dx%d does not fit Concat model.%d (%dx%d)", i, w, h, cat_of[i], c.w, c.h);
    slot = c.slice(cat_off[i], width[i]);
    return &slot;
  };
  Levels lv;
  lv.dw_cls = g.dw_cls;
  for (int i = 0; i < n; ++i) {
    const TrunkRow& r = g.rows[i];
    const int f = from(r, 0);
    const View& x = i == 0 ? img : out[f];
    GTX_CHECK(i == 0 || r.mod == TrunkRow::DETECT || r.mod == TrunkRow::CONCAT || x.ptr, "internal: model.%d reads model.%d, which has no output", i, f);
    GTX_CHECK(i == 0 || up_src[f] < 0 || r.mod == TrunkRow::BLOCK || r.mod == TrunkRow::ELAN || r.mod == TrunkRow::A2C2F || r.mod == TrunkRow::C3, "internal: only a C2f / C3k2 / ELAN / A2C2f / C3 block reads an upsampled source in place (model.%d)", i);
    switch (r.mod) {
      case TrunkRow::CONV:
        if (i == 0) { out[i] = stem(img, front); break; }
        if (net_.tensor(name(i) + ".conv.weight").shape.size() == 4 && net_.tensor(name(i) + ".conv.weight").shape[2] == 1) {   // yolov5.yaml's Conv(c, 1, 1)
          out[i] = conv(name(i) + ".conv", x, 1, place(i, x.h, x.w), nullptr);
          break;
        }
        out[i] = conv(name(i) + ".conv", x, 2, place(i, (x.h - 1) / 2 + 1, (x.w - 1) / 2 + 1), nullptr);
        break;
      case TrunkRow::C3:
        out[i] = c3(name(i), x, r.shortcut, place(i, x.h, x.w), up_src[f] >= 0 ? &out[up_src[f]] : nullptr);
        break;
      case TrunkRow::BLOCK:
        out[i] = c2f(name(i), x, r.shortcut, place(i, x.h, x.w), up_src[f] >= 0 ? &out[up_src[f]] : nullptr);
        break;
      case TrunkRow::SPPF: {
        const View* s = place(i, x.h, x.w);
        out[i] = s ? *s : net_.new_view(x.h, x.w, width[i]);
        sppf(name(i), x, out[i], ".cv2.conv", r.shortcut);
        break;
      }
      case TrunkRow::C2PSA: out[i] = c2psa(name(i), x, place(i, x.h, x.w)); break;
      case TrunkRow::A2C2F:
        out[i] = a2c2f(name(i), x, r.area, r.shortcut, place(i, x.h, x.w), up_src[f] >= 0 ? &out[up_src[f]] : nullptr);
        break;
      case TrunkRow::PSA: out[i] = c2psa(name(i), x, place(i, x.h, x.w), true); break;
      case TrunkRow::ELAN:
        out[i] = elan(name(i), x, r.shortcut, place(i, x.h, x.w), up_src[f] >= 0 ? &out[up_src[f]] : nullptr);
        break;
      case TrunkRow::ADOWN: out[i] = adown(name(i), x, place(i, x.h / 2, x.w / 2)); break;
      case TrunkRow::SPPELAN: {
        const View* s = place(i, x.h, x.w);
        out[i] = s ? *s : net_.new_view(x.h, x.w, width[i]);
        sppf(name(i), x, out[i], ".cv5.conv");
        break;
      }
      case TrunkRow::SCDOWN: out[i] = scdown(name(i), x, place(i, (x.h - 1) / 2 + 1, (x.w - 1) / 2 + 1)); break;
      case TrunkRow::UPSAMPLE: {
        const View* s = place(i, 2 * x.h, 2 * x.w);
        GTX_CHECK(s && cat_off[i] == 0, "internal: Upsample model.%d must lead a Concat", i);
        if (!fuse_up) upsample(name(i), x, *s);
        break;
      }
      case TrunkRow::CONCAT:
        GTX_CHECK(out[i].ptr, "internal: Concat model.%d has no member in front of it", i);
        if (fuse_up && g.rows[f].mod == TrunkRow::UPSAMPLE) up_src[i] = from(g.rows[f], 0);
        break;
      case TrunkRow::DETECT:
        for (int k = 0; k < n_from(r); ++k) {
          lv.in.push_back(out[from(r, k)]);
          lv.strides.push_back((float)(img.h / lv.in.back().h));
        }
        lv.det_pfx = name(i);
        break;
    }
  }
  if (lv.in.empty()) lv.in.push_back(out[n - 1]);   // a table without a Detect row (the cls backbone): its last layer
  return lv;
}

void YoloTrunk::fuse() {
  fuse_front();
  fuse_stem();
  release_hidden_layers();
}

// model.1.conv (3x3 stride 2, all of its output channels in one cout tile) and model.2.cv1.conv (the 1x1 that is its only
// consumer) become one launch: ConvProblem::post_w. The 3x3 layer's output is never written; the launch writes the 1x1
// layer's. GTX_FUSE_FRONT=0 keeps the two launches. YOLOv8 n and s qualify (32 / 64 channels); the wider scales do not.
void YoloTrunk::fuse_front() {
  if (net_.format() != DT_F32S || !env_flag("GTX_FUSE_FRONT", true)) return;
  for (size_t i = 0; i + 1 < ops_.size(); ++i) {
    if (ops_[i].name != "model.1.conv" || ops_[i + 1].name != "model.2.cv1.conv") continue;
    const Op &a = ops_[i], &b = ops_[i + 1];
    if (a.kind != Op::CONV || b.kind != Op::CONV || a.grp.count != 1 || b.grp.count != 1) return;
    const ConvProblem &pa = a.grp.p[0], &pb = b.grp.p[0];
    const bool ok = a.cfg.variant == ConvForm::Split && a.cfg.ks == 3 && a.cfg.stride == 2 && pa.Cout == a.cfg.bn && !pa.res &&
                    b.cfg.variant == ConvForm::Split && b.cfg.ks == 1 && b.cfg.kc == 32 && b.cfg.bn == pb.Cout && pb.Cin == pa.Cout && pb.Cout == pa.Cout &&
                    pb.in == pa.out && pb.in_cstride == pa.out_cstride && pb.in_coff == pa.out_coff && !pb.res && !pb.in2;
    if (!ok) return;
    unfused_ = {a, b};
    Op f = a;
    f.name = "model.1.conv+model.2.cv1.conv";
    ConvProblem& p = f.grp.p[0];
    p.post_w = pb.wpack; p.post_bias = pb.bias; p.post_scale = pb.acc_scale; p.post_act = pb.act;
    p.out = pb.out; p.out_cstride = pb.out_cstride; p.out_coff = pb.out_coff; p.out_plain = pb.out_plain;
    ops_[i] = f;
    ops_.erase(ops_.begin() + (long)i + 1);
    return;
  }
}

// model.0.conv (the stem) moves into the launch of its only consumer, model.1.conv (already carrying model.2.cv1 when
// fuse_front() applied): ConvProblem::front_img. The stem's output -- the largest tensor of the network, 236 MB per two
// 1920 x 1920 frames -- is neither written nor read back; the workgroup recomputes the one-pixel halo of its patch (9.6 %).
// Built for model.1 in one cout tile and at most two 16-channel K chunks: YOLOv8 n (16 -> 32) and s (32 -> 64).
// GTX_FUSE_STEM=0 keeps the stem's own launch.
void YoloTrunk::fuse_stem() {
  if (net_.format() != DT_F32S || !env_flag("GTX_FUSE_STEM", true) || ops_.size() < 2) return;
  const Op& st = ops_[0];
  Op& cv = ops_[1];
  if (st.kind != Op::STEM || cv.kind != Op::CONV || cv.grp.count != 1 || !st.front_wpk) return;
  ConvProblem& p = cv.grp.p[0];
  const bool ok = cv.cfg.variant == ConvForm::Split && cv.cfg.ks == 3 && cv.cfg.stride == 2 && cv.cfg.kc == 16 && cv.cfg.th == 8 && ((cv.cfg.bn == 32 && p.Cin == 16) || (cv.cfg.bn == 64 && p.Cin == 32)) &&
                  p.Cout <= cv.cfg.bn && !p.res && p.in == st.out.ptr && p.in_cstride == st.out.c && p.in_coff == 0 && p.Cin == st.out.c &&
                  st.in.h == 2 * st.out.h && st.in.w == 2 * st.out.w && p.H == st.out.h && p.W == st.out.w;
  if (!ok) return;
  unfused_.insert(unfused_.begin(), st);
  p.front_img = st.in.ptr;
  p.front_w = st.front_wpk;
  p.front_bias = st.bias;
  p.front_scale = st.front_scale;
  p.front_h = st.in.h;
  p.front_w_px = st.in.w;
  cv.name = "model.0.conv+" + cv.name;
  cv.family = "conv_front_split_kernel";
  ops_.erase(ops_.begin());
}

// The stem's output and model.1's are written by no launch of the fused forward pass (354 MB per two 1920 x 1920 frames and
// detector): their buffers are given back here. layer_output() of one of them re-creates them and runs the stand-alone
// launches (unfused_). Until then every reference to them holds a token that is no device address. Only the trunk reads them:
// its own op list is all the liveness check needs to scan.
namespace {
void swap_ptr(Op& o, const void* from, void* to) {
  if (o.in.ptr == from) o.in.ptr = to;
  if (o.out.ptr == from) o.out.ptr = to;
  for (int i = 0; i < o.grp.count; ++i) {
    ConvProblem& p = o.grp.p[i];
    if (p.in == from) p.in = to;
    if (p.out == from) p.out = to;
    if (p.res == from) p.res = to;
    if (p.in2 == from) p.in2 = to;
  }
}
}  // namespace

void YoloTrunk::release_hidden_layers() {
  std::vector<void*> ptrs;
  for (size_t i = 0; i + 1 < unfused_.size() || (i < unfused_.size() && unfused_[i].kind == Op::STEM); ++i) {
    const Op& o = unfused_[i];                       // every stand-alone op but the last conv writes a hidden tensor
    void* out = o.kind == Op::STEM ? o.out.ptr : (o.grp.count == 1 ? o.grp.p[0].out : nullptr);
    if (out) ptrs.push_back(out);
  }
  for (void* ptr : ptrs) {
    bool live = false;                               // still written or read by a launch of the forward pass?
    for (const Op& o : ops_) {
      if (o.kind != Op::CONV && (o.in.ptr == ptr || o.out.ptr == ptr)) live = true;
      for (int i = 0; i < o.grp.count; ++i) {
        const ConvProblem& q = o.grp.p[i];
        const bool reads_in = !q.front_img;          // a front stage computes its input patch from the image instead of loading it
        if ((reads_in && q.in == ptr) || q.out == ptr || q.res == ptr || q.in2 == ptr) live = true;
      }
    }
    if (live) continue;
    const size_t bytes = net_.release_buffer(ptr);
    if (!bytes) continue;
    void* token = reinterpret_cast<void*>(static_cast<uintptr_t>(16 * (hidden_.size() + 1)));
    hidden_.push_back({token, bytes, nullptr});
    for (Op& o : unfused_) swap_ptr(o, ptr, token);
    net_.repoint_layer_views(ptr, token);
  }
}

void YoloTrunk::materialize_hidden_layers() {
  for (Hidden& h : hidden_) {
    if (h.real) continue;
    h.real = net_.alloc(h.bytes);
    for (Op& o : unfused_) swap_ptr(o, h.token, h.real);
    net_.repoint_layer_views(h.token, h.real);
  }
}

bool YoloTrunk::hidden(const void* p) const {
  for (const Hidden& h : hidden_)
    if (!h.real && h.token == p) return true;
  return false;
}

bool YoloTrunk::recompute_hidden(const std::string& layer, int nb, hipStream_t s) {
  // model.0 / model.1 of a fused front launch are RECOMPUTED here by their stand-alone launches (same products, another
  // summation order): what comes back is not what the network consumed. The last entry of unfused_ is a layer the fused
  // launch does write.
  int k = -1;
  for (size_t i = 0; i < unfused_.size(); ++i) {
    const bool still_written = i + 1 == unfused_.size() && unfused_[i].kind != Op::STEM;   // the fused launch's own output layer
    if (!still_written && unfused_[i].name == layer) k = (int)i;
  }
  if (k < 0) return false;
  GTX_CHECK(nb > 0, "layer_output('%s'): no forward pass has run yet", layer.c_str());
  GTX_HIP(hipSetDevice(net_.device()));
  materialize_hidden_layers();
  for (int j = 0; j <= k; ++j) {
    Op o = unfused_[(size_t)j];
    if (o.kind == Op::CONV) {
      for (int i = 0; i < o.grp.count; ++i) o.grp.p[i].N = nb;
      conv_group_finalize(o.grp, o.cfg);
    }
    run_op(o, nb, s);
  }
  GTX_HIP(hipStreamSynchronize(s));
  return true;
}

void YoloTrunk::run_op(const Op& op, int nb, hipStream_t s) const {
  const int fmt = net_.format();
  switch (op.kind) {
    case Op::CONV:
      conv_launch(op.grp, op.cfg, s);
      break;
    case Op::STEM:
      if (op.stem_k == 6) {
        launch_stem6(dtype_ == DT_F32 ? fmt : dtype_, op.in.ptr, nb, op.in.h, op.in.w, op.w27, op.bias, op.wpk, op.out.c, op.out.ptr, op.out.h, op.out.w, s,
                     op.stem_scale);
        break;
      }
      launch_stem(dtype_ == DT_F32 ? fmt : dtype_, op.in.ptr, nb, op.in.h, op.in.w, op.w27, op.bias, op.wpk, op.out.c, op.out.ptr, op.out.h,
                  op.out.w, s, op.stem_scale);
      break;
    case Op::POOL: launch_sppf_pool(fmt == DT_F32S ? DT_F32S : dtype_, op.out.ptr, nb, op.in.h, op.in.w, op.in.c, s); break;
    case Op::UPSAMPLE:
      // a raw copy: all it needs is what a stored element takes -- 2 bytes under half, 4 in fp32 and in the pair format (dtype_ is
      // DT_F32 there), also where the net allocates more per element than it stores (rtdetr-l's fp16 maps in 4-byte slots)
      launch_upsample2x(dtype_size(dtype_), op.in.ptr, nb, op.in.h, op.in.w, op.in.c, op.in.cstride, op.in.coff, op.out.ptr,
                        op.out.cstride, op.out.coff, s);
      break;
    case Op::DWCONV: {
      const RtMap res = op.dw_res.map();
      launch_rt_dwconv(fmt, op.in.map(), op.out.map(), nb, op.dw_k, op.dw_stride, op.dw_w, op.dw_bias, op.dw_act, op.sat, s, res.ptr ? &res : nullptr);
      break;
    }
    case Op::POOLDOWN: launch_pool_down(fmt, op.in.map(), op.out.map(), op.out2.map(), nb, s); break;
    case Op::ATTN: launch_psa_attention(fmt, op.in.map(), op.out.map(), nb, op.heads, op.dw_w, op.dw_bias, op.sat, s); break;
    case Op::AREAATTN: launch_area_attention(fmt, op.in.map(), op.out.map(), nb, op.heads, op.area, true, op.sat, s); break;
    case Op::SCALEADD: launch_scale_add(fmt, op.in.map(), op.dw_res.map(), op.out.map(), nb, op.dw_w, op.sat, s); break;
  }
}

void set_batch_op(Op& op, int nb, size_t es, bool pad_skip_on) {
  if (op.kind == Op::CONV) {
    for (int i = 0; i < op.grp.count; ++i) {
      op.grp.p[i].N = nb;
      op.grp.p[i].ty_first = pad_skip_on ? op.ty_first[i] : 0;
      op.grp.p[i].ty_count = pad_skip_on ? op.ty_count[i] : 0;
    }
    conv_group_finalize(op.grp, op.cfg);
    op.flops = 0;
    op.bytes = 0;
    for (int i = 0; i < op.grp.count; ++i) {
      const ConvProblem& p = op.grp.p[i];
      // the share of the output rows this launch computes (letterbox-padding rows are skipped: plan_pad_skip)
      const double part = std::min(1.0, (double)p.tiles_y * op.cfg.th / p.Ho);
      op.flops += part * conv_flops(p, op.cfg.ks);
      op.bytes += part * ((double)p.N * p.H * p.W * (p.Cin - 0.75 * p.c_split) + (double)p.N * p.Ho * p.Wo * p.Cout) * es +
                  (double)p.Cout * p.Cin * op.cfg.ks * op.cfg.ks * es;
      if (p.post_w) {                     // the fused 1x1 layer: its FLOPs and weights; its output replaces the 3x3 layer's (same size)
        op.flops += part * 2.0 * p.N * p.Ho * p.Wo * (double)p.Cout * p.Cout;
        op.bytes += (double)p.Cout * p.Cout * es;
      }
      if (p.front_img) {                  // the fused stem: its FLOPs; RGB0 bytes are read instead of the stem's output
        op.flops += part * 2.0 * p.N * p.H * p.W * (double)p.Cin * 27;
        op.bytes += part * ((double)p.N * p.front_h * p.front_w_px * 4 - (double)p.N * p.H * p.W * p.Cin * es);
      }
    }
  } else if (op.kind == Op::STEM) {
    op.flops = 2.0 * nb * op.out.h * op.out.w * op.out.c * 3 * op.stem_k * op.stem_k;
    op.bytes = (double)nb * ((double)op.in.h * op.in.w * 4 + (double)op.out.h * op.out.w * op.out.c * es);   // RGB0 bytes in
  } else if (op.kind == Op::POOL) {
    op.flops = 0;
    op.bytes = (double)nb * op.in.h * op.in.w * op.in.c * 4 * es;
  } else if (op.kind == Op::UPSAMPLE) {
    op.flops = 0;
    op.bytes = (double)nb * op.in.h * op.in.w * op.in.c * 5 * es;
  } else if (op.kind == Op::DWCONV) {
    op.flops = 2.0 * op.dw_k * op.dw_k * nb * op.out.h * op.out.w * op.in.c;
    op.bytes = (double)nb * ((double)op.in.h * op.in.w + (double)op.out.h * op.out.w * (op.dw_res.ptr ? 2 : 1)) * op.in.c * es;
  } else if (op.kind == Op::POOLDOWN) {             // three additions per averaged element, eight maxima per maximum; every map once
    op.flops = (double)nb * op.in.h * op.in.w * (3.0 * op.out.c + 3.0 * op.out2.c) + 8.0 * nb * op.out2.h * op.out2.w * op.out2.c;
    op.bytes = (double)nb * ((double)op.in.h * op.in.w * (op.in.c + op.out.c) + (double)op.out2.h * op.out2.w * op.out2.c) * es;
  } else if (op.kind == Op::ATTN) {                 // q.k (depth 32) + p.v (width 64) per query-key pair and head, + pe; the qkv map in, the output map out
    const double T = (double)op.in.h * op.in.w;
    op.flops = nb * (op.heads * T * T * 2.0 * (32 + 64) + 2.0 * 9 * T * op.out.c);
    op.bytes = nb * T * (op.in.c + op.out.c) * es;
  } else if (op.kind == Op::AREAATTN) {             // q.k and p.v (width 32 each) per query-key pair of a band and head; the qkv map in, the output map out
    const double T = (double)op.in.h * op.in.w;
    op.flops = nb * op.heads * T * (T / op.area) * 2.0 * (32 + 32);
    op.bytes = nb * T * (op.in.c + op.out.c) * es;
  } else if (op.kind == Op::SCALEADD) {
    op.flops = 2.0 * nb * op.out.h * op.out.w * op.out.c;
    op.bytes = 3.0 * nb * op.out.h * op.out.w * op.out.c * es;
  }
}

void set_batch_ops(std::vector<Op>& ops, int nb, size_t es, bool pad_skip_on) {
  for (Op& op : ops) set_batch_op(op, nb, es, pad_skip_on);
}

}  // namespace gtx
