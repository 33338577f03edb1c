// YoloTrunk (yolo_trunk.hpp): the YOLOv8 / YOLOv8-P2 backbone + neck, shared by the YOLOv8 detector and YOLOv8-RTDETR. Layer
// topology follows ultralytics' cfg/models/v8/yolov8.yaml (backbone 0-9, head 10-21) or yolov8-p2.yaml (head 10-27, one more
// stage at stride 4); channel widths and bottleneck counts are read off the tensor shapes, so every v8 scale (n/s/m/l/x) loads unchanged.
#include "yolo_trunk.hpp"
#include "rtdetr_kernels.hpp"
#include "split_format.hpp"

#include <algorithm>

namespace gtx {

View YoloTrunk::conv(const std::string& name, const View& x, int stride, const View* out_slice, const View* residual, const View* up_src) {
  GTX_CHECK(net_.format() != DT_F32S || !up_src || !up_src->plain, "%s: a plain fp32 tensor cannot feed a split convolution", name.c_str());
  NetRuntime::ConvArgs a;
  a.stride = stride; a.act = 1; a.out_slice = out_slice; a.residual = residual;
  const View out = net_.emit_named_conv(ops_, name, x, a);
  if (up_src) {
    Op& op = ops_.back();
    if (op.cfg.variant == 6) op.cfg.variant = 2;     // the second source is read by the 32x32x16 kernel only (same weight image)
    GTX_CHECK(op.cfg.ks == 1 && stride == 1 && op.cfg.variant == 2 && up_src->h * 2 == x.h && up_src->w * 2 == x.w && up_src->c < x.c,
              "%s: upsampled source does not fit", name.c_str());
    ConvProblem& p = op.grp.p[0];
    p.in2 = up_src->ptr; p.in2_cstride = up_src->cstride; p.in2_coff = up_src->coff; p.c_split = up_src->c;
    op.family = conv_kernel_name(op.cfg);
  }
  return out;
}

View YoloTrunk::c2f(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src) {
  const HostTensor& w1 = net_.tensor(pfx + ".cv1.conv.weight");
  const int c = (int)w1.shape[0] / 2;
  int n = 0;
  while (net_.has(pfx + ".m." + std::to_string(n) + ".cv1.conv.weight")) ++n;
  View cat = net_.new_view(x.h, x.w, (2 + n) * c);
  View first = cat.slice(0, 2 * c);
  conv(pfx + ".cv1.conv", x, 1, &first, nullptr, up_src);
  for (int k = 0; k < n; ++k) {
    // a buffer of its own per bottleneck: rows that no launch rewrites (plan_pad_skip) must keep ONE producer's values
    View tmp = net_.new_view(x.h, x.w, c);
    const std::string m = pfx + ".m." + std::to_string(k);
    View src = cat.slice((1 + k) * c, c);
    View dst = cat.slice((2 + k) * c, c);
    conv(m + ".cv1.conv", src, 1, &tmp, nullptr);
    conv(m + ".cv2.conv", tmp, 1, &dst, shortcut ? &src : nullptr);
  }
  View out = conv(pfx + ".cv2.conv", cat, 1, out_slice, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

void YoloTrunk::upsample(const std::string& name, const View& src, const View& dst) {
  Op op;
  op.kind = Op::UPSAMPLE;
  op.name = name;
  op.family = "upsample2x_kernel";
  op.in = src;
  op.out = dst;
  ops_.push_back(op);
}

// ---- SPPF (model.9): cv1 -> 3 cascaded pools -> cv2; its output is written into the slice `s9` of the last Concat
void YoloTrunk::sppf(const View& a8, const View& s9) {
  const int cm = (int)net_.tensor("model.9.cv1.conv.weight").shape[0];
  View sp = net_.new_view(a8.h, a8.w, 4 * cm);
  View sp0 = sp.slice(0, cm);
  conv("model.9.cv1.conv", a8, 1, &sp0, nullptr);
  Op op;
  op.kind = Op::POOL;
  op.name = "model.9.m";
  op.family = "sppf_pool_kernel";
  op.in = sp0;
  op.out = sp;
  ops_.push_back(op);
  conv("model.9.cv2.conv", sp, 1, &s9, nullptr);
  net_.set_layer_view("model.9", s9);
}

// ============================================================================ YOLO11 (ultralytics cfg/models/11/yolo11.yaml)
// One stride-1 Conv op with the given activation (0 none, 1 SiLU). The convolution kernels take channel counts that are
// multiples of 16: a narrower layer (the 8-channel hidden layer of scale n's model.2 bottleneck) gets zero output channels
// appended -- SiLU(0) = 0 -- and its consumer zero input weights for them, which changes no sum.
View YoloTrunk::conv_act(const std::string& name, const View& x, int act, const View* out_slice, const View* residual) {
  const HostTensor& w = net_.tensor(name + ".weight");
  GTX_CHECK(w.shape.size() == 4 && w.shape[2] == w.shape[3], "%s: expected OIHW square kernel", name.c_str());
  const int cout = (int)w.shape[0], cin = (int)w.shape[1], ks = (int)w.shape[2], taps = ks * ks;
  const int cout_p = (cout + 15) / 16 * 16, cin_p = x.c;
  NetRuntime::ConvArgs a;
  a.act = act; a.out_slice = out_slice; a.residual = residual;
  if (cout_p == cout && cin_p == cin) return net_.emit_named_conv(ops_, name, x, a);
  GTX_CHECK(cin_p >= cin && (cout_p == cout || (!out_slice && !residual)), "%s: %d -> %d channels cannot be padded here", name.c_str(), cin, cout);
  std::vector<float> wp((size_t)cout_p * cin_p * taps, 0.f), bp(cout_p, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int i = 0; i < cin; ++i)
      for (int t = 0; t < taps; ++t) wp[((size_t)o * cin_p + i) * taps + t] = w.data[((size_t)o * cin + i) * taps + t];
  if (const float* b = net_.bias_of(name, cout)) std::copy(b, b + cout, bp.begin());
  a.out_pixels = (long)x.n * x.h * x.w;
  return net_.emit_conv(ops_, name, wp.data(), cout_p, cin_p, ks, bp.data(), x, a);
}

// Bottleneck(c, c, shortcut, k = (3, 3), e): src -> dst (+ src); the hidden width is read off cv1 (c / 2 in C3k2, c in C3k)
View YoloTrunk::bottleneck_half(const std::string& m, const View& src, const View& dst, bool shortcut) {
  const View tmp = conv_act(m + ".cv1.conv", src, 1, nullptr, nullptr);   // a buffer of its own, as in c2f()
  return conv_act(m + ".cv2.conv", tmp, 1, &dst, shortcut ? &src : nullptr);
}

// C3k: cv3(cat(m(cv1(x)), cv2(x))), m = Bottlenecks of full hidden width
View YoloTrunk::c3k(const std::string& m, const View& src, const View& dst, bool shortcut) {
  const int ch = (int)net_.tensor(m + ".cv1.conv.weight").shape[0];
  int n = 0;
  while (net_.has(m + ".m." + std::to_string(n) + ".cv1.conv.weight")) ++n;
  View cat = net_.new_view(src.h, src.w, 2 * ch);
  View left = cat.slice(0, ch), right = cat.slice(ch, ch);
  View y = n == 0 ? left : net_.new_view(src.h, src.w, ch);
  conv_act(m + ".cv1.conv", src, 1, &y, nullptr);
  for (int j = 0; j < n; ++j) {
    View nxt = j + 1 == n ? left : net_.new_view(src.h, src.w, ch);
    bottleneck_half(m + ".m." + std::to_string(j), y, nxt, shortcut);
    y = nxt;
  }
  conv_act(m + ".cv2.conv", src, 1, &right, nullptr);
  return conv_act(m + ".cv3.conv", cat, 1, &dst, nullptr);
}

// C3k2 = C2f whose m.{k} is a half-width Bottleneck (c3k = False) or a C3k (c3k = True: the block has a cv3)
View YoloTrunk::c3k2(const std::string& pfx, const View& x, bool shortcut, const View* out_slice, const View* up_src) {
  const int c = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0] / 2;
  int n = 0;
  while (net_.has(pfx + ".m." + std::to_string(n) + ".cv1.conv.weight")) ++n;
  View cat = net_.new_view(x.h, x.w, (2 + n) * c);
  View first = cat.slice(0, 2 * c);
  conv(pfx + ".cv1.conv", x, 1, &first, nullptr, up_src);
  for (int k = 0; k < n; ++k) {
    const std::string m = pfx + ".m." + std::to_string(k);
    View src = cat.slice((1 + k) * c, c), dst = cat.slice((2 + k) * c, c);
    if (net_.has(m + ".cv3.conv.weight")) c3k(m, src, dst, shortcut); else bottleneck_half(m, src, dst, shortcut);
  }
  View out = conv(pfx + ".cv2.conv", cat, 1, out_slice, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

// C2PSA: cv1 -> a | b; per PSABlock b += proj(attention(qkv(b)) + pe(v)), b += ffn.1(ffn.0(b)); cv2 on cat(a, b). The convolutions
// without activation take the residual in their epilogue (activation first, then the residual: x + conv(x)). The last block
// writes b back into cv1's buffer, which cv2 then reads whole.
View YoloTrunk::c2psa(const std::string& pfx, const View& x, const View* out_slice) {
  const int c = (int)net_.tensor(pfx + ".cv1.conv.weight").shape[0] / 2;
  GTX_CHECK(c % 64 == 0, "%s: %d hidden channels are not whole 64-wide attention heads", pfx.c_str(), c);
  const int heads = c / 64;
  int n = 0;
  while (net_.has(pfx + ".m." + std::to_string(n) + ".attn.qkv.conv.weight")) ++n;
  GTX_CHECK(n > 0, "%s: no PSABlock", pfx.c_str());
  View ab = conv(pfx + ".cv1.conv", x, 1, nullptr, nullptr);
  View b = ab.slice(c, c);
  for (int k = 0; k < n; ++k) {
    const std::string m = pfx + ".m." + std::to_string(k);
    const HostTensor &wq = net_.tensor(m + ".attn.qkv.conv.weight"), &wp = net_.tensor(m + ".attn.pe.conv.weight");
    GTX_CHECK((int)wq.shape[0] == heads * 128 && wp.shape.size() == 4 && (int)wp.shape[0] == c && wp.shape[1] == 1 && wp.shape[2] == 3,
              "%s: attention of %d heads with key_dim 32 / head_dim 64 expected", m.c_str(), heads);
    const View qkv = conv_act(m + ".attn.qkv.conv", b, 0, nullptr, nullptr);
    View att = net_.new_view(x.h, x.w, c);
    {
      std::vector<float> wt((size_t)9 * c);
      for (int ch = 0; ch < c; ++ch)
        for (int t = 0; t < 9; ++t) wt[(size_t)t * c + ch] = wp.data[(size_t)ch * 9 + t];
      std::vector<float> bias(c, 0.f);
      if (const float* pb = net_.bias_of(m + ".attn.pe.conv", c)) std::copy(pb, pb + c, bias.begin());
      Op op;
      op.kind = Op::ATTN;
      op.name = m + ".attn";
      op.family = "psa_attn_kernel";
      op.in = qkv; op.out = att;
      op.heads = heads;
      op.dw_w = net_.upload(wt); op.dw_bias = net_.upload(bias);
      op.sat = net_.sat_flag();
      ops_.push_back(op);
      net_.set_layer_view(m + ".attn.out", att);       // softmax(q^T k) v + pe(v): what proj reads
    }
    View b1 = net_.new_view(x.h, x.w, c);
    conv_act(m + ".attn.proj.conv", att, 0, &b1, &b);
    const View f0 = conv_act(m + ".ffn.0.conv", b1, 1, nullptr, nullptr);
    View b2 = k + 1 == n ? ab.slice(c, c) : net_.new_view(x.h, x.w, c);
    conv_act(m + ".ffn.1.conv", f0, 0, &b2, &b1);
    b = b2;
  }
  View out = conv(pfx + ".cv2.conv", ab, 1, out_slice, nullptr);
  net_.set_layer_view(pfx, out);
  return out;
}

View YoloTrunk::dwconv(const std::string& name, const View& x, int act) {
  const HostTensor& w = net_.tensor(name + ".weight");
  const int c = x.c;
  GTX_CHECK(w.shape.size() == 4 && (int)w.shape[0] == c && w.shape[1] == 1 && w.shape[2] == 3 && w.shape[3] == 3 && c % 8 == 0,
            "%s: expected a depthwise 3x3 convolution on %d channels", name.c_str(), c);
  std::vector<float> wt((size_t)9 * c), bias(c, 0.f);
  for (int ch = 0; ch < c; ++ch)
    for (int t = 0; t < 9; ++t) wt[(size_t)t * c + ch] = w.data[(size_t)ch * 9 + t];
  if (const float* pb = net_.bias_of(name, c)) std::copy(pb, pb + c, bias.begin());
  Op op;
  op.kind = Op::DWCONV;
  op.name = name;
  op.family = c % 32 == 0 ? "rt_dwconv_tile_kernel<3>" : "rt_dwconv_kernel<3>";     // launch_rt_dwconv's rule
  op.in = x;
  op.out = net_.new_view(x.h, x.w, c);
  op.dw_w = net_.upload(wt); op.dw_bias = net_.upload(bias);
  op.dw_act = act;
  op.sat = net_.sat_flag();
  ops_.push_back(op);
  net_.set_layer_view(name, op.out);
  return op.out;
}

// Backbone 0-10 (C3k2 stages, SPPF, C2PSA), neck 11-22, Detect = model.23 on 16 / 19 / 22. Widths, repeats and c3k-or-not are read
// off the tensors, so every scale (n / s / m / l / x) loads unchanged. Shortcuts: on in the backbone; in the neck kNeckShortcut, which
// no tensor tells (taken as off, as in yolov8.yaml's neck; tests/yolo11_ref.py names the doubt).
YoloTrunk::Levels YoloTrunk::build_yolo11(const View& a0) {
  constexpr bool kNeckShortcut = false;
  const int H = a0.h * 2, W = a0.w * 2, fmt = net_.format();
  auto cout_of = [&](const std::string& n) { return (int)net_.tensor(n + ".weight").shape[0]; };
  const int c4 = cout_of("model.4.cv2.conv"), c6 = cout_of("model.6.cv2.conv"), c9 = cout_of("model.9.cv2.conv");
  const int c10 = cout_of("model.10.cv2.conv"), c13 = cout_of("model.13.cv2.conv");
  const int c17 = cout_of("model.17.conv"), c20 = cout_of("model.20.conv");
  View a1 = conv("model.1.conv", a0, 2, nullptr, nullptr);
  View a2 = c3k2("model.2", a1, true, nullptr);
  View a3 = conv("model.3.conv", a2, 2, nullptr, nullptr);
  View cat15 = net_.new_view(H / 8, W / 8, c13 + c4);             // [up14, model.4]
  View s4 = cat15.slice(c13, c4);
  View a4 = c3k2("model.4", a3, true, &s4);
  View a5 = conv("model.5.conv", a4, 2, nullptr, nullptr);
  View cat12 = net_.new_view(H / 16, W / 16, c10 + c6);           // [up11, model.6]
  View s6 = cat12.slice(c10, c6);
  View a6 = c3k2("model.6", a5, true, &s6);
  View a7 = conv("model.7.conv", a6, 2, nullptr, nullptr);
  View a8 = c3k2("model.8", a7, true, nullptr);
  View s9 = net_.new_view(H / 32, W / 32, c9);
  sppf(a8, s9);
  View cat21 = net_.new_view(H / 32, W / 32, c20 + c10);          // [conv20, model.10]
  View s10 = cat21.slice(c20, c10);
  c2psa("model.10", s9, &s10);
  // Upsample + Concat in front of model.13 / model.16: read in place by the C3k2's first 1x1 on the split-f16x3 path (as in yolov8.yaml)
  const bool fuse_up = fmt == DT_F32S && c10 % 32 == 0 && c13 % 32 == 0;
  if (!fuse_up) upsample("model.11", s10, cat12.slice(0, c10));
  View cat18 = net_.new_view(H / 16, W / 16, c17 + c13);          // [conv17, model.13]
  View s13 = cat18.slice(c17, c13);
  c3k2("model.13", cat12, kNeckShortcut, &s13, fuse_up ? &s10 : nullptr);
  if (!fuse_up) upsample("model.14", s13, cat15.slice(0, c13));
  View a16 = c3k2("model.16", cat15, kNeckShortcut, nullptr, fuse_up ? &s13 : nullptr);
  View s17 = cat18.slice(0, c17);
  conv("model.17.conv", a16, 2, &s17, nullptr);
  View a19 = c3k2("model.19", cat18, kNeckShortcut, nullptr);
  View s20 = cat21.slice(0, c20);
  conv("model.20.conv", a19, 2, &s20, nullptr);
  View a22 = c3k2("model.22", cat21, kNeckShortcut, nullptr);
  Levels lv;
  lv.in = {a16, a19, a22};
  lv.strides = {8.f, 16.f, 32.f};
  lv.det_pfx = "model.23";
  lv.dw_cls = true;
  return lv;
}

YoloTrunk::Levels YoloTrunk::build(const View& img) {
  const int H = img.h, W = img.w;
  const int fmt = net_.format();

  // ---- layer 0: stem (dedicated 3-channel kernel) ----
  const HostTensor& w0 = net_.tensor("model.0.conv.weight");
  GTX_CHECK(w0.shape.size() == 4 && w0.shape[1] == 3 && w0.shape[2] == 3, "model.0 must be a 3x3 conv on 3 channels");
  const int c0 = (int)w0.shape[0];
  View a0 = net_.new_view(H / 2, W / 2, c0);
  {
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
    Op op;
    op.kind = Op::STEM;
    op.name = "model.0.conv";
    op.family = dtype_ == DT_F16 ? "stem_mfma_kernel" : (fmt == DT_F32S ? "stem_split_kernel" : "stem_kernel");
    op.in = img;
    op.out = a0;
    op.w27 = dw;
    op.bias = db;
    if (dtype_ == DT_F16) {
      const std::vector<uint16_t> pk = pack_stem_weights_f16(w27.data(), c0);
      void* dp = net_.alloc(pk.size() * 2);
      GTX_HIP(hipMemcpy(dp, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
      op.wpk = dp;
    } else if (fmt == DT_F32S) {
      const std::vector<uint16_t> pk = pack_stem_weights_split(w27.data(), c0, &op.stem_scale);
      void* dp = net_.alloc(pk.size() * 2);
      GTX_HIP(hipMemcpy(dp, pk.data(), pk.size() * 2, hipMemcpyHostToDevice));
      op.wpk = dp;
      if (c0 % 16 == 0) {                       // fuse_stem(): whole 16-channel K chunks of model.1
        const std::vector<uint16_t> fk = pack_front_weights_split(w27.data(), c0, &op.front_scale);
        void* fp = net_.alloc(fk.size() * 2);
        GTX_HIP(hipMemcpy(fp, fk.data(), fk.size() * 2, hipMemcpyHostToDevice));
        op.front_wpk = fp;
      }
    }
    ops_.push_back(op);
    net_.set_layer_view("model.0.conv", a0);
  }

  auto cout_of = [&](const std::string& n) { return (int)net_.tensor(n + ".weight").shape[0]; };
  // yolov8.yaml (Detect = model.22 on 15 / 18 / 21) or yolov8-p2.yaml (one more Upsample + Concat + C2f at stride 4 in the neck,
  // Detect = model.28 on 18 / 21 / 24 / 27): told apart by the tensor names, like the reference's model yaml does
  const bool p2 = net_.has("model.28.cv2.0.0.conv.weight");
  // yolo11.yaml: C2PSA at model.10 and Detect (depthwise class branch) at model.23 -- names no YOLOv8 file has
  if (net_.has("model.10.m.0.attn.qkv.conv.weight") && net_.has("model.23.cv3.0.0.0.conv.weight")) return build_yolo11(a0);
  Levels lv;
  if (!p2) {
    // ---- backbone ----
    View a1 = conv("model.1.conv", a0, 2, nullptr, nullptr);
    View a2 = c2f("model.2", a1, true, nullptr);
    View a3 = conv("model.3.conv", a2, 2, nullptr, nullptr);
    // model.4 output feeds conv5 and Concat(14) = [up13, model.4]
    const int c4 = cout_of("model.4.cv2.conv"), c6 = cout_of("model.6.cv2.conv");
    const int c9 = cout_of("model.9.cv2.conv"), c12 = cout_of("model.12.cv2.conv");
    const int c16 = cout_of("model.16.conv"), c19 = cout_of("model.19.conv");
    View cat14 = net_.new_view(H / 8, W / 8, c12 + c4);
    View s4 = cat14.slice(c12, c4);
    View a4 = c2f("model.4", a3, true, &s4);
    View a5 = conv("model.5.conv", a4, 2, nullptr, nullptr);
    View cat11 = net_.new_view(H / 16, W / 16, c9 + c6);
    View s6 = cat11.slice(c9, c6);
    View a6 = c2f("model.6", a5, true, &s6);
    View a7 = conv("model.7.conv", a6, 2, nullptr, nullptr);
    View a8 = c2f("model.8", a7, true, nullptr);
    // SPPF output lives in Concat(20) = [conv19, model.9]
    View cat20 = net_.new_view(H / 32, W / 32, c19 + c9);
    View s9 = cat20.slice(c19, c9);
    sppf(a8, s9);
    // ---- head ----
    // torch's Upsample + Concat in front of model.12 / model.15: the split-f16x3 path reads the low-resolution tensor in
    // place from the C2f's first 1x1 conv (ConvProblem::in2), the other arithmetics write the upsampled copy
    const bool fuse_up = fmt == DT_F32S && c9 % 32 == 0 && c12 % 32 == 0;
    if (!fuse_up) upsample("model.10", s9, cat11.slice(0, c9));
    View cat17 = net_.new_view(H / 16, W / 16, c16 + c12);
    View s12 = cat17.slice(c16, c12);
    c2f("model.12", cat11, false, &s12, fuse_up ? &s9 : nullptr);
    if (!fuse_up) upsample("model.13", s12, cat14.slice(0, c12));
    View a15 = c2f("model.15", cat14, false, nullptr, fuse_up ? &s12 : nullptr);
    View s16 = cat17.slice(0, c16);
    conv("model.16.conv", a15, 2, &s16, nullptr);
    View a18 = c2f("model.18", cat17, false, nullptr);
    View s19 = cat20.slice(0, c19);
    conv("model.19.conv", a18, 2, &s19, nullptr);
    View a21 = c2f("model.21", cat20, false, nullptr);
    lv.in = {a15, a18, a21};
    lv.strides = {8.f, 16.f, 32.f};
    lv.det_pfx = "model.22";
  } else {
    // ---- backbone (as yolov8.yaml); model.2's output also feeds Concat(17) = [up16, model.2] ----
    const int c2 = cout_of("model.2.cv2.conv"), c4 = cout_of("model.4.cv2.conv"), c6 = cout_of("model.6.cv2.conv");
    const int c9 = cout_of("model.9.cv2.conv"), c12 = cout_of("model.12.cv2.conv"), c15 = cout_of("model.15.cv2.conv");
    const int c19 = cout_of("model.19.conv"), c22 = cout_of("model.22.conv"), c25 = cout_of("model.25.conv");
    View a1 = conv("model.1.conv", a0, 2, nullptr, nullptr);
    View cat17 = net_.new_view(H / 4, W / 4, c15 + c2);
    View s2 = cat17.slice(c15, c2);
    View a2 = c2f("model.2", a1, true, &s2);
    View a3 = conv("model.3.conv", a2, 2, nullptr, nullptr);
    View cat14 = net_.new_view(H / 8, W / 8, c12 + c4);           // [up13, model.4]
    View s4 = cat14.slice(c12, c4);
    View a4 = c2f("model.4", a3, true, &s4);
    View a5 = conv("model.5.conv", a4, 2, nullptr, nullptr);
    View cat11 = net_.new_view(H / 16, W / 16, c9 + c6);          // [up10, model.6]
    View s6 = cat11.slice(c9, c6);
    View a6 = c2f("model.6", a5, true, &s6);
    View a7 = conv("model.7.conv", a6, 2, nullptr, nullptr);
    View a8 = c2f("model.8", a7, true, nullptr);
    View cat26 = net_.new_view(H / 32, W / 32, c25 + c9);         // [conv25, model.9]
    View s9 = cat26.slice(c25, c9);
    sppf(a8, s9);
    // ---- head: three Upsample + Concat + C2f stages down to stride 4, then three stride-2 Conv + Concat + C2f back up ----
    const bool fuse_up = fmt == DT_F32S && c9 % 32 == 0 && c12 % 32 == 0 && c15 % 32 == 0;
    if (!fuse_up) upsample("model.10", s9, cat11.slice(0, c9));
    View cat23 = net_.new_view(H / 16, W / 16, c22 + c12);        // [conv22, model.12]
    View s12 = cat23.slice(c22, c12);
    c2f("model.12", cat11, false, &s12, fuse_up ? &s9 : nullptr);
    if (!fuse_up) upsample("model.13", s12, cat14.slice(0, c12));
    View cat20 = net_.new_view(H / 8, W / 8, c19 + c15);          // [conv19, model.15]
    View s15 = cat20.slice(c19, c15);
    c2f("model.15", cat14, false, &s15, fuse_up ? &s12 : nullptr);
    if (!fuse_up) upsample("model.16", s15, cat17.slice(0, c15));
    View a18 = c2f("model.18", cat17, false, nullptr, fuse_up ? &s15 : nullptr);
    View s19 = cat20.slice(0, c19);
    conv("model.19.conv", a18, 2, &s19, nullptr);
    View a21 = c2f("model.21", cat20, false, nullptr);
    View s22 = cat23.slice(0, c22);
    conv("model.22.conv", a21, 2, &s22, nullptr);
    View a24 = c2f("model.24", cat23, false, nullptr);
    View s25 = cat26.slice(0, c25);
    conv("model.25.conv", a24, 2, &s25, nullptr);
    View a27 = c2f("model.27", cat26, false, nullptr);
    lv.in = {a18, a21, a24, a27};
    lv.strides = {4.f, 8.f, 16.f, 32.f};
    lv.det_pfx = "model.28";
  }
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
    const bool ok = a.cfg.variant == 2 && a.cfg.ks == 3 && a.cfg.stride == 2 && pa.Cout == a.cfg.bn && !pa.res &&
                    (b.cfg.variant == 2 || b.cfg.variant == 6) && b.cfg.ks == 1 && b.cfg.kc == 32 && b.cfg.bn == pb.Cout && pb.Cin == pa.Cout && pb.Cout == pa.Cout &&
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
  const bool ok = cv.cfg.variant == 2 && cv.cfg.ks == 3 && cv.cfg.stride == 2 && cv.cfg.kc == 16 && cv.cfg.th == 8 && ((cv.cfg.bn == 32 && p.Cin == 16) || (cv.cfg.bn == 64 && p.Cin == 32)) &&
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
      launch_stem(dtype_ == DT_F32 ? fmt : dtype_, op.in.ptr, nb, op.in.h, op.in.w, op.w27, op.bias, op.wpk, op.out.c, op.out.ptr, op.out.h,
                  op.out.w, s, op.stem_scale);
      break;
    case Op::POOL: launch_sppf_pool(fmt == DT_F32S ? DT_F32S : dtype_, op.out.ptr, nb, op.in.h, op.in.w, op.in.c, s); break;
    case Op::UPSAMPLE:
      launch_upsample2x(dtype_, op.in.ptr, nb, op.in.h, op.in.w, op.in.c, op.in.cstride, op.in.coff, op.out.ptr,
                        op.out.cstride, op.out.coff, s);
      break;
    case Op::DWCONV:
      launch_rt_dwconv(fmt, RtMap{op.in.ptr, op.in.h, op.in.w, op.in.cstride, op.in.coff, op.in.c},
                       RtMap{op.out.ptr, op.out.h, op.out.w, op.out.cstride, op.out.coff, op.out.c}, nb, 3, 1, op.dw_w, op.dw_bias, op.dw_act, op.sat, s);
      break;
    case Op::ATTN:
      launch_psa_attention(fmt, RtMap{op.in.ptr, op.in.h, op.in.w, op.in.cstride, op.in.coff, op.in.c},
                           RtMap{op.out.ptr, op.out.h, op.out.w, op.out.cstride, op.out.coff, op.out.c}, nb, op.heads, op.dw_w, op.dw_bias, op.sat, s);
      break;
  }
}

void set_batch_ops(std::vector<Op>& ops, int nb, size_t es, bool pad_skip_on) {
  for (Op& op : ops) {
    if (op.kind != Op::CONV) continue;
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
  }
  for (Op& op : ops) {
    if (op.kind == Op::STEM) {
      op.flops = 2.0 * nb * op.out.h * op.out.w * op.out.c * 27;
      op.bytes = (double)nb * ((double)op.in.h * op.in.w * 4 + (double)op.out.h * op.out.w * op.out.c * es);   // RGB0 bytes in
    } else if (op.kind == Op::POOL) {
      op.flops = 0;
      op.bytes = (double)nb * op.in.h * op.in.w * op.in.c * 4 * es;
    } else if (op.kind == Op::UPSAMPLE) {
      op.flops = 0;
      op.bytes = (double)nb * op.in.h * op.in.w * op.in.c * 5 * es;
    } else if (op.kind == Op::DWCONV) {
      op.flops = 2.0 * 9 * nb * op.in.h * op.in.w * op.in.c;
      op.bytes = 2.0 * nb * op.in.h * op.in.w * op.in.c * es;
    } else if (op.kind == Op::ATTN) {               // q.k (depth 32) + p.v (width 64) per query-key pair and head, + pe; the qkv map in, the output map out
      const double T = (double)op.in.h * op.in.w;
      op.flops = nb * (op.heads * T * T * 2.0 * (32 + 64) + 2.0 * 9 * T * op.out.c);
      op.bytes = nb * T * (op.in.c + op.out.c) * es;
    }
  }
}

}  // namespace gtx
