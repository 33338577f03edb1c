// The operator hooks of libgtx.so's C ABI (gtx_op_*, include/gtx.h): one launcher, or one host routine, at a time on host arrays.
// The float64 tests drive them, and the package calls a few itself (the registration matcher, the georeference chain, CLAHE).
// A hook checks every size, and every index a kernel would turn into an address, before it touches the GPU; then it stages its
// arrays with op_staging.hpp, launches as the product launches, and copies the results back. The hooks of file-local kernels
// (op_gmc_* in gmc.hip, op_ecc_* in ecc.hip, op_orb_match in stabilizer.hip, op_orb_ransac in homography.hip, op_sift_* in sift.hip) keep their staging beside the kernels and have only their checks here.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gtx.h"
#include "api_guard.hpp"
#include "area_attn.hpp"
#include "clahe.hpp"
#include "common.hpp"
#include "conv_igemm.hpp"
#include "det_kernels.hpp"
#include "detector.hpp"
#include "draw.hpp"
#include "ecc.hpp"
#include "geometry.hpp"
#include "gmc.hpp"
#include "homography.hpp"
#include "jpeg_enc.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_restart.hpp"
#include "match_l2.hpp"
#include "op_staging.hpp"
#include "pool_down.hpp"
#include "register.hpp"
#include "rtdetr_kernels.hpp"
#include "sift.hpp"
#include "stabilizer.hpp"
#include "stem6.hpp"
#include "tracker.hpp"

namespace {
using gtx::download;
using gtx::download_fmt;
using gtx::fill_ff;
using gtx::guarded;
using gtx::need;
using gtx::op_bad;
using gtx::time_launches;
using gtx::upload;
using gtx::upload_fmt;
using gtx::zeros;
}  // namespace

extern "C" {

// ---- the convolution launcher and the detector's small map kernels (tests/test_ops_gpu.py, tests/test_conv_k32s2_gpu.py; the dwconv and
// PSA hooks: tests/test_yolov10_gpu.py, tests/test_reid_yolo11_gpu.py)

namespace {
struct ConvOpState {
  gtx::DevBuf x, w, b, r, y;
  gtx::ConvGroup g{};
  gtx::ConvConfig cfg{};
  int ho = 0, wo = 0;
};

// force_kc > 0 pins the K chunk (conv_pick_config); y_plain: the output buffer is plain fp32 whatever d->dtype (ConvProblem::out_plain).
// res_cstride > 0: the residual array has that many channels per pixel and the launch adds the slice at res_coff (0: [..][cout]).
// in_place: y_init is the one array behind input, residual and output; it is uploaded once and all three pointers are that buffer
// (gtx_op_conv2d_fused has checked the slices).
void conv_setup(gtx_ctx* ctx, const gtx_conv_desc* d, const void* x, const float* w, const float* bias,
                const void* residual, const void* y_init, ConvOpState& st, int force_kc = 0, bool y_plain = false,
                int res_cstride = 0, int res_coff = 0, bool in_place = false) {
  using namespace gtx;
  need(ctx, "ctx"); need(d, "desc");
  GTX_HIP(hipSetDevice(ctx->device));
  if (d->dtype != GTX_F16 && d->dtype != GTX_F32 && d->dtype != GTX_F32S) fail(GTX_ERR_INVALID, "bad dtype %d", d->dtype);
  const size_t es = dtype_size(d->dtype);
  const int pad = d->ksize / 2;
  st.ho = (d->h + 2 * pad - d->ksize) / d->stride + 1;
  st.wo = (d->w + 2 * pad - d->ksize) / d->stride + 1;
  st.cfg = conv_pick_config(d->dtype, d->ksize, d->stride, d->cin, d->cout, force_kc);
  const bool pairs = d->dtype == GTX_F32S;       // host arrays are plain fp32; the device buffers hold the pair format (split_format.hpp)
  const int vn = pairs ? 8 : 16 / (int)es;
  GTX_CHECK(d->in_cstride % vn == 0 && d->in_coff % vn == 0 && d->out_cstride % (pairs ? 8 : 4) == 0 && d->out_coff % (pairs ? 8 : 4) == 0 &&
                (!pairs || d->cout % 8 == 0),
            "conv: channel strides/offsets must keep 16-byte (input) / 4-element (output) alignment, whole 8-channel groups for the split-f16x3 path");
  GTX_CHECK(d->in_coff + d->cin <= d->in_cstride && d->out_coff + d->cout <= d->out_cstride, "conv: slice outside buffer");
  const size_t xin = (size_t)d->n * d->h * d->w * d->in_cstride * es;
  const size_t yout = (size_t)d->n * st.ho * st.wo * d->out_cstride * es;
  // timing calls (no data handed in) run on pseudo-random activations and weights: zeros would flatter the matrix pipe
  // (no operand toggling, no power throttling) -- the layer sweeps of rounds 1 and 2 up to this change were taken on zeros
  unsigned long long lcg = 0x2545F4914F6CDD1Dull;
  const bool all_zero = std::getenv("GTX_TIME_ZEROS") != nullptr;   // the old behaviour, to show the difference
  auto uni = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return all_zero ? 0.f : (float)((lcg >> 40) * (1.0 / 8388608.0) - 1.0); };
  if (in_place) {
    need(y_init, "y");                               // st.x stays empty: `in` is the output buffer
  } else if (x) {
    upload_fmt(st.x, d->dtype, x, xin);
  } else if (es == 2) {
    std::vector<_Float16> hx(xin / 2);
    for (auto& v : hx) v = (_Float16)uni();
    upload(st.x, hx.data(), xin);
  } else {
    std::vector<float> hx(xin / 4);
    for (auto& v : hx) v = uni();
    upload_fmt(st.x, d->dtype, hx.data(), xin);
  }
  if (y_init) upload_fmt(st.y, y_plain ? GTX_F32 : d->dtype, y_init, yout);
  else st.y.alloc(yout);
  std::vector<uint8_t> packed;
  float acc_scale = 1.f;
  if (w) {
    packed = pack_conv_weights(w, d->cout, d->cin, st.cfg, &acc_scale);
  } else {
    std::vector<float> hw((size_t)d->cout * d->cin * d->ksize * d->ksize);
    const float sc = 1.f / std::sqrt((float)(d->cin * d->ksize * d->ksize));
    for (auto& v : hw) v = uni() * sc;
    packed = pack_conv_weights(hw.data(), d->cout, d->cin, st.cfg, &acc_scale);
  }
  upload(st.w, packed.data(), packed.size());
  if (bias) {
    const size_t padded = (size_t)(d->cout + 63) / 64 * 64 * sizeof(float);      // whole cout tiles: the kernels load a tile's bias unconditionally
    zeros(st.b, padded);
    GTX_HIP(hipMemcpy(st.b.p, bias, d->cout * sizeof(float), hipMemcpyHostToDevice));
  }
  const int rcs = res_cstride > 0 ? res_cstride : d->cout;
  if (d->has_residual && !in_place) {
    const size_t rb = (size_t)d->n * st.ho * st.wo * rcs * es;
    if (residual) upload_fmt(st.r, d->dtype, residual, rb);
    else zeros(st.r, rb);
  }
  ConvProblem& p = st.g.p[0];
  p.in = in_place ? st.y.p : st.x.p; p.out = st.y.p; p.wpack = st.w.p;
  p.bias = bias ? st.b.as<float>() : nullptr;
  p.res = d->has_residual ? (in_place ? st.y.p : st.r.p) : nullptr;
  p.N = d->n; p.H = d->h; p.W = d->w; p.Ho = st.ho; p.Wo = st.wo; p.Cin = d->cin; p.Cout = d->cout;
  p.in_cstride = d->in_cstride; p.in_coff = d->in_coff;
  p.out_cstride = d->out_cstride; p.out_coff = d->out_coff;
  p.res_cstride = rcs; p.res_coff = res_cstride > 0 ? res_coff : 0;
  p.act = d->act;
  p.acc_scale = acc_scale;
  p.in2 = nullptr; p.in2_cstride = p.in2_coff = p.c_split = 0;
  p.out_plain = 0; p.sat_flag = nullptr;
  p.post_w = nullptr; p.post_bias = nullptr; p.post_scale = 1.f; p.post_act = 0;
  st.g.count = 1;
  conv_group_finalize(st.g, st.cfg);
}
}  // namespace

int gtx_op_conv2d(gtx_ctx* ctx, const gtx_conv_desc* d, const void* x, const float* w_ohwi, const float* bias,
                  const void* residual, void* y) {
  return guarded([&] {
    need(x, "x"); need(w_ohwi, "w"); need(y, "y");
    if (d && d->has_residual) need(residual, "residual");
    ConvOpState st;
    conv_setup(ctx, d, x, w_ohwi, bias, residual, y, st);
    gtx::conv_launch(st.g, st.cfg, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    const size_t yb = (size_t)d->n * st.ho * st.wo * d->out_cstride * gtx::dtype_size(d->dtype);
    download_fmt(y, d->dtype, st.y, yb);
  });
}

int gtx_op_conv2d_group(gtx_ctx* ctx, int n_members, const gtx_conv_desc* descs, const void* const* xs, const float* const* ws,
                        const float* const* biases, void* const* ys, const int* ty_first, const int* ty_count) {
  return guarded([&] {
    need(descs, "descs"); need(xs, "xs"); need(ws, "ws"); need(ys, "ys");
    if (n_members < 1 || n_members > gtx::kMaxGroup) gtx::fail(GTX_ERR_INVALID, "1..%d members", gtx::kMaxGroup);
    std::vector<ConvOpState> st(n_members);
    gtx::ConvGroup g{};
    for (int i = 0; i < n_members; ++i) {
      need(xs[i], "x"); need(ws[i], "w"); need(ys[i], "y");
      if (descs[i].has_residual) gtx::fail(GTX_ERR_INVALID, "grouped op: no residual");
      conv_setup(ctx, &descs[i], xs[i], ws[i], biases ? biases[i] : nullptr, nullptr, ys[i], st[i]);
      if (!gtx::same_kernel(st[0].cfg, st[i].cfg))
        gtx::fail(GTX_ERR_INVALID, "grouped op: member %d picks another kernel than member 0", i);
      g.p[i] = st[i].g.p[0];
      g.p[i].ty_first = ty_first ? ty_first[i] : 0;
      g.p[i].ty_count = ty_count ? ty_count[i] : 0;
    }
    g.count = n_members;
    gtx::conv_group_finalize(g, st[0].cfg);
    gtx::conv_launch(g, st[0].cfg, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n_members; ++i) {
      const size_t yb = (size_t)descs[i].n * st[i].ho * st[i].wo * descs[i].out_cstride * gtx::dtype_size(descs[i].dtype);
      download_fmt(ys[i], descs[i].dtype, st[i].y, yb);
    }
  });
}

int gtx_op_conv_xcd_ranges(int n_members, const int* blocks, const int* cin, int xcd_begin[9], int* grid_blocks) {
  return guarded([&] {
    need(blocks, "blocks"); need(cin, "cin"); need(xcd_begin, "xcd_begin");
    if (n_members < 1 || n_members > gtx::kMaxGroup) gtx::fail(GTX_ERR_INVALID, "1..%d members", gtx::kMaxGroup);
    gtx::ConvGroup g{};
    gtx::ConvConfig c{};
    c.bn = 64; c.th = 8; c.tw = 16;                       // one workgroup per (8 x 16 pixel tile, 64-cout tile): blocks[i] = tiles_y
    g.count = n_members;
    for (int i = 0; i < n_members; ++i) {
      if (blocks[i] < 1 || cin[i] < 1) gtx::fail(GTX_ERR_INVALID, "member %d: blocks and cin must be positive", i);
      gtx::ConvProblem& p = g.p[i];
      p.N = 1; p.Wo = 16; p.Ho = 8 * blocks[i]; p.Cout = 64; p.Cin = cin[i];
    }
    gtx::conv_group_finalize(g, c);
    for (int k = 0; k < 9; ++k) xcd_begin[k] = g.xcd_begin[k];
    if (grid_blocks) *grid_blocks = g.grid_blocks;
  });
}

int gtx_op_conv_config(int dtype, int ksize, int stride, int cin, int cout, int force_kc, int* form, int* bn, int* kc, char* name, int name_cap) {
  return guarded([&] {
    need(form, "form"); need(bn, "bn"); need(kc, "kc");
    if (dtype != GTX_F16 && dtype != GTX_F32 && dtype != GTX_F32S) op_bad("conv_config", "dtype: GTX_F16, GTX_F32 or GTX_F32S");
    if (cin < 1 || cout < 1 || force_kc < 0 || (name && name_cap < 1)) op_bad("conv_config", "cin, cout and name_cap must be positive, force_kc not negative");
    const gtx::ConvConfig c = gtx::conv_pick_config(dtype, ksize, stride, cin, cout, force_kc);
    *form = (int)c.variant; *bn = c.bn; *kc = c.kc;
    if (name) std::snprintf(name, (size_t)name_cap, "%s", gtx::conv_kernel_name(c));
  });
}

int gtx_op_conv2d_time(gtx_ctx* ctx, const gtx_conv_desc* d, int iters, float* ms_per_launch, double* flops) {
  return guarded([&] {
    need(ms_per_launch, "ms_per_launch");
    if (iters < 1) gtx::fail(GTX_ERR_INVALID, "iters must be >= 1");
    ConvOpState st;
    conv_setup(ctx, d, nullptr, nullptr, nullptr, nullptr, nullptr, st);
    *ms_per_launch = time_launches(ctx->stream, iters, [&] { gtx::conv_launch(st.g, st.cfg, ctx->stream); });
    if (flops) *flops = gtx::conv_flops(st.g.p[0], d->ksize);
  });
}

// One launch with the stages and sources gtx_op_conv2d leaves off (tests/test_front_ops_gpu.py). The staging is conv_setup's; what
// the extras ask of the kernel is checked by the launchers themselves (conv_launch, conv_split_launch and the other forms'),
// which refuse before anything is launched -- only what a launcher cannot know, the size of a host array, is checked here.
int gtx_op_conv2d_fused(gtx_ctx* ctx, const gtx_conv_desc* d, const gtx_conv_fused* f, const void* x, const float* w_ohwi, const float* bias,
                        const void* residual, void* y) {
  return guarded([&] {
    need(d, "desc"); need(f, "fused"); need(w_ohwi, "w"); need(y, "y");
    if (!f->front_img) need(x, "x");                  // a front stage computes its input: `in` is not read
    if (d->has_residual) need(residual, "residual");
    const bool pairs = d->dtype == GTX_F32S;
    if (f->x2) {
      if (f->c_split < 1 || f->in2_coff < 0 || (long)f->in2_coff + f->c_split > f->in2_cstride || (pairs && (f->in2_cstride % 8 || f->in2_coff % 8)))
        op_bad("conv2d_fused", "the second source's channel slice does not fit its stride (whole 8-channel groups on the split-f16x3 path)");
      if (d->n < 1 || d->h < 2 || d->w < 2) op_bad("conv2d_fused", "a second source needs a map of at least 2 x 2");
    }
    if (f->post_w && (d->cout < 1 || d->cout > 1024)) op_bad("conv2d_fused", "bad Cout");
    if (f->front_img) {
      need(f->front_w27, "front_w27"); need(f->front_bias, "front_bias");
      if (d->n < 1 || f->front_h < 1 || f->front_w_px < 1 || d->cin < 1 || d->cin > 1024) op_bad("conv2d_fused", "front stage: bad sizes");
    }
    if (f->force_kc < 0 || f->members < 0 || f->members > gtx::kMaxGroup) op_bad("conv2d_fused", "bad force_kc / members");
    // a residual slice as the kernels address it: 4 elements per load (whole 8-channel groups in the pair format), inside its stride
    const int rvn = pairs ? 8 : 4;
    if (f->res_cstride < 0 || f->res_coff < 0 || (f->res_cstride == 0 && f->res_coff != 0) || (f->res_cstride > 0 && !d->has_residual))
      op_bad("conv2d_fused", "residual slice: res_cstride / res_coff must not be negative and need a residual");
    if (f->res_cstride > 0 && (d->cout < 1 || (long)f->res_coff + d->cout > f->res_cstride || f->res_cstride % rvn || f->res_coff % rvn))
      op_bad("conv2d_fused", "the residual's channel slice does not fit its stride (4-element alignment, whole 8-channel groups on the split-f16x3 path)");
    if (f->in_place) {
      if (f->in_place != 1 || d->stride != 1 || (d->ksize != 1 && d->ksize != 3) || f->x2 || f->front_img || f->post_w || f->out_plain)
        op_bad("conv2d_fused", "in_place: a plain stride-1 launch (no second source, fused stage or plain output)");
      if (x != y || (d->has_residual && residual != y)) op_bad("conv2d_fused", "in_place: x, residual and y must be the same array");
      if (d->cin < 1 || d->cout < 1 || d->in_coff < 0 || d->out_coff < 0 || d->in_cstride != d->out_cstride ||
          (d->has_residual && f->res_cstride != d->out_cstride))
        op_bad("conv2d_fused", "in_place: input, residual and output share one channel stride");
      const auto meets = [&](long a, long na) { return a < (long)d->out_coff + d->cout && (long)d->out_coff < a + na; };
      if (meets(d->in_coff, d->cin) || (d->has_residual && meets(f->res_coff, d->cout)))
        op_bad("conv2d_fused", "in_place: the input and residual channels must not overlap the output's");
    }
    // the fused stages belong to the 32x32x16 kernel and its 16-channel chunks (yolo_trunk.cpp: YoloTrunk::conv)
    const int force_kc = f->force_kc > 0 ? f->force_kc : ((f->post_w || f->front_img) ? 16 : 0);
    const bool plain = f->out_plain != 0;
    ConvOpState st;
    conv_setup(ctx, d, x, w_ohwi, bias, residual, y, st, force_kc, plain, f->res_cstride, f->res_coff, f->in_place != 0);
    gtx::ConvProblem& p = st.g.p[0];
    gtx::DevBuf x2, sat, pw, pb, fimg, fw, fb, mid;
    gtx::ConvGroup g2{};                                // post_separate: the 1x1 layer as a launch of its own
    gtx::ConvConfig c2{};
    if (f->x2) {
      upload_fmt(x2, d->dtype, f->x2, (size_t)d->n * (d->h / 2) * (d->w / 2) * f->in2_cstride * gtx::dtype_size(d->dtype));
      p.in2 = x2.p; p.in2_cstride = f->in2_cstride; p.in2_coff = f->in2_coff; p.c_split = f->c_split;
    }
    p.out_plain = plain ? 1 : 0;
    if (f->sat) {
      zeros(sat, 4);
      p.sat_flag = sat.as<int>();
    }
    if (f->post_w) {                                    // as fuse_front() finds model.2.cv1: the 1x1 layer's own packed image, 32-channel chunks
      c2 = gtx::conv_pick_config(d->dtype, 1, 1, d->cout, d->cout, 32);
      float sc = 1.f;
      const std::vector<uint8_t> img = gtx::pack_conv_weights(f->post_w, d->cout, d->cout, c2, &sc);
      upload(pw, img.data(), img.size());
      p.post_w = pw.p; p.post_scale = sc; p.post_act = f->post_act;
      if (f->post_bias) {
        zeros(pb, (size_t)(d->cout + 63) / 64 * 64 * sizeof(float));
        GTX_HIP(hipMemcpy(pb.p, f->post_bias, d->cout * sizeof(float), hipMemcpyHostToDevice));
        p.post_bias = pb.as<float>();
      }
    }
    if (f->front_img) {                                 // as YoloTrunk::stem() keeps them for fuse_stem()
      upload(fimg, f->front_img, (size_t)d->n * f->front_h * f->front_w_px * 4);
      float sc = 1.f;
      const std::vector<uint16_t> img = gtx::pack_front_weights_split(f->front_w27, d->cin, &sc);
      upload(fw, img.data(), img.size() * 2);
      zeros(fb, (size_t)(d->cin + 31) / 32 * 32 * sizeof(float));
      GTX_HIP(hipMemcpy(fb.p, f->front_bias, d->cin * sizeof(float), hipMemcpyHostToDevice));
      p.front_img = fimg.p; p.front_w = fw.p; p.front_bias = fb.as<float>(); p.front_scale = sc;
      p.front_h = f->front_h; p.front_w_px = f->front_w_px;
    }
    if (f->post_w && f->post_separate) {
      // What the post stage replaces, as the detector runs it with GTX_FUSE_FRONT=0: the 3x3 launch writes its pair-format output to
      // HBM and the 1x1 layer reads it there. (Two hook calls would take the map through the host instead, and hi + lo split again
      // is not always the same two halves: a tie in fp16(hi + lo) may go the other way.)
      if (f->ty_count || f->members > 1 || d->dtype != GTX_F32S) op_bad("conv2d_fused", "post_separate: one whole split-f16x3 launch");
      zeros(mid, (size_t)d->n * st.ho * st.wo * d->cout * 4);
      // q is filled field by field: a member added to ConvProblem that a stand-alone 1x1 launch needs has to be set here too
      // (conv_setup fills the first launch's; g2{} leaves everything else of q zero = off)
      gtx::ConvProblem& q = g2.p[0];
      q.in = mid.p; q.out = p.out; q.wpack = p.post_w; q.bias = p.post_bias;
      q.N = d->n; q.H = q.Ho = st.ho; q.W = q.Wo = st.wo; q.Cin = q.Cout = d->cout;
      q.in_cstride = d->cout; q.out_cstride = p.out_cstride; q.out_coff = p.out_coff; q.res_cstride = d->cout;
      q.act = p.post_act; q.acc_scale = p.post_scale; q.post_scale = 1.f; q.out_plain = p.out_plain; q.sat_flag = p.sat_flag;
      p.out = mid.p; p.out_cstride = d->cout; p.out_coff = 0; p.out_plain = 0;
      p.post_w = nullptr; p.post_bias = nullptr; p.post_scale = 1.f; p.post_act = 0;
      g2.count = 1;
      gtx::conv_group_finalize(g2, c2);
    }
    p.ty_first = f->ty_first; p.ty_count = f->ty_count;
    for (int i = 1; i < f->members; ++i) st.g.p[i] = p;   // the same problem again: only to meet a launcher's rule on group size
    st.g.count = f->members > 1 ? f->members : 1;
    gtx::conv_group_finalize(st.g, st.cfg);
    gtx::conv_launch(st.g, st.cfg, ctx->stream);
    if (g2.count) gtx::conv_launch(g2, c2, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    const size_t yb = (size_t)d->n * st.ho * st.wo * d->out_cstride * gtx::dtype_size(d->dtype);
    download_fmt(y, plain ? GTX_F32 : d->dtype, st.y, yb);
    if (f->sat) download(f->sat, sat, 4);
  });
}

// The stem (model.0: 3x3 stride 2 on RGB0 bytes + bias + SiLU) as launch_stem runs it for the detector and the ReID crops
// (tests/test_front_ops_gpu.py). packed = 0 with GTX_F16: the VALU kernel; GTX_F32 is always that kernel, GTX_F32S always packed.
int gtx_op_stem(gtx_ctx* ctx, int dtype, int packed, int n, int h, int w, int c0, const void* img, const float* w27, const float* bias,
                void* out) {
  return guarded([&] {
    if (dtype != GTX_F16 && dtype != GTX_F32 && dtype != GTX_F32S) op_bad("stem", "dtype: GTX_F16, GTX_F32 or GTX_F32S");
    if (c0 < 16 || c0 > 96 || c0 % 16) op_bad("stem", "c0 must be 16, 32, 48, 64, 80 or 96");
    if (n < 1 || h < 1 || w < 1 || (double)n * h * w > 1e9) op_bad("stem", "n, h and w must be at least 1");
    need(ctx, "ctx"); need(img, "img"); need(w27, "w27"); need(bias, "bias"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const size_t ob = (size_t)n * ho * wo * c0 * gtx::dtype_size(dtype);
    gtx::DevBuf dimg, dw, db, dpk, dout;
    upload(dimg, img, (size_t)n * h * w * 4);
    upload(dw, w27, (size_t)27 * c0 * 4);
    zeros(db, (size_t)(c0 + 31) / 32 * 32 * sizeof(float));      // whole 32-channel groups: the MFMA stems read a group's bias unconditionally
    GTX_HIP(hipMemcpy(db.p, bias, c0 * sizeof(float), hipMemcpyHostToDevice));
    zeros(dout, ob);
    float sc = 1.f;
    if (dtype == GTX_F32S) {
      const std::vector<uint16_t> pk = gtx::pack_stem_weights_split(w27, c0, &sc);
      upload(dpk, pk.data(), pk.size() * 2);
    } else if (dtype == GTX_F16 && packed) {
      const std::vector<uint16_t> pk = gtx::pack_stem_weights_f16(w27, c0);
      upload(dpk, pk.data(), pk.size() * 2);
    }
    gtx::launch_stem(dtype, dimg.p, n, h, w, dw.as<float>(), db.as<float>(), dpk.p, c0, dout.p, ho, wo, ctx->stream, sc);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dout, ob);
  });
}

// yolov5.yaml's stem (model.0: 6x6 stride 2 pad 2 on RGB0 bytes + bias + SiLU) as launch_stem6 runs it for the detector
// (tests/test_yolov5u_gpu.py). GTX_F16 and GTX_F32S: the matrix-core kernels on their packed weights; GTX_F32: the exact kernel.
// iters > 0: *ms_per_launch = mean time of that many further launches.
int gtx_op_stem6(gtx_ctx* ctx, int dtype, int n, int h, int w, int c0, const void* img, const float* w108, const float* bias, void* out,
                 int iters, float* ms_per_launch) {
  return guarded([&] {
    if (dtype != GTX_F16 && dtype != GTX_F32 && dtype != GTX_F32S) op_bad("stem6", "dtype: GTX_F16, GTX_F32 or GTX_F32S");
    if (c0 < 16 || c0 > 96 || c0 % 16) op_bad("stem6", "c0 must be 16, 32, 48, 64, 80 or 96");
    if (n < 1 || h < 2 || w < 2 || (double)n * h * w > 1e9) op_bad("stem6", "n must be at least 1, h and w at least 2");
    need(ctx, "ctx"); need(img, "img"); need(w108, "w108"); need(bias, "bias"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    const int ho = gtx::stem6_out(h), wo = gtx::stem6_out(w);
    const size_t ob = (size_t)n * ho * wo * c0 * gtx::dtype_size(dtype);
    gtx::DevBuf dimg, dw, db, dpk, dout;
    upload(dimg, img, (size_t)n * h * w * 4);
    upload(dw, w108, (size_t)108 * c0 * 4);
    zeros(db, (size_t)(c0 + 31) / 32 * 32 * sizeof(float));      // whole 32-channel groups: the matrix-core kernels read a group's bias unconditionally
    GTX_HIP(hipMemcpy(db.p, bias, c0 * sizeof(float), hipMemcpyHostToDevice));
    zeros(dout, ob);
    float sc = 1.f;
    if (dtype != GTX_F32) {
      const std::vector<uint16_t> pk = dtype == GTX_F32S ? gtx::pack_stem6_weights_split(w108, c0, &sc) : gtx::pack_stem6_weights_f16(w108, c0);
      upload(dpk, pk.data(), pk.size() * 2);
    }
    auto once = [&] { gtx::launch_stem6(dtype, dimg.p, n, h, w, dw.as<float>(), db.as<float>(), dpk.p, c0, dout.p, ho, wo, ctx->stream, sc); };
    once();
    if (iters > 0 && ms_per_launch) *ms_per_launch = time_launches(ctx->stream, iters, once);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dout, ob);
  });
}

int gtx_op_sppf_pool(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, void* x_inout) {
  return guarded([&] {
    need(ctx, "ctx"); need(x_inout, "x");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * h * w * 4 * c * gtx::dtype_size(dtype);
    gtx::DevBuf d;
    upload_fmt(d, dtype, x_inout, bytes);
    gtx::launch_sppf_pool(dtype, d.p, n, h, w, c, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(x_inout, dtype, d, bytes);
  });
}

int gtx_op_upsample2x(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, const void* x, int in_cstride,
                      int in_coff, void* y, int out_cstride, int out_coff) {
  return guarded([&] {
    need(ctx, "ctx"); need(x, "x"); need(y, "y");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t es = gtx::dtype_size(dtype);
    const size_t xb = (size_t)n * h * w * in_cstride * es, yb = (size_t)n * 4 * h * w * out_cstride * es;
    gtx::DevBuf dx, dy;
    upload(dx, x, xb); upload(dy, y, yb);
    gtx::launch_upsample2x(es, dx.p, n, h, w, c, in_cstride, in_coff, dy.p, out_cstride, out_coff, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(y, dy, yb);
  });
}

int gtx_op_psa_attention(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int heads, const void* qkv, int in_cstride, int in_coff,
                         const float* pe_w, const float* pe_b, void* out, int out_cstride, int out_coff, int form, int iters, float* ms_per_launch,
                         int* saturated) {
  return guarded([&] {
    need(ctx, "ctx"); need(qkv, "qkv"); need(pe_w, "pe_w"); need(pe_b, "pe_b"); need(out, "out");
    if (n < 1 || n_alloc < n || h < 1 || w < 1 || heads < 1 || iters < 0) gtx::fail(GTX_ERR_INVALID, "psa_attention: bad sizes");
    if (in_coff < 0 || in_coff + heads * 128 > in_cstride || out_coff < 0 || out_coff + heads * 64 > out_cstride)
      gtx::fail(GTX_ERR_INVALID, "psa_attention: the channel slices do not fit their strides");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t es = gtx::dtype_size(dtype), C = (size_t)heads * 64;
    const size_t xb = (size_t)n_alloc * h * w * in_cstride * es, yb = (size_t)n * h * w * out_cstride * es;
    gtx::DevBuf dx, dy, dw, db, ds;
    upload_fmt(dx, dtype, qkv, xb); upload_fmt(dy, dtype, out, yb);
    upload(dw, pe_w, 9 * C * 4); upload(db, pe_b, C * 4);
    zeros(ds, 4);
    const gtx::RtMap in{dx.p, h, w, in_cstride, in_coff, heads * 128}, o{dy.p, h, w, out_cstride, out_coff, heads * 64};
    auto once = [&] { gtx::launch_psa_attention(dtype, in, o, n, heads, dw.as<float>(), db.as<float>(), ds.as<int>(), ctx->stream, form); };
    once();
    if (iters > 0 && ms_per_launch) *ms_per_launch = time_launches(ctx->stream, iters, once);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dy, yb);
    if (saturated) download(saturated, ds, 4);
  });
}

int gtx_op_area_attention(gtx_ctx* ctx, int dtype, int n, int h, int w, int heads, int area, int planar, const void* qkv, int in_cstride, int in_coff,
                          void* out, int out_cstride, int out_coff, int iters, float* ms_per_launch, int* saturated) {
  return guarded([&] {
    need(ctx, "ctx"); need(qkv, "qkv"); need(out, "out");
    if (n < 1 || h < 1 || w < 1 || heads < 1 || area < 1 || iters < 0) gtx::fail(GTX_ERR_INVALID, "area_attention: bad sizes");
    if (in_coff < 0 || in_coff + heads * 96 > in_cstride || out_coff < 0 || out_coff + heads * 32 > out_cstride)
      gtx::fail(GTX_ERR_INVALID, "area_attention: the channel slices do not fit their strides");
    if (!gtx::area_attention_fits(h, w, area))
      gtx::fail(GTX_ERR_UNSUPPORTED, "area_attention: a %d x %d map (%d positions) does not cut into %d equal areas", w, h, h * w, area);
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t es = gtx::dtype_size(dtype);
    const size_t xb = (size_t)n * h * w * in_cstride * es, yb = (size_t)n * h * w * out_cstride * es;
    gtx::DevBuf dx, dy, ds;
    upload_fmt(dx, dtype, qkv, xb); upload_fmt(dy, dtype, out, yb);
    zeros(ds, 4);
    const gtx::RtMap in{dx.p, h, w, in_cstride, in_coff, heads * 96}, o{dy.p, h, w, out_cstride, out_coff, heads * 32};
    auto once = [&] { gtx::launch_area_attention(dtype, in, o, n, heads, area, planar != 0, ds.as<int>(), ctx->stream); };
    once();
    if (iters > 0 && ms_per_launch) *ms_per_launch = time_launches(ctx->stream, iters, once);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dy, yb);
    if (saturated) download(saturated, ds, 4);
  });
}

int gtx_op_dwconv(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, int k, int stride, const void* x, const float* wt, const float* bias,
                  int act, const void* res, void* out, int* saturated) {
  return guarded([&] {
    need(ctx, "ctx"); need(x, "x"); need(wt, "w"); need(bias, "bias"); need(out, "out");
    if (n < 1 || h < 1 || w < 1 || c < 8 || c % 8 || (k != 3 && k != 5 && k != 7) || (stride != 1 && stride != 2)) gtx::fail(GTX_ERR_INVALID, "dwconv: bad sizes");
    GTX_HIP(hipSetDevice(ctx->device));
    const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
    const size_t es = gtx::dtype_size(dtype);
    const size_t xb = (size_t)n * h * w * c * es, yb = (size_t)n * ho * wo * c * es, wb = (size_t)k * k * c * 4;
    gtx::DevBuf dx, dy, dr, dw, db, ds;
    upload_fmt(dx, dtype, x, xb);
    if (res) upload_fmt(dr, dtype, res, yb);
    upload(dw, wt, wb); upload(db, bias, (size_t)c * 4);
    zeros(ds, 4); zeros(dy, yb);
    const gtx::RtMap in{dx.p, h, w, c, 0, c}, o{dy.p, ho, wo, c, 0, c}, r{dr.p, ho, wo, c, 0, c};
    gtx::launch_rt_dwconv(dtype, in, o, n, k, stride, dw.as<float>(), db.as<float>(), act, ds.as<int>(), ctx->stream, res ? &r : nullptr);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dy, yb);
    if (saturated) download(saturated, ds, 4);
  });
}

int gtx_op_pool_down(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c_avg, int c_max, const void* x, int in_cstride, int in_coff,
                     void* avg, int avg_cstride, int avg_coff, void* mx, int max_cstride, int max_coff, int iters, float* ms_per_launch) {
  return guarded([&] {
    // every size first: a kernel turns them into addresses
    if (n_alloc < n || iters < 0) op_bad("pool_down", "bad sizes");
    if (c_avg % 8 || c_max % 8 || c_avg < 8 || c_max < 0) op_bad("pool_down", "channel counts must be multiples of 8 (c_avg > 0)");
    char stub = 0;                                      // the shape check wants non-null buffers; none is touched
    const gtx::RtMap in0{&stub, h, w, in_cstride, in_coff, c_avg + c_max}, avg0{&stub, h, w, avg_cstride, avg_coff, c_avg},
        mx0{c_max ? &stub : nullptr, h / 2, w / 2, c_max ? max_cstride : 0, c_max ? max_coff : 0, c_max};
    if (const char* why = gtx::pool_down_refusal(dtype, in0, avg0, mx0, n)) op_bad("pool_down", why);
    need(x, "x"); need(avg, "avg");
    if (c_max) need(mx, "max");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t es = gtx::dtype_size(dtype);
    const size_t xb = (size_t)n_alloc * h * w * in_cstride * es, ab = (size_t)n_alloc * h * w * avg_cstride * es,
                 mb = c_max ? (size_t)n_alloc * (h / 2) * (w / 2) * max_cstride * es : 0;
    gtx::DevBuf dx, da, dm;
    upload_fmt(dx, dtype, x, xb); upload_fmt(da, dtype, avg, ab);
    if (c_max) upload_fmt(dm, dtype, mx, mb);
    const gtx::RtMap in{dx.p, h, w, in_cstride, in_coff, c_avg + c_max}, a{da.p, h, w, avg_cstride, avg_coff, c_avg},
        m{c_max ? dm.p : nullptr, h / 2, w / 2, c_max ? max_cstride : 0, c_max ? max_coff : 0, c_max};
    auto once = [&] { gtx::launch_pool_down(dtype, in, a, m, n, ctx->stream); };
    once();
    if (iters > 0 && ms_per_launch) *ms_per_launch = time_launches(ctx->stream, iters, once);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(avg, dtype, da, ab);
    if (c_max) download_fmt(mx, dtype, dm, mb);
  });
}

// ---- RT-DETR's token-side kernels, one hook per launcher (tests/test_rtdetr_ops_gpu.py). Every size is checked here, before
// anything touches the GPU: whatever a launcher's own GTX_CHECK would refuse, and whatever would let a kernel read or write
// outside the arrays it is given.
namespace {
// Up to three levels of NHWC maps [n][h][w][cstride] with `c` channels read from coff
struct RtLevelSet {
  gtx::RtLevels L{};
  gtx::DevBuf buf[3];
  int S = 0;
};
void rt_levels_check(const char* op, int fmt, int n, int n_levels, const void* const* maps, const int* h, const int* w, const int* cstride,
                     const int* coff, int c, bool allow_split) {
  need(maps, "maps"); need(h, "h"); need(w, "w"); need(cstride, "cstride"); need(coff, "coff");
  if (!(fmt == GTX_F16 || fmt == GTX_F32 || (allow_split && fmt == GTX_F32S))) op_bad(op, "unsupported map format");
  if (n < 1 || n_levels < 1 || n_levels > 3 || c < 1) op_bad(op, "bad sizes");
  long S = 0;
  for (int l = 0; l < n_levels; ++l) {
    need(maps[l], "maps[l]");
    if (h[l] < 1 || w[l] < 1 || coff[l] < 0 || (long)coff[l] + c > cstride[l]) op_bad(op, "a level's channel slice does not fit its stride");
    if (fmt == GTX_F32S && (cstride[l] % 8 || coff[l] % 8)) op_bad(op, "pair-format maps need channel strides and offsets that are multiples of 8");
    S += (long)h[l] * w[l];
    if (S > (1l << 24) || (double)n * h[l] * w[l] * cstride[l] > 1e9) op_bad(op, "maps too large");
  }
}
void rt_levels_upload(RtLevelSet& s, int fmt, int n, int n_levels, const void* const* maps, const int* h, const int* w, const int* cstride,
                      const int* coff) {
  s.L.n_levels = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    upload_fmt(s.buf[l], fmt, maps[l], (size_t)n * h[l] * w[l] * cstride[l] * gtx::dtype_size(fmt));
    s.L.ptr[l] = s.buf[l].p; s.L.h[l] = h[l]; s.L.w[l] = w[l]; s.L.cstride[l] = cstride[l]; s.L.coff[l] = coff[l];
    s.S += h[l] * w[l];
  }
}
}  // namespace

int gtx_op_rt_linear(gtx_ctx* ctx, int M, int K, int Nout, const float* x, int ldx, const float* x2, int ldx2, int x2_cols, const float* w,
                     const float* bias, const float* res, int ldr, float* y, int ldy, int ycol, int act) {
  return guarded([&] {
    const char* op = "rt_linear";
    if (M < 1 || M > (1 << 20) || K < 16 || K % 16 || K > (1 << 16) || Nout < 16 || Nout % 16 || Nout > (1 << 16)) op_bad(op, "M >= 1, K and Nout positive multiples of 16");
    if (ldx < K || ldx % 4 || ldx > (1 << 20)) op_bad(op, "ldx must hold K values and be a multiple of 4");
    if (x2 && (ldx2 < K || ldx2 % 4 || ldx2 > (1 << 20) || x2_cols < 0 || (x2_cols % 64 && x2_cols < Nout)))
      op_bad(op, "the second addend needs ldx2 >= K, a multiple of 4, and x2_cols a multiple of 64 or all of Nout");
    if (res && (ldr < Nout || ldr > (1 << 20))) op_bad(op, "ldr must hold Nout values");
    if (ycol < 0 || ldy > (1 << 20) || (long)ycol + Nout > ldy) op_bad(op, "the output columns do not fit ldy");
    if (act != 0 && act != 2 && act != 3) op_bad(op, "act: 0 none, 2 ReLU, 3 GELU");
    need(ctx, "ctx"); need(x, "x"); need(w, "w"); need(y, "y");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf dx, dx2, dw, db, dr, dy;
    upload(dx, x, (size_t)M * ldx * 4);
    if (x2) upload(dx2, x2, (size_t)M * ldx2 * 4);
    upload(dw, w, (size_t)Nout * K * 4);
    if (bias) upload(db, bias, (size_t)Nout * 4);
    if (res) upload(dr, res, (size_t)M * ldr * 4);
    upload(dy, y, (size_t)M * ldy * 4);
    gtx::RtLinear p{};
    p.x = dx.as<float>(); p.ldx = ldx;
    p.x2 = x2 ? dx2.as<float>() : nullptr; p.ldx2 = ldx2; p.x2_cols = x2_cols;
    p.w = dw.as<float>(); p.bias = bias ? db.as<float>() : nullptr;
    p.res = res ? dr.as<float>() : nullptr; p.ldr = ldr;
    p.y = dy.as<float>() + ycol; p.ldy = ldy;
    p.M = M; p.K = K; p.Nout = Nout; p.act = act;
    gtx::launch_rt_linear(p, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(y, dy, (size_t)M * ldy * 4);
  });
}

int gtx_op_rt_layernorm(gtx_ctx* ctx, int rows, int C, int in_fmt, const void* in, int in_cstride, int in_coff, int out_fmt, void* out,
                        int out_cstride, int out_coff, const float* gamma, const float* beta, int* saturated) {
  return guarded([&] {
    const char* op = "rt_layernorm";
    if (rows < 1 || rows > (1 << 22) || C < 8 || C % 8 || C > 1024) op_bad(op, "rows >= 1, C a multiple of 8 up to 1024");
    const bool pair_ok = (in_fmt == GTX_F32 && (out_fmt == GTX_F32 || out_fmt == GTX_F32S || out_fmt == GTX_F16)) ||
                         (in_fmt == GTX_F32S && out_fmt == GTX_F32S) || (in_fmt == GTX_F16 && out_fmt == GTX_F16);
    if (!pair_ok) op_bad(op, "formats: F32 -> F32 / F32S / F16, F32S -> F32S, F16 -> F16");
    if (in_coff < 0 || in_coff % 8 || in_cstride % 8 || in_cstride > (1 << 16) || (long)in_coff + C > in_cstride || out_coff < 0 || out_coff % 8 ||
        out_cstride % 8 || out_cstride > (1 << 16) || (long)out_coff + C > out_cstride)
      op_bad(op, "channel strides / offsets must be multiples of 8 and hold C channels");
    need(ctx, "ctx"); need(in, "in"); need(out, "out"); need(gamma, "gamma"); need(beta, "beta");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t xb = (size_t)rows * in_cstride * gtx::dtype_size(in_fmt), yb = (size_t)rows * out_cstride * gtx::dtype_size(out_fmt);
    gtx::DevBuf dx, dy, dg, dbt, ds;
    upload_fmt(dx, in_fmt, in, xb); upload_fmt(dy, out_fmt, out, yb);
    upload(dg, gamma, (size_t)C * 4);
    upload(dbt, beta, (size_t)C * 4);
    zeros(ds, 4);
    const gtx::RtRows ri{dx.p, in_cstride, in_coff, in_fmt}, ro{dy.p, out_cstride, out_coff, out_fmt};
    gtx::launch_rt_layernorm(ri, ro, rows, C, dg.as<float>(), dbt.as<float>(), ds.as<int>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, out_fmt, dy, yb);
    if (saturated) download(saturated, ds, 4);
  });
}

int gtx_op_rt_mha(gtx_ctx* ctx, int n, int T, int C, int heads, const float* qkv, int ld, float* out, int ldo, int form) {
  return guarded([&] {
    const char* op = "rt_mha";
    if (n < 1 || n > 1024 || T < 1 || T > (1 << 20) || heads < 1 || C < 1 || C % heads) op_bad(op, "bad sizes");
    const int d = C / heads;
    if (d != 8 && d != 16 && d != 32) op_bad(op, "head dimension 8, 16 or 32");
    if (ld < 3 * C || ld % 4 || ld > (1 << 16) || ldo < C || ldo % 4 || ldo > (1 << 16)) op_bad(op, "ld >= 3 C, ldo >= C, both multiples of 4");
    if (form != 0 && form != 1) op_bad(op, "form: 0 the library's rule, 1 the generic kernel");
    need(ctx, "ctx"); need(qkv, "qkv"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf dq, dout;
    upload(dq, qkv, (size_t)n * T * ld * 4);
    upload(dout, out, (size_t)n * T * ldo * 4);
    gtx::launch_rt_mha(dq.as<float>(), ld, n, T, C, heads, dout.as<float>(), ldo, ctx->stream, form);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(out, dout, (size_t)n * T * ldo * 4);
  });
}

int gtx_op_rt_topk(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* scores, const int* h, const int* w, const int* cstride,
                   const int* coff, int nc, int nq, int* idx) {
  return guarded([&] {
    const char* op = "rt_topk";
    rt_levels_check(op, fmt, n, n_levels, scores, h, w, cstride, coff, nc, false);
    long S = 0;
    for (int l = 0; l < n_levels; ++l) S += (long)h[l] * w[l];
    if (nq < 1 || nq > 1024 || S < nq) op_bad(op, "1..1024 queries, no more than there are anchors");
    need(ctx, "ctx"); need(idx, "idx");
    GTX_HIP(hipSetDevice(ctx->device));
    RtLevelSet lv;
    rt_levels_upload(lv, fmt, n, n_levels, scores, h, w, cstride, coff);
    gtx::DevBuf keys((size_t)n * lv.S * 4), di((size_t)n * nq * 4);
    gtx::launch_rt_topk(fmt, lv.L, nc, n, nq, keys.as<unsigned>(), di.as<int>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(idx, di, (size_t)n * nq * 4);
  });
}

int gtx_op_rt_gather_refer(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* enc, const int* h, const int* w, const int* cstride,
                           const int* coff, int C, int nq, const int* idx, const float* delta, int ldd, int mode, float* embed, float* anchors,
                           float* refer) {
  return guarded([&] {
    const char* op = "rt_gather_refer";
    if (mode != 0 && mode != 1) op_bad(op, "mode 0 (gather + anchors) or 1 (inverse sigmoid of refer)");
    if (n < 1 || nq < 1 || (long)n * nq > (1 << 20) || ldd < 4 || ldd > (1 << 16)) op_bad(op, "bad sizes");
    need(delta, "delta"); need(refer, "refer");
    const int M = n * nq;
    if (mode == 0) {
      rt_levels_check(op, fmt, n, n_levels, enc, h, w, cstride, coff, C, true);
      need(idx, "idx"); need(embed, "embed"); need(anchors, "anchors");
      long S = 0;
      for (int l = 0; l < n_levels; ++l) S += (long)h[l] * w[l];
      for (int m = 0; m < M; ++m)
        if (idx[m] < 0 || idx[m] >= S) op_bad(op, "an anchor index is outside the level set");
    }
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf dd, dr;
    upload(dd, delta, (size_t)M * ldd * 4);
    if (mode == 1) {
      upload(dr, refer, (size_t)M * 16 * 4);
      gtx::launch_rt_refer(dd.as<float>(), ldd, nullptr, dr.as<float>(), M, 1, ctx->stream);
    } else {
      RtLevelSet lv;
      rt_levels_upload(lv, fmt, n, n_levels, enc, h, w, cstride, coff);
      gtx::DevBuf di, de((size_t)M * C * 4), da((size_t)M * 4 * 4);
      upload(di, idx, (size_t)M * 4);
      zeros(dr, (size_t)M * 16 * 4);
      gtx::launch_rt_gather(fmt, lv.L, C, n, nq, di.as<int>(), de.as<float>(), da.as<float>(), ctx->stream);
      gtx::launch_rt_refer(dd.as<float>(), ldd, da.as<float>(), dr.as<float>(), M, 0, ctx->stream);
      GTX_HIP(hipStreamSynchronize(ctx->stream));
      download(embed, de, (size_t)M * C * 4);
      download(anchors, da, (size_t)M * 4 * 4);
    }
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(refer, dr, (size_t)M * 16 * 4);
  });
}

int gtx_op_rt_deform(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* value, const int* h, const int* w, const int* cstride,
                     const int* coff, int hd, int nh, int npts, int nq, const float* offaw, const float* refer, float* out) {
  return guarded([&] {
    const char* op = "rt_deform";
    if (hd < 1 || hd > 1024 || nh < 1 || hd % nh || npts < 1 || npts > 64 || nq < 1 || n < 1 || (long)n * nq > (1 << 20)) op_bad(op, "bad sizes");
    rt_levels_check(op, fmt, n, n_levels, value, h, w, cstride, coff, hd, true);
    need(ctx, "ctx"); need(offaw, "offaw"); need(refer, "refer"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    const int M = n * nq;
    RtLevelSet lv;
    rt_levels_upload(lv, fmt, n, n_levels, value, h, w, cstride, coff);
    gtx::DevBuf dof, dr, dout((size_t)M * hd * 4);
    upload(dof, offaw, (size_t)M * nh * n_levels * npts * 3 * 4);
    upload(dr, refer, (size_t)M * 16 * 4);
    gtx::launch_rt_deform(fmt, lv.L, hd, nh, npts, dof.as<float>(), dr.as<float>(), n, nq, dout.as<float>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(out, dout, (size_t)M * hd * 4);
  });
}

int gtx_op_rt_post(gtx_ctx* ctx, int n, int nq, int nc, const float* logits, int ldl, const float* refer, float conf, uint64_t class_mask0,
                   uint64_t class_mask1, int frame_w, int frame_h, int max_det, float* out_rows, int* out_n, float* raw) {
  return guarded([&] {
    const char* op = "rt_post";
    if (nq < 1 || nq > 512) op_bad(op, "1..512 queries");
    if (nc < 1 || nc > 128) op_bad(op, "1..128 classes (the class mask has two 64-bit words)");
    if (n < 1 || n > 4096 || ldl < nc || ldl > (1 << 16) || max_det < 1 || max_det > (1 << 16) || frame_w < 1 || frame_h < 1) op_bad(op, "bad sizes");
    need(ctx, "ctx"); need(logits, "logits"); need(refer, "refer"); need(out_rows, "out_rows"); need(out_n, "out_n");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t M = (size_t)n * nq, rawb = M * (4 + nc) * 4, rowb = (size_t)n * max_det * 6 * 4;
    gtx::DevBuf dl, dr, drows, dn, draw(raw ? rawb : 16);
    upload(dl, logits, M * ldl * 4);
    upload(dr, refer, M * 16 * 4);
    upload(drows, out_rows, rowb);
    zeros(dn, (size_t)n * 4);
    const unsigned long long mask[2] = {class_mask0, class_mask1};
    gtx::launch_rt_post(dl.as<float>(), ldl, dr.as<float>(), n, nq, nc, conf, mask, frame_w, frame_h, max_det, drows.as<float>(), dn.as<int>(),
                        raw ? draw.as<float>() : nullptr, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(out_rows, drows, rowb);
    download(out_n, dn, (size_t)n * 4);
    if (raw) download(raw, draw, rawb);
  });
}

// ---- RT-DETR's map-side kernels, one hook per launcher (tests/test_rtdetr_map_ops_gpu.py). As above: every size is checked before
// anything touches the GPU. Every map holds n_alloc images of which the first n run: what lies behind them, and beside a channel
// slice, is uploaded as given and comes back with the output, so a test sees a read or a write outside the launch's own data.
namespace {
void rt_map_fmt_check(const char* op, int dtype) {
  if (dtype != GTX_F16 && dtype != GTX_F32 && dtype != GTX_F32S) op_bad(op, "dtype: GTX_F16, GTX_F32 or GTX_F32S");
}
void rt_map_batch_check(const char* op, int n, int n_alloc) {
  if (n < 1 || n_alloc < n || n_alloc > 4096) op_bad(op, "n >= 1 and n <= n_alloc <= 4096");
}
// c channels (whole groups of `group`) at coff of an [n_alloc][h][w][cstride] map: the kernels move 16- and 32-byte groups of 8 channels
void rt_map_check(const char* op, int n_alloc, int h, int w, int c, int cstride, int coff, int group = 8) {
  if (h < 1 || w < 1 || h > (1 << 14) || w > (1 << 14)) op_bad(op, "h and w must be 1..16384");
  if (c < group || c % group) op_bad(op, group == 16 ? "the channel count must be a positive multiple of 16" : "the channel count must be a positive multiple of 8");
  if (cstride < 8 || cstride % 8 || cstride > (1 << 16) || coff < 0 || coff % 8) op_bad(op, "channel strides and offsets must be multiples of 8");
  if ((long)coff + c > cstride) op_bad(op, "a channel slice does not fit its stride");
  if ((double)n_alloc * h * w * cstride > 1e9) op_bad(op, "maps too large");
}
size_t rt_map_bytes(int dtype, int n_alloc, int h, int w, int cstride) { return (size_t)n_alloc * h * w * cstride * gtx::dtype_size(dtype); }
}  // namespace

int gtx_op_rt_stem1(gtx_ctx* ctx, int dtype, int n, int n_alloc, int H, int W, int c0, const void* img, const float* w27, const float* bias, void* out,
                    int out_cstride, int out_coff, int* saturated) {
  return guarded([&] {
    const char* op = "rt_stem1";
    rt_map_fmt_check(op, dtype);
    rt_map_batch_check(op, n, n_alloc);
    if (H < 2 || W < 2 || H % 2 || W % 2) op_bad(op, "H and W must be even and at least 2");
    if (c0 > 1024) op_bad(op, "at most 1024 channels");
    rt_map_check(op, n_alloc, H / 2, W / 2, c0, out_cstride, out_coff, 16);
    need(img, "img"); need(w27, "w27"); need(bias, "bias"); need(out, "out"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t ob = rt_map_bytes(dtype, n_alloc, H / 2, W / 2, out_cstride);
    gtx::DevBuf dimg, dw, db, dout, ds;
    upload(dimg, img, (size_t)n_alloc * H * W * 4);
    upload(dw, w27, (size_t)27 * c0 * 4); upload(db, bias, (size_t)c0 * 4);
    upload_fmt(dout, dtype, out, ob);
    zeros(ds, 4);
    const gtx::RtMap o{dout.p, H / 2, W / 2, out_cstride, out_coff, c0};
    gtx::launch_rt_stem1(dtype, dimg.p, n, H, W, dw.as<float>(), db.as<float>(), o, ds.as<int>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dout, ob);
    if (saturated) download(saturated, ds, 4);
  });
}

int gtx_op_rt_pool2(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, const void* in, int in_cstride, int in_coff, void* out,
                    int out_cstride, int out_coff, int* saturated) {
  return guarded([&] {
    const char* op = "rt_pool2";
    rt_map_fmt_check(op, dtype);
    rt_map_batch_check(op, n, n_alloc);
    rt_map_check(op, n_alloc, h, w, c, in_cstride, in_coff);
    rt_map_check(op, n_alloc, h, w, c, out_cstride, out_coff);
    need(in, "in"); need(out, "out"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t xb = rt_map_bytes(dtype, n_alloc, h, w, in_cstride), yb = rt_map_bytes(dtype, n_alloc, h, w, out_cstride);
    gtx::DevBuf dx, dy, ds;
    upload_fmt(dx, dtype, in, xb); upload_fmt(dy, dtype, out, yb);
    zeros(ds, 4);
    const gtx::RtMap i{dx.p, h, w, in_cstride, in_coff, c}, o{dy.p, h, w, out_cstride, out_coff, c};
    gtx::launch_rt_pool2(dtype, i, o, n, ds.as<int>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dy, yb);
    if (saturated) download(saturated, ds, 4);
  });
}

int gtx_op_rt_dwconv(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, int k, int stride, const void* x, int in_cstride, int in_coff,
                     const float* wt, const float* bias, int act, const void* res, int res_cstride, int res_coff, void* out, int out_cstride, int out_coff,
                     int* saturated) {
  return guarded([&] {
    const char* op = "rt_dwconv";
    rt_map_fmt_check(op, dtype);
    rt_map_batch_check(op, n, n_alloc);
    if ((k != 3 && k != 5 && k != 7) || (stride != 1 && stride != 2)) op_bad(op, "k must be 3, 5 or 7 and the stride 1 or 2");
    if (act < 0 || act > 2) op_bad(op, "act: 0 none, 1 SiLU, 2 ReLU");
    rt_map_check(op, n_alloc, h, w, c, in_cstride, in_coff);
    const int ho = (h - 1) / stride + 1, wo = (w - 1) / stride + 1;
    rt_map_check(op, n_alloc, ho, wo, c, out_cstride, out_coff);
    if (res) rt_map_check(op, n_alloc, ho, wo, c, res_cstride, res_coff);
    need(x, "x"); need(wt, "w"); need(out, "out"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t xb = rt_map_bytes(dtype, n_alloc, h, w, in_cstride), yb = rt_map_bytes(dtype, n_alloc, ho, wo, out_cstride);
    gtx::DevBuf dx, dy, dr, dw, db, ds;
    upload_fmt(dx, dtype, x, xb); upload_fmt(dy, dtype, out, yb);
    if (res) upload_fmt(dr, dtype, res, rt_map_bytes(dtype, n_alloc, ho, wo, res_cstride));
    upload(dw, wt, (size_t)k * k * c * 4);
    if (bias) upload(db, bias, (size_t)c * 4);
    zeros(ds, 4);
    const gtx::RtMap i{dx.p, h, w, in_cstride, in_coff, c}, o{dy.p, ho, wo, out_cstride, out_coff, c}, r{dr.p, ho, wo, res_cstride, res_coff, c};
    gtx::launch_rt_dwconv(dtype, i, o, n, k, stride, dw.as<float>(), bias ? db.as<float>() : nullptr, act, ds.as<int>(), ctx->stream, res ? &r : nullptr);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(out, dtype, dy, yb);
    if (saturated) download(saturated, ds, 4);
  });
}

int gtx_op_rt_upsample2x(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, const void* x, int in_cstride, int in_coff, void* y,
                         int out_cstride, int out_coff) {
  return guarded([&] {
    const char* op = "rt_upsample2x";
    rt_map_fmt_check(op, dtype);
    rt_map_batch_check(op, n, n_alloc);
    rt_map_check(op, n_alloc, h, w, c, in_cstride, in_coff);
    rt_map_check(op, n_alloc, 2 * h, 2 * w, c, out_cstride, out_coff);
    need(x, "x"); need(y, "y"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t xb = rt_map_bytes(dtype, n_alloc, h, w, in_cstride), yb = rt_map_bytes(dtype, n_alloc, 2 * h, 2 * w, out_cstride);
    gtx::DevBuf dx, dy;
    upload_fmt(dx, dtype, x, xb); upload_fmt(dy, dtype, y, yb);
    gtx::launch_upsample2x(gtx::dtype_size(dtype), dx.p, n, h, w, c, in_cstride, in_coff, dy.p, out_cstride, out_coff, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(y, dtype, dy, yb);
  });
}

int gtx_op_rt_tokens_in(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, const void* in, int in_cstride, int in_coff, const float* pos,
                        float* src, float* q) {
  return guarded([&] {
    const char* op = "rt_tokens_in";
    rt_map_fmt_check(op, dtype);
    rt_map_batch_check(op, n, n_alloc);
    rt_map_check(op, n_alloc, h, w, c, in_cstride, in_coff);
    if ((pos == nullptr) != (q == nullptr)) op_bad(op, "pos and q are given together or not at all");
    need(in, "in"); need(src, "src"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t tb = (size_t)n_alloc * h * w * c * 4;
    gtx::DevBuf dx, dp, dsrc, dq;
    upload_fmt(dx, dtype, in, rt_map_bytes(dtype, n_alloc, h, w, in_cstride));
    upload(dsrc, src, tb);
    if (q) {
      upload(dp, pos, (size_t)h * w * c * 4);
      upload(dq, q, tb);
    }
    const gtx::RtMap i{dx.p, h, w, in_cstride, in_coff, c};
    gtx::launch_rt_tokens_in(dtype, i, n, q ? dp.as<float>() : nullptr, dsrc.as<float>(), q ? dq.as<float>() : nullptr, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(src, dsrc, tb);
    if (q) download(q, dq, tb);
  });
}

int gtx_op_rt_mask_invalid(gtx_ctx* ctx, int dtype, int n, int n_alloc, int h, int w, int c, void* m, int cstride, int coff, int level) {
  return guarded([&] {
    const char* op = "rt_mask_invalid";
    rt_map_fmt_check(op, dtype);
    rt_map_batch_check(op, n, n_alloc);
    rt_map_check(op, n_alloc, h, w, c, cstride, coff);
    if (level < 0 || level > 5) op_bad(op, "level must be 0..5");
    need(m, "m"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t mb = rt_map_bytes(dtype, n_alloc, h, w, cstride);
    gtx::DevBuf dm;
    upload_fmt(dm, dtype, m, mb);
    const gtx::RtMap mm{dm.p, h, w, cstride, coff, c};
    gtx::launch_rt_mask_invalid(dtype, mm, n, level, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download_fmt(m, dtype, dm, mb);
  });
}

// ---- the detector's post-pass kernels, one hook per launcher (tests/test_head_ops_gpu.py). As above: every size, and every index a
// kernel would follow, is checked before anything touches the GPU.
namespace {
struct HeadSet {
  gtx::HeadParams hp{};
  gtx::DevBuf feat[gtx::kMaxLevels], wb[gtx::kMaxLevels], bb[gtx::kMaxLevels], wc[gtx::kMaxLevels], bc[gtx::kMaxLevels];
};
// gate: the class branch is read (16-byte loads); boxes: the box branch is
long head_check(const char* op, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, bool gate, bool boxes) {
  if (dtype != GTX_F16 && dtype != GTX_F32) op_bad(op, "maps are GTX_F16 or GTX_F32");
  if (n_levels > gtx::kMaxLevels) op_bad(op, "at most 4 levels");
  if (n < 1 || n > 64 || n_levels < 1) op_bad(op, "bad sizes");
  if (gate && (nc < 1 || nc > 128)) op_bad(op, "1..128 classes (the class mask has two 64-bit words)");
  need(lv, "lv");
  const int al = dtype == GTX_F16 ? 8 : 4;          // elements in 16 bytes
  long A = 0;
  for (int l = 0; l < n_levels; ++l) {
    const gtx_head_level& L = lv[l];
    need(L.feat, "lv[l].feat");
    if (L.h < 1 || L.w < 1 || L.cb < 0 || L.cc < 0 || L.cstride < 1 || L.cstride > (1 << 16) || (long)L.cb + L.cc > L.cstride)
      op_bad(op, "a level's channels do not fit its stride");
    if ((double)n * L.h * L.w * L.cstride > 2.5e8) op_bad(op, "maps too large");
    A += (long)L.h * L.w;
    if (gate) {
      need(L.wc, "lv[l].wc"); need(L.bc, "lv[l].bc");
      if (L.cc < 8 || L.cc % 8) op_bad(op, "cc must be a positive multiple of 8 (the kernel reads 8-channel chunks)");
      if (L.cb % al || L.cstride % al) op_bad(op, "cb and cstride must keep the class features 16-byte aligned");
    }
    if (boxes) {
      need(L.wb, "lv[l].wb"); need(L.bb, "lv[l].bb");
      if (L.cb < 1 || L.cb > 128) op_bad(op, "1..128 box channels");
      if (L.cb > lv[0].cb) op_bad(op, "no level's cb may exceed level 0's (the kernel's LDS layout)");
    }
  }
  if (A > (1l << 22)) op_bad(op, "too many anchors");
  return A;
}
void head_upload(HeadSet& s, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, bool gate, bool boxes, int box_out = 64) {
  s.hp.n_levels = n_levels;
  s.hp.nc = nc;
  int anchor = 0;
  for (int l = 0; l < n_levels; ++l) {
    const gtx_head_level& L = lv[l];
    gtx::HeadLevel& H = s.hp.lv[l];
    upload(s.feat[l], L.feat, (size_t)n * L.h * L.w * L.cstride * gtx::dtype_size(dtype));
    H.feat = s.feat[l].p; H.h = L.h; H.w = L.w; H.cstride = L.cstride; H.cb = L.cb; H.cc = L.cc; H.stride = L.stride;
    H.anchor_begin = anchor;
    anchor += L.h * L.w;
    if (gate) {
      upload(s.wc[l], L.wc, (size_t)nc * L.cc * 4);
      upload(s.bc[l], L.bc, (size_t)nc * 4);
      H.wc = s.wc[l].as<float>(); H.bc = s.bc[l].as<float>();
    }
    if (boxes) {
      upload(s.wb[l], L.wb, (size_t)L.cb * box_out * 4);
      upload(s.bb[l], L.bb, (size_t)box_out * 4);
      H.wb = s.wb[l].as<float>(); H.bb = s.bb[l].as<float>();
    }
  }
  s.hp.n_anchors = anchor;
}
// the first min(count, cap) entries of every image index an anchor below `anchors`
void cand_check(const char* op, int n, int cap, const int* count, const int* anchor, long anchors) {
  need(count, "count"); need(anchor, "anchor");
  for (int b = 0; b < n; ++b) {
    if (count[b] < 0) op_bad(op, "a negative count");
    const int m = std::min(count[b], cap);
    for (int i = 0; i < m; ++i)
      if (anchor[(size_t)b * cap + i] < 0 || anchor[(size_t)b * cap + i] >= anchors) op_bad(op, "an anchor index is outside the level set");
  }
}
void geometry_check(const char* op, int src_h, int src_w, int net_h, int net_w, double gain) {
  if (src_h < 1 || src_w < 1 || net_h < 1 || net_w < 1 || src_h > (1 << 16) || src_w > (1 << 16) || net_h > (1 << 16) || net_w > (1 << 16) || !(gain > 0.0))
    op_bad(op, "bad letterbox geometry");
}
gtx::Letterbox geometry(int src_h, int src_w, int net_h, int net_w, double gain) {
  gtx::Letterbox lb{};
  lb.src_h = src_h; lb.src_w = src_w; lb.net_h = net_h; lb.net_w = net_w; lb.gain = gain;
  return lb;
}
}  // namespace

int gtx_op_head_gate(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, float conf, uint64_t class_mask0,
                     uint64_t class_mask1, int cap, int lvl_cap, int* count, float* cand_score, int* cand_anchor, int* cand_cls, int* lvl_count,
                     int* lvl_list) {
  return guarded([&] {
    const char* op = "head_gate";
    head_check(op, dtype, n, n_levels, lv, nc, true, false);
    if (cap < 1 || cap > (1 << 22) || lvl_cap < 0 || lvl_cap > (1 << 22)) op_bad(op, "cap >= 1, lvl_cap >= 0");
    need(count, "count"); need(cand_score, "cand_score"); need(cand_anchor, "cand_anchor"); need(cand_cls, "cand_cls");
    if (lvl_cap) { need(lvl_count, "lvl_count"); need(lvl_list, "lvl_list"); }
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    HeadSet hs;
    head_upload(hs, dtype, n, n_levels, lv, nc, true, false);
    hs.hp.conf = conf;
    hs.hp.class_mask[0] = class_mask0; hs.hp.class_mask[1] = class_mask1;
    const size_t m = (size_t)n * cap, lb = (size_t)n * gtx::kMaxLevels * (size_t)std::max(lvl_cap, 1) * 4;
    gtx::DevBuf dc, ds, da, dk, dlc, dll;
    fill_ff(dc, (size_t)n * 4); fill_ff(ds, m * 4); fill_ff(da, m * 4); fill_ff(dk, m * 4);
    gtx::NmsBuffers nb{};
    nb.cap = cap;
    nb.count = dc.as<int>(); nb.cand_score = ds.as<float>(); nb.cand_anchor = da.as<int>(); nb.cand_cls = dk.as<int>();
    if (lvl_cap) {
      fill_ff(dlc, (size_t)n * gtx::kMaxLevels * 4); fill_ff(dll, lb);
      nb.lvl_count = dlc.as<int>(); nb.lvl_list = dll.as<int>(); nb.lvl_cap = lvl_cap;
    }
    gtx::launch_head_gate(dtype, hs.hp, n, nb, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(count, dc, (size_t)n * 4); download(cand_score, ds, m * 4); download(cand_anchor, da, m * 4); download(cand_cls, dk, m * 4);
    if (lvl_cap) { download(lvl_count, dlc, (size_t)n * gtx::kMaxLevels * 4); download(lvl_list, dll, lb); }
  });
}

namespace {
// box_out: 64 (4 x 16 DFL bins) or 4 (reg_max = 1)
void head_boxes_op(const char* op, int box_out, gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int cap, const int* count,
                   const int* cand_anchor, float* cand_box) {
  const long A = head_check(op, dtype, n, n_levels, lv, 0, false, true);
  if (cap < 1 || cap > (1 << 22)) op_bad(op, "cap >= 1");
  cand_check(op, n, cap, count, cand_anchor, A);
  need(cand_box, "cand_box"); need(ctx, "ctx");
  GTX_HIP(hipSetDevice(ctx->device));
  HeadSet hs;
  head_upload(hs, dtype, n, n_levels, lv, 0, false, true, box_out);
  hs.hp.reg_max = box_out / 4;
  const size_t m = (size_t)n * cap;
  gtx::DevBuf dc, da, db;
  upload(dc, count, (size_t)n * 4); upload(da, cand_anchor, m * 4); fill_ff(db, m * 16);
  gtx::NmsBuffers nb{};
  nb.cap = cap;
  nb.count = dc.as<int>(); nb.cand_anchor = da.as<int>(); nb.cand_box = db.as<float>();
  gtx::launch_head_boxes(dtype, hs.hp, n, nb, ctx->stream);
  GTX_HIP(hipStreamSynchronize(ctx->stream));
  download(cand_box, db, m * 16);
}
}  // namespace

int gtx_op_head_boxes(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int cap, const int* count, const int* cand_anchor,
                      float* cand_box) {
  return guarded([&] { head_boxes_op("head_boxes", 64, ctx, dtype, n, n_levels, lv, cap, count, cand_anchor, cand_box); });
}

int gtx_op_head_boxes_r1(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int cap, const int* count, const int* cand_anchor,
                         float* cand_box) {
  return guarded([&] { head_boxes_op("head_boxes_r1", 4, ctx, dtype, n, n_levels, lv, cap, count, cand_anchor, cand_box); });
}

// The sparse box launch (head_sparse.hip; tests/test_head_sparse_ops_gpu.py): the levels' maps go up in the pair format, the first
// layer's whole stack is packed as the detector packs it and the kernel gets its tile 0 with the stack's scale (Detector::plan_sparse_box).
int gtx_op_head_sparse_box(gtx_ctx* ctx, int n, int n_levels, const gtx_sparse_level* lv, int reg_max, int cap, int lvl_cap, const int* count,
                           const int* cand_anchor, const int* lvl_count, const int* lvl_list, float* cand_box, int* sat) {
  return guarded([&] {
    const char* op = "head_sparse_box";
    if (n_levels > gtx::kMaxLevels) op_bad(op, "at most 4 levels");
    if (n < 1 || n > 64 || n_levels < 1) op_bad(op, "bad sizes");
    if (reg_max != 16 && reg_max != 1) op_bad(op, "reg_max is 16 or 1");
    if (cap < 1 || cap > (1 << 22)) op_bad(op, "cap >= 1");
    if (lvl_cap < 1 || lvl_cap > (1 << 22)) op_bad(op, "lvl_cap >= 1");
    need(lv, "lv");
    long begin[gtx::kMaxLevels + 1] = {0};
    for (int l = 0; l < n_levels; ++l) {
      const gtx_sparse_level& L = lv[l];
      need(L.feat, "lv[l].feat"); need(L.w1, "lv[l].w1"); need(L.b1, "lv[l].b1"); need(L.w2, "lv[l].w2"); need(L.b2, "lv[l].b2");
      need(L.wb, "lv[l].wb"); need(L.bb, "lv[l].bb");
      if (L.h < 1 || L.w < 1 || L.cstride < 1 || L.cstride > (1 << 16) || L.cstride % 8) op_bad(op, "a level's map: h, w >= 1, cstride a multiple of 8");
      if (L.cin < 32 || L.cin % 32) op_bad(op, "cin must be a positive multiple of 32 (the kernel's K chunk)");
      if (L.coff < 0 || L.coff % 8) op_bad(op, "coff must be a multiple of 8 (whole pair-format groups)");
      if ((long)L.coff + L.cin > L.cstride) op_bad(op, "a level's channels do not fit its stride");
      if (L.c1out < 64 || L.c1out % 64 || L.c1out > 1024) op_bad(op, "c1out must be a multiple of 64 in [64, 1024]");
      if ((double)n * L.h * L.w * L.cstride > 2.5e8) op_bad(op, "maps too large");
      begin[l + 1] = begin[l] + (long)L.h * L.w;
    }
    if (begin[n_levels] > (1l << 22)) op_bad(op, "too many anchors");
    need(count, "count"); need(cand_anchor, "cand_anchor"); need(lvl_count, "lvl_count"); need(lvl_list, "lvl_list");
    // every entry the kernel follows: lvl_list -> cand_anchor -> a cell of the level it is filed under
    for (int b = 0; b < n; ++b)
      for (int l = 0; l < n_levels; ++l) {
        const int c = lvl_count[b * gtx::kMaxLevels + l];
        if (c < 0) op_bad(op, "a negative lvl_count");
        const int* list = lvl_list + ((size_t)b * gtx::kMaxLevels + l) * lvl_cap;
        for (int k = 0; k < std::min(c, lvl_cap); ++k) {
          if (list[k] < 0 || list[k] >= cap) op_bad(op, "a lvl_list entry is outside [0, cap)");
          const int a = cand_anchor[(size_t)b * cap + list[k]];
          if (a < begin[l] || a >= begin[l + 1]) op_bad(op, "an entry's anchor is not inside the level it is filed under");
        }
      }
    need(cand_box, "cand_box"); need(sat, "sat"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    // What conv_pick_config gives the K32 form (32-channel chunks, 64-cout tiles), written out: the pick follows GTX_K32, and
    // pack_conv_weights_split reads kc, ks and bn only. A copy: if the K32 form's packing parameters change, change them here too --
    // the detector feeds the kernel the pick's image (Detector::plan_sparse_box), and only the dense-route case of
    // tests/test_head_sparse_ops_gpu.py would notice a difference.
    gtx::ConvConfig k32{};
    k32.variant = gtx::ConvForm::K32; k32.dtype = GTX_F32S; k32.ks = 3; k32.stride = 1; k32.kc = 32; k32.bn = 64; k32.th = 8; k32.tw = 16;
    const int box_out = 4 * reg_max;
    gtx::DevBuf feat[gtx::kMaxLevels], w1[gtx::kMaxLevels], b1[gtx::kMaxLevels], w2[gtx::kMaxLevels], b2[gtx::kMaxLevels], wb[gtx::kMaxLevels],
        bb[gtx::kMaxLevels], dc, da, dlc, dll, db, dsat;
    gtx::SparseBox sb{};
    for (int l = 0; l < n_levels; ++l) {
      const gtx_sparse_level& L = lv[l];
      gtx::SparseBoxLevel& S = sb.lv[l];
      upload_fmt(feat[l], GTX_F32S, L.feat, (size_t)n * L.h * L.w * L.cstride * 4);
      const std::vector<uint8_t> i1 = gtx::pack_conv_weights_split(L.w1, L.c1out, L.cin, k32, &S.sc1);
      const std::vector<uint8_t> i2 = gtx::pack_conv_weights_split(L.w2, 64, 64, k32, &S.sc2);
      upload(w1[l], i1.data(), i1.size()); upload(b1[l], L.b1, (size_t)L.c1out * 4);
      upload(w2[l], i2.data(), i2.size()); upload(b2[l], L.b2, 64 * 4);
      upload(wb[l], L.wb, (size_t)64 * box_out * 4); upload(bb[l], L.bb, (size_t)box_out * 4);
      S.in = feat[l].p; S.H = L.h; S.W = L.w; S.cstride = L.cstride; S.coff = L.coff; S.cin = L.cin;
      S.w1 = w1[l].p; S.b1 = b1[l].as<float>();          // tile 0 of the stack is the image's first 64-cout tile
      S.w2 = w2[l].p; S.b2 = b2[l].as<float>();
      S.wb = wb[l].as<float>(); S.bb = bb[l].as<float>(); S.stride = L.stride; S.anchor_begin = (int)begin[l];
    }
    const size_t m = (size_t)n * cap, lb = (size_t)n * gtx::kMaxLevels * lvl_cap * 4;
    upload(dc, count, (size_t)n * 4); upload(da, cand_anchor, m * 4);
    upload(dlc, lvl_count, (size_t)n * gtx::kMaxLevels * 4); upload(dll, lvl_list, lb);
    fill_ff(db, m * 16); zeros(dsat, 4);
    sb.n_levels = n_levels; sb.cap = lvl_cap; sb.sat_flag = dsat.as<int>(); sb.reg_max = reg_max;
    gtx::NmsBuffers nb{};
    nb.cap = cap;
    nb.count = dc.as<int>(); nb.cand_anchor = da.as<int>(); nb.cand_box = db.as<float>();
    nb.lvl_count = dlc.as<int>(); nb.lvl_list = dll.as<int>(); nb.lvl_cap = lvl_cap;
    gtx::launch_head_sparse_box(sb, n, nb, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(cand_box, db, m * 16); download(sat, dsat, 4);
  });
}

int gtx_op_nms(gtx_ctx* ctx, int n, int cap, const int* count, const float* cand_score, const int* cand_anchor, const int* cand_cls,
               const float* cand_box, float iou_thr, int agnostic, int max_nms, int nms_cap, int max_det, int src_h, int src_w, int net_h, int net_w,
               double gain, int which, float* out_rows, int* out_n, int* out_anchor) {
  return guarded([&] {
    const char* op = "nms";
    if (n < 1 || n > 64 || cap < 1 || cap > (1 << 20) || max_det < 1 || max_det > (1 << 16) || max_nms < 1) op_bad(op, "bad sizes");
    if (nms_cap < 64 || nms_cap % 64 || nms_cap > 32768 || (double)n * nms_cap * (nms_cap / 64) * 8 > 3e8) op_bad(op, "nms_cap: a multiple of 64, the mask within 300 MB");
    if (which < 0 || which > 2) op_bad(op, "which: 0 both paths, 1 the single-workgroup kernel, 2 the general kernels");
    geometry_check(op, src_h, src_w, net_h, net_w, gain);
    cand_check(op, n, cap, count, cand_anchor, gtx::nms_max_anchors());
    need(cand_score, "cand_score"); need(cand_cls, "cand_cls"); need(cand_box, "cand_box"); need(out_rows, "out_rows"); need(out_n, "out_n");
    need(out_anchor, "out_anchor");
    for (int b = 0; b < n; ++b)
      for (int i = 0; i < std::min(count[b], cap); ++i) {
        if (!(cand_score[(size_t)b * cap + i] > 0.f)) op_bad(op, "scores must be positive (the sort key is their bit pattern)");
        if (cand_cls[(size_t)b * cap + i] < 0 || cand_cls[(size_t)b * cap + i] > 127) op_bad(op, "classes 0..127");
      }
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t m = (size_t)n * cap, sm = (size_t)n * nms_cap, rows = (size_t)n * max_det;
    gtx::DevBuf dc, ds, da, dk, db, dsn, sb(sm * 16), ss(sm * 4), sc(sm * 4), sa(sm * 4), dm(sm * (nms_cap / 64) * 8), dn, dr, doa;
    upload(dc, count, (size_t)n * 4); upload(ds, cand_score, m * 4); upload(da, cand_anchor, m * 4); upload(dk, cand_cls, m * 4);
    upload(db, cand_box, m * 16);
    upload(dn, out_n, (size_t)n * 4); upload(dr, out_rows, rows * 24); upload(doa, out_anchor, rows * 4);
    zeros(dsn, (size_t)n * 4);                         // which == 2 alone: an image left to the other path has nothing sorted
    gtx::NmsBuffers nb{};
    nb.cap = cap;
    nb.count = dc.as<int>(); nb.cand_score = ds.as<float>(); nb.cand_anchor = da.as<int>(); nb.cand_cls = dk.as<int>(); nb.cand_box = db.as<float>();
    nb.nms_cap = nms_cap;
    nb.sorted_n = dsn.as<int>(); nb.s_box = sb.as<float>(); nb.s_score = ss.as<float>(); nb.s_cls = sc.as<int>(); nb.s_anchor = sa.as<int>();
    nb.mask = dm.as<unsigned long long>();
    nb.max_det = max_det;
    nb.out_n = dn.as<int>(); nb.out_rows = dr.as<float>(); nb.out_anchor = doa.as<int>();
    gtx::launch_nms(nb, n, iou_thr, agnostic != 0, max_nms, geometry(src_h, src_w, net_h, net_w, gain), ctx->stream, which);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(out_n, dn, (size_t)n * 4); download(out_rows, dr, rows * 24); download(out_anchor, doa, rows * 4);
  });
}

int gtx_op_v10_select(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, float conf, int cap, const int* count,
                      const float* cand_score, const int* cand_anchor, int sel_cap, int lvl_cap, int* sel_count, float* sel_score, int* sel_anchor,
                      int* sel_cls, int* lvl_count, int* lvl_list, float* scores, int* score_anchor) {
  return guarded([&] {
    const char* op = "v10_select";
    const long A = head_check(op, dtype, n, n_levels, lv, nc, true, false);
    if (cap < 1 || cap > (1 << 22)) op_bad(op, "cap >= 1");
    if (sel_cap < gtx::kV10Keep || sel_cap > 512) op_bad(op, "sel_cap in [300, 512]");
    if (lvl_cap != 0 && (lvl_cap < gtx::kV10Keep || lvl_cap > (1 << 16))) op_bad(op, "lvl_cap: 0 (not kept) or >= 300");
    cand_check(op, n, cap, count, cand_anchor, A);
    need(cand_score, "cand_score");
    for (int b = 0; b < n; ++b)
      for (int i = 0; i < std::min(count[b], cap); ++i)
        if (!(cand_score[(size_t)b * cap + i] > 0.f)) op_bad(op, "scores must be positive (the select key is their bit pattern)");
    need(sel_count, "sel_count"); need(sel_score, "sel_score"); need(sel_anchor, "sel_anchor"); need(sel_cls, "sel_cls"); need(scores, "scores");
    need(score_anchor, "score_anchor");
    if (lvl_cap) { need(lvl_count, "lvl_count"); need(lvl_list, "lvl_list"); }
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    HeadSet hs;
    head_upload(hs, dtype, n, n_levels, lv, nc, true, false);
    hs.hp.conf = conf;
    hs.hp.class_mask[0] = hs.hp.class_mask[1] = ~0ull;
    const size_t m = (size_t)n * cap, sm = (size_t)n * sel_cap, scb = (size_t)n * gtx::kV10Keep * nc * 4,
                 lb = (size_t)n * gtx::kMaxLevels * (size_t)std::max(lvl_cap, 1) * 4;
    gtx::DevBuf dc, ds, da, qc, qs, qa, qk, dlc, dll, dsc, dka;
    fill_ff(dka, (size_t)n * gtx::kV10Keep * 4);
    upload(dc, count, (size_t)n * 4); upload(ds, cand_score, m * 4); upload(da, cand_anchor, m * 4);
    fill_ff(qc, (size_t)n * 4); fill_ff(qs, sm * 4); fill_ff(qa, sm * 4); fill_ff(qk, sm * 4); fill_ff(dsc, scb);
    gtx::NmsBuffers cand{}, sel{};
    cand.cap = cap;
    cand.count = dc.as<int>(); cand.cand_score = ds.as<float>(); cand.cand_anchor = da.as<int>();
    sel.cap = sel_cap;
    sel.count = qc.as<int>(); sel.cand_score = qs.as<float>(); sel.cand_anchor = qa.as<int>(); sel.cand_cls = qk.as<int>();
    if (lvl_cap) {
      fill_ff(dlc, (size_t)n * gtx::kMaxLevels * 4); fill_ff(dll, lb);
      sel.lvl_count = dlc.as<int>(); sel.lvl_list = dll.as<int>(); sel.lvl_cap = lvl_cap;
    }
    gtx::launch_v10_select(dtype, hs.hp, n, cand, sel, dsc.as<float>(), ctx->stream, dka.as<int>());
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(sel_count, qc, (size_t)n * 4); download(sel_score, qs, sm * 4); download(sel_anchor, qa, sm * 4); download(sel_cls, qk, sm * 4);
    download(scores, dsc, scb); download(score_anchor, dka, (size_t)n * gtx::kV10Keep * 4);
    if (lvl_cap) { download(lvl_count, dlc, (size_t)n * gtx::kMaxLevels * 4); download(lvl_list, dll, lb); }
  });
}

int gtx_op_v10_rows(gtx_ctx* ctx, int n, int sel_cap, const int* sel_count, const float* sel_score, const int* sel_anchor, const int* sel_cls,
                    const float* sel_box, uint64_t class_mask0, uint64_t class_mask1, int max_det, int src_h, int src_w, int net_h, int net_w,
                    double gain, float* out_rows, int* out_n, int* out_anchor) {
  return guarded([&] {
    const char* op = "v10_rows";
    if (n < 1 || n > 64 || sel_cap < 1 || sel_cap > 512 || max_det < 1 || max_det > (1 << 16)) op_bad(op, "sel_cap in [1, 512], max_det >= 1");
    geometry_check(op, src_h, src_w, net_h, net_w, gain);
    need(sel_count, "sel_count"); need(sel_score, "sel_score"); need(sel_anchor, "sel_anchor"); need(sel_cls, "sel_cls"); need(sel_box, "sel_box");
    need(out_rows, "out_rows"); need(out_n, "out_n"); need(out_anchor, "out_anchor");
    for (int b = 0; b < n; ++b)
      if (sel_count[b] < 0) op_bad(op, "a negative count");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t sm = (size_t)n * sel_cap, rows = (size_t)n * max_det;
    gtx::DevBuf qc, qs, qa, qk, qb, dn, dr, doa;
    upload(qc, sel_count, (size_t)n * 4); upload(qs, sel_score, sm * 4); upload(qa, sel_anchor, sm * 4); upload(qk, sel_cls, sm * 4);
    upload(qb, sel_box, sm * 16);
    upload(dn, out_n, (size_t)n * 4); upload(dr, out_rows, rows * 24); upload(doa, out_anchor, rows * 4);
    gtx::NmsBuffers sel{};
    sel.cap = sel_cap;
    sel.count = qc.as<int>(); sel.cand_score = qs.as<float>(); sel.cand_anchor = qa.as<int>(); sel.cand_cls = qk.as<int>(); sel.cand_box = qb.as<float>();
    sel.max_det = max_det;
    sel.out_n = dn.as<int>(); sel.out_rows = dr.as<float>(); sel.out_anchor = doa.as<int>();
    const unsigned long long mask[2] = {class_mask0, class_mask1};
    gtx::launch_v10_rows(sel, mask, n, geometry(src_h, src_w, net_h, net_w, gain), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(out_n, dn, (size_t)n * 4); download(out_rows, dr, rows * 24); download(out_anchor, doa, rows * 4);
  });
}

int gtx_op_obj_feats(gtx_ctx* ctx, int dtype, int n, int n_levels, const void* const* maps, const int* h, const int* w, const int* cstride,
                     const int* coff, const int* c, int dim, int max_det, const int* out_n, const int* out_anchor, float* out) {
  return guarded([&] {
    const char* op = "obj_feats";
    if (dtype != GTX_F16 && dtype != GTX_F32 && dtype != GTX_F32S) op_bad(op, "unsupported map format");
    if (n_levels > gtx::kMaxLevels) op_bad(op, "at most 4 levels");
    if (n < 1 || n > 64 || n_levels < 1 || dim < 1 || dim > (1 << 12) || max_det < 1 || max_det > (1 << 16)) op_bad(op, "bad sizes");
    need(maps, "maps"); need(h, "h"); need(w, "w"); need(cstride, "cstride"); need(coff, "coff"); need(c, "c");
    long A = 0;
    for (int l = 0; l < n_levels; ++l) {
      need(maps[l], "maps[l]");
      if (h[l] < 1 || w[l] < 1 || coff[l] < 0 || c[l] < 1 || cstride[l] > (1 << 16) || (long)coff[l] + c[l] > cstride[l]) op_bad(op, "a level's channel slice does not fit its stride");
      if (c[l] % dim) op_bad(op, "every level's channel count must be a multiple of dim");
      if (dtype == GTX_F32S && cstride[l] % 8) op_bad(op, "pair-format maps need channel strides that are multiples of 8");
      if ((double)n * h[l] * w[l] * cstride[l] > 2.5e8) op_bad(op, "maps too large");
      A += (long)h[l] * w[l];
    }
    if (A > (1l << 22)) op_bad(op, "too many anchors");
    cand_check(op, n, max_det, out_n, out_anchor, A);
    need(out, "out"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::FeatLevels fl{};
    gtx::DevBuf buf[gtx::kMaxLevels], dn, doa, dout;
    int anchor = 0;
    for (int l = 0; l < n_levels; ++l) {
      upload_fmt(buf[l], dtype, maps[l], (size_t)n * h[l] * w[l] * cstride[l] * gtx::dtype_size(dtype));
      fl.feat[l] = buf[l].p; fl.h[l] = h[l]; fl.w[l] = w[l]; fl.cstride[l] = cstride[l]; fl.coff[l] = coff[l]; fl.c[l] = c[l];
      fl.anchor_begin[l] = anchor;
      anchor += h[l] * w[l];
    }
    fl.n_levels = n_levels;
    fl.dim = dim;
    const size_t rows = (size_t)n * max_det;
    upload(dn, out_n, (size_t)n * 4); upload(doa, out_anchor, rows * 4); upload(dout, out, rows * dim * 4);
    gtx::NmsBuffers nb{};
    nb.max_det = max_det;
    nb.out_n = dn.as<int>(); nb.out_anchor = doa.as<int>();
    gtx::launch_obj_feats(dtype, fl, n, nb, dout.as<float>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(out, dout, rows * dim * 4);
  });
}

// ---- the sparse-optical-flow GMC's kernels one launcher at a time (tests/test_gmc_ops_gpu.py). Sizes, and every coordinate a
// kernel would turn into an address, are checked before anything touches the GPU.
int gtx_op_gmc_corners(gtx_ctx* ctx, const uint8_t* gray, int h, int w, int cap, int* n, float* xy, int counts[4]) {
  return guarded([&] {
    const char* op = "gmc_corners";
    if (h < 16 || w < 16 || h > 8192 || w > 8192) op_bad(op, "a gray image of 16..8192 pixels a side");
    if (cap < 1000) op_bad(op, "room for 1000 corners");
    need(gray, "gray"); need(n, "n"); need(xy, "xy"); need(counts, "counts"); need(ctx, "ctx");
    gtx::op_gmc_corners(ctx, gray, h, w, n, xy, counts);
  });
}

int gtx_op_gmc_lk(gtx_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int h, int w, const float* pts, int n, float* next, int* status) {
  return guarded([&] {
    const char* op = "gmc_lk";
    if (h < 16 || w < 16 || h > 8192 || w > 8192) op_bad(op, "gray images of 16..8192 pixels a side (every pyramid level at least two wide)");
    if (n < 0 || n > 1000) op_bad(op, "0 <= n <= 1000 points");
    need(prev, "prev"); need(cur, "cur");
    if (n > 0) { need(pts, "pts"); need(next, "next"); need(status, "status"); }
    for (int i = 0; i < n; ++i) {
      const float x = pts[2 * i], y = pts[2 * i + 1];
      if (!(x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1))) op_bad(op, "a point outside the image (or not a number)");
    }
    need(ctx, "ctx");
    gtx::op_gmc_lk(ctx, prev, cur, h, w, pts, n, next, status);
  });
}

int gtx_op_gmc_ransac(gtx_ctx* ctx, const float* pairs, int n, uint32_t seed, int* best_count, int* winner, double model[4], int* count) {
  return guarded([&] {
    const char* op = "gmc_ransac";
    if (n < 0 || n > 1024) op_bad(op, "0 <= n <= 1024 pairs (the compaction step's list)");
    if (n > 0) need(pairs, "pairs");
    for (int i = 0; i < 4 * n; ++i)
      if (!std::isfinite(pairs[i])) op_bad(op, "a coordinate that is not a finite number");
    need(best_count, "best_count"); need(winner, "winner"); need(model, "model"); need(count, "count"); need(ctx, "ctx");
    gtx::op_gmc_ransac(ctx, pairs, n, seed, best_count, winner, model, count);
  });
}

// ---- GMC method ecc: the prepare kernel, and the gradient kernel with one round of the fit's four launches (tests/test_ecc_ops_gpu.py).
// Sizes, the map and the state a kernel branches on are checked before anything touches the GPU.
int gtx_op_ecc_prepare(gtx_ctx* ctx, const uint8_t* frame_bgr, int H, int W, float* out) {
  return guarded([&] {
    const char* op = "ecc_prepare";
    if (H < 8 || W < 8 || H > 16384 || W > 16384) op_bad(op, "a frame of 8..16384 pixels a side");
    need(frame_bgr, "frame_bgr"); need(out, "out"); need(ctx, "ctx");
    gtx::op_ecc_prepare(ctx, frame_bgr, H, W, out);
  });
}

int gtx_op_ecc_iterate(gtx_ctx* ctx, const float* tmpl, const float* img, int h, int w, const float map[6], int exact, double rho_in,
                       double last_rho_in, double eps, int iter_in, int max_iters, int status_in, int done_in, float* gx, float* gy,
                       double* partial_stats, double* partial_accum, float map_out[6], int state_i[3], double state_d[5], float means[2]) {
  return guarded([&] {
    const char* op = "ecc_iterate";
    if (h < 2 || w < 2 || h > 8192 || w > 8192) op_bad(op, "images of 2..8192 pixels a side (REFLECT_101 needs two)");
    need(map, "map");
    for (int k = 0; k < 6; ++k)
      if (!(std::fabs(map[k]) <= 1e6f)) op_bad(op, "a map entry that is not a number, or beyond 1e6");
    if (exact != 0 && exact != 1) op_bad(op, "exact is 0 or 1");
    if (!(eps > 0.0)) op_bad(op, "eps > 0");
    if (max_iters < 1 || iter_in < 0 || iter_in >= max_iters) op_bad(op, "0 <= iter_in < max_iters");
    if (status_in < 0 || status_in > 2 || (done_in != 0 && done_in != 1)) op_bad(op, "status_in 0..2, done_in 0 or 1");
    need(tmpl, "tmpl"); need(img, "img"); need(gx, "gx"); need(gy, "gy"); need(partial_stats, "partial_stats"); need(partial_accum, "partial_accum");
    need(map_out, "map_out"); need(state_i, "state_i"); need(state_d, "state_d"); need(means, "means"); need(ctx, "ctx");
    gtx::EccOpState st{};
    for (int k = 0; k < 6; ++k) st.map[k] = map[k];
    st.iter = iter_in; st.status = status_in; st.done = done_in; st.rho = rho_in; st.last_rho = last_rho_in;
    gtx::op_ecc_iterate(ctx, tmpl, img, h, w, exact != 0, eps, max_iters, &st, gx, gy, partial_stats, partial_accum);
    for (int k = 0; k < 6; ++k) map_out[k] = st.map[k];
    state_i[0] = st.iter; state_i[1] = st.status; state_i[2] = st.done;
    state_d[0] = st.rho; state_d[1] = st.last_rho; state_d[2] = st.n; state_d[3] = st.img_norm; state_d[4] = st.tmp_norm;
    means[0] = st.img_mean; means[1] = st.tmp_mean;
  });
}

// ---- the stabilizer's matcher and RANSAC kernel, one launch each (tests/test_orb_ops_gpu.py). As for the hooks above: sizes are
// checked before anything touches the GPU.
int gtx_op_orb_match(gtx_ctx* ctx, const uint8_t* desc_q, int nq, int slots_q, const uint8_t* desc_t, int nt, int slots_t, float ratio, int keep_all,
                     const float* xy_q, const float* xy_t, int* best_idx, int* best_d, int* second_d, int* m_q, int* m_t, int* m_d, float* m_pts,
                     int* n_match) {
  return guarded([&] {
    const char* op = "orb_match";
    if (nq < 1 || nt < 0 || slots_q < nq || slots_t < std::max(nt, 1) || slots_q > (1 << 16) || slots_t > (1 << 20)) op_bad(op, "1 <= nq <= slots_q <= 65536, 0 <= nt <= slots_t <= 2^20, slots_t >= 1");
    if ((double)gtx::cdiv(slots_t, 256) * slots_q > 6.4e7) op_bad(op, "the per-chunk partials would pass 768 MB");
    if (!(ratio >= 0.f && ratio <= 4.f)) op_bad(op, "ratio in [0, 4]");
    need(desc_q, "desc_q"); need(xy_q, "xy_q");
    if (nt > 0) { need(desc_t, "desc_t"); need(xy_t, "xy_t"); }
    need(best_idx, "best_idx"); need(best_d, "best_d"); need(second_d, "second_d"); need(m_q, "m_q"); need(m_t, "m_t"); need(m_d, "m_d");
    need(m_pts, "m_pts"); need(n_match, "n_match"); need(ctx, "ctx");
    gtx::op_orb_match(ctx, desc_q, nq, slots_q, desc_t, nt, slots_t, ratio, keep_all != 0, xy_q, xy_t, best_idx, best_d, second_d, m_q, m_t, m_d, m_pts,
                      n_match);
  });
}

// ---- the stabilizer's working-resolution gray image (tests/test_stab_ratio_gpu.py; the engine's "frame" route calls the _dev entry
// per frame). One check for both entries: the frame, the ratio and the working size the caller believes in.
static void gray_resize_check(const char* op, int h, int w, float ratio, int gh, int gw) {
  if (h < 1 || w < 1 || h > 0xffff || w > 0xffff) op_bad(op, "frames of 1..65535 pixels a side");
  if (!(ratio > 0.f && ratio <= 1.f)) op_bad(op, "downsample_ratio must be in (0, 1]");
  int eh = 0, ew = 0;
  gtx::gray_working_size(h, w, ratio, &eh, &ew);
  if (eh < 1 || ew < 1) op_bad(op, "the working image would be empty");
  if (gh != eh || gw != ew) gtx::fail(GTX_ERR_INVALID, "%s: gray image is %dx%d, the working size of a %dx%d frame at ratio %g is %dx%d", op, gw, gh, w, h, ratio, ew, eh);
}

int gtx_op_gray_working_size(int h, int w, float ratio, int* gh, int* gw) {
  return guarded([&] {
    const char* op = "gray_working_size";
    need(gh, "gh"); need(gw, "gw");
    if (h < 1 || w < 1 || h > 0xffff || w > 0xffff) op_bad(op, "frames of 1..65535 pixels a side");
    if (!(ratio > 0.f && ratio <= 1.f)) op_bad(op, "downsample_ratio must be in (0, 1]");
    gtx::gray_working_size(h, w, ratio, gh, gw);
  });
}

int gtx_op_gray_resize_dev(gtx_ctx* ctx, const void* bgr_dptr, int h, int w, float ratio, void* gray_dptr, int gh, int gw) {
  return guarded([&] {
    gray_resize_check("gray_resize_dev", h, w, ratio, gh, gw);
    need(bgr_dptr, "bgr"); need(gray_dptr, "gray"); need(ctx, "ctx");
    gtx::gray_resize_dev(ctx, bgr_dptr, h, w, ratio, gray_dptr);
  });
}

int gtx_op_gray_resize_ms(gtx_ctx* ctx, const void* bgr_dptr, int h, int w, float ratio, void* gray_dptr, int gh, int gw, int reps, float* ms) {
  return guarded([&] {
    const char* op = "gray_resize_ms";
    gray_resize_check(op, h, w, ratio, gh, gw);
    if (reps < 1 || reps > 100000) op_bad(op, "1..100000 repetitions");
    need(bgr_dptr, "bgr"); need(gray_dptr, "gray"); need(ms, "ms"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    *ms = time_launches(ctx->stream, reps, [&] { gtx::gray_resize_dev(ctx, bgr_dptr, h, w, ratio, gray_dptr); });
  });
}

int gtx_op_gray_resize(gtx_ctx* ctx, const uint8_t* bgr, int h, int w, float ratio, uint8_t* gray, int gh, int gw) {
  return guarded([&] {
    gray_resize_check("gray_resize", h, w, ratio, gh, gw);
    need(bgr, "bgr"); need(gray, "gray"); need(ctx, "ctx");
    gtx::op_gray_resize(ctx, bgr, h, w, ratio, gray);
  });
}

int gtx_op_orb_ransac(gtx_ctx* ctx, const float* pts, int n, uint32_t seed, int n_hyp, int frame_w, int frame_h, float thr, int affine, int* best,
                      int64_t* cost, double H[9]) {
  return guarded([&] {
    const char* op = "orb_ransac";
    if (n < 0 || n > (1 << 20)) op_bad(op, "0 <= n <= 2^20 point pairs");
    if (n_hyp < 1 || n_hyp > 65536) op_bad(op, "1..65536 hypotheses (the winner's index has 16 bits of the key)");
    if (frame_w < 1 || frame_h < 1 || frame_w > (1 << 16) || frame_h > (1 << 16)) op_bad(op, "bad frame size");
    if (!(thr > 0.f && thr <= 64.f)) op_bad(op, "threshold in (0, 64] px (a match costs at most thr^2 * 1024, the sum has 47 bits)");
    if (affine != 0 && affine != 1) op_bad(op, "affine is 0 or 1");
    if (n > 0) need(pts, "pts");
    need(best, "best"); need(cost, "cost"); need(H, "H"); need(ctx, "ctx");
    long long c = 0;
    gtx::op_orb_ransac(ctx, pts, n, seed, n_hyp, frame_w, frame_h, thr, affine, best, &c, H);
    *cost = c;
  });
}

// ---- the SIFT kernels one stage at a time (tests/test_sift_ops_gpu.py). Sizes, and every record field a kernel turns into an address
// or a loop bound, are checked before anything touches the GPU.
namespace {
void sift_image_ok(const char* op, int h, int w, int octave) {
  if (h < 1 || w < 1 || h > 4096 || w > 4096) op_bad(op, "images of 1..4096 pixels a side");
  if (octave < 0 || octave > 15) op_bad(op, "octave 0..15");
}
}  // namespace

int gtx_op_sift_blur(gtx_ctx* ctx, const float* src, int h, int w, double sigma, int form, float* dst, float* dog) {
  return guarded([&] {
    const char* op = "sift_blur";
    sift_image_ok(op, h, w, 0);
    if (!(sigma > 0.0 && sigma <= 64.0)) op_bad(op, "sigma in (0, 64]");
    if (form < 0 || form > 2) op_bad(op, "form: 0 the pyramid's dispatch, 1 the generic tile kernel, 2 the row / column / subtraction passes");
    (void)gtx::sift_blur_radius(sigma);                    // a radius above 16 is refused here, before any launch
    need(src, "src"); need(dst, "dst"); need(ctx, "ctx");
    gtx::op_sift_blur(ctx, src, h, w, sigma, form, dst, dog);
  });
}

int gtx_op_sift_extrema(gtx_ctx* ctx, const float* dog5, int h, int w, int octave, int cap, int* count, int* cand) {
  return guarded([&] {
    const char* op = "sift_extrema";
    sift_image_ok(op, h, w, octave);
    if (cap < 1 || cap > (1 << 24)) op_bad(op, "cap in [1, 2^24]");
    need(dog5, "dog5"); need(count, "count"); need(cand, "cand"); need(ctx, "ctx");
    gtx::op_sift_extrema(ctx, dog5, h, w, octave, cap, count, cand);
  });
}

int gtx_op_sift_refine(gtx_ctx* ctx, const float* dog5, int h, int w, int octave, const int* cand, int n, int* count, void* out) {
  return guarded([&] {
    const char* op = "sift_refine";
    sift_image_ok(op, h, w, octave);
    if (n < 0 || n > (1 << 24)) op_bad(op, "0 <= n <= 2^24 candidates");
    need(dog5, "dog5"); need(count, "count");
    if (n > 0) { need(cand, "cand"); need(out, "out"); }
    for (int i = 0; i < n; ++i) {
      const int* c = cand + 4 * (size_t)i;
      if (c[0] != octave) op_bad(op, "a candidate of another octave");
      if (c[1] < 1 || c[1] > 3 || c[2] < 5 || c[2] >= h - 5 || c[3] < 5 || c[3] >= w - 5) op_bad(op, "a candidate outside layers 1..3 or inside the border of 5");
    }
    need(ctx, "ctx");
    gtx::op_sift_refine(ctx, dog5, h, w, octave, cand, n, count, out);
  });
}

int gtx_op_sift_orient(gtx_ctx* ctx, const float* gauss_layer, int h, int w, int octave, const void* refined, int n, int cap, int* count, void* out,
                       float* hist) {
  return guarded([&] {
    const char* op = "sift_orient";
    sift_image_ok(op, h, w, octave);
    if (n < 0 || n > (1 << 20)) op_bad(op, "0 <= n <= 2^20 keypoints");
    if (cap < 1 || cap > (1 << 24)) op_bad(op, "cap in [1, 2^24]");
    need(gauss_layer, "gauss_layer"); need(count, "count"); need(out, "out");
    if (n > 0) { need(refined, "refined"); need(hist, "hist"); }
    for (int i = 0; i < n; ++i) {
      float f[4];
      int k[5];
      std::memcpy(f, static_cast<const char*>(refined) + 52 * (size_t)i, sizeof f);
      std::memcpy(k, static_cast<const char*>(refined) + 52 * (size_t)i + 16, sizeof k);
      if (k[1] != octave) op_bad(op, "a keypoint of another octave");
      if (k[2] < 0 || k[2] > 5 || k[3] < 0 || k[3] >= h || k[4] < 0 || k[4] >= w) op_bad(op, "a keypoint outside layers 0..5 or outside the image");
      // the window's radius is rint(4.5 * size / 2 / 2^octave) pixels; the kernel walks (2 radius + 1)^2 of them
      if (!(f[2] > 0.f && 4.5 * 0.5 * (double)f[2] / (double)(1 << octave) <= 2048.0)) op_bad(op, "a keypoint size that is not positive, or a window radius above 2048");
    }
    need(ctx, "ctx");
    gtx::op_sift_orient(ctx, gauss_layer, h, w, octave, refined, n, cap, count, out, hist);
  });
}

int gtx_op_sift_describe(gtx_ctx* ctx, const float* gauss_layer, int h, int w, const void* finals, int n, int root, float root_eps, float* desc) {
  return guarded([&] {
    const char* op = "sift_describe";
    sift_image_ok(op, h, w, 0);
    if (n < 0 || n > (1 << 20)) op_bad(op, "0 <= n <= 2^20 keypoints");
    if (root != 0 && root != 1) op_bad(op, "root is 0 or 1");
    need(gauss_layer, "gauss_layer");
    if (n > 0) { need(finals, "finals"); need(desc, "desc"); }
    for (int i = 0; i < n; ++i) {
      double ori;
      float f[3];
      int k[2];
      const char* rec = static_cast<const char*>(finals) + 32 * (size_t)i;
      std::memcpy(&ori, rec, sizeof ori);
      std::memcpy(f, rec + 8, sizeof f);
      std::memcpy(k, rec + 20, sizeof k);
      if (k[0] != 0 || k[1] < 0 || k[1] > 5) op_bad(op, "records name octave 0 and a layer 0..5 (the one image given)");
      if (!(ori >= 0.0 && ori <= 360.0)) op_bad(op, "ori in [0, 360] degrees");
      if (!(std::fabs(f[0]) <= 1e6f && std::fabs(f[1]) <= 1e6f)) op_bad(op, "a position that is not a number, or beyond 1e6 pixels");
      if (!(f[2] > 0.f && f[2] <= 1e6f)) op_bad(op, "scl in (0, 1e6] (the window's radius is clamped by the image diagonal)");
    }
    need(ctx, "ctx");
    gtx::op_sift_describe(ctx, gauss_layer, h, w, finals, n, root, root_eps, desc);
  });
}

int gtx_op_sift_select(gtx_ctx* ctx, const void* oriented, int n, int max_features, const int* rects, int n_rects, int* count, void* finals,
                       float* xy, float* kp5, int* octave) {
  return guarded([&] {
    const char* op = "sift_select";
    if (n < 0 || n > (1 << 20)) op_bad(op, "0 <= n <= 2^20 records");
    if (max_features < 1 || max_features > gtx::sift_select_max_features()) op_bad(op, "max_features in [1, 65536]");
    if (n_rects < 0 || n_rects > gtx::sift_select_max_rects()) op_bad(op, "0 <= n_rects <= 1024 rectangles");
    need(count, "count");
    if (n > 0) need(oriented, "oriented");
    if (n_rects > 0) need(rects, "rects");
    std::vector<uint64_t> keys((size_t)n);
    for (int i = 0; i < n; ++i) {
      float f[5];
      int k[8];
      std::memcpy(f, static_cast<const char*>(oriented) + 52 * (size_t)i, sizeof f);
      std::memcpy(k, static_cast<const char*>(oriented) + 52 * (size_t)i + 20, sizeof k);     // word, o, layer, key (o, layer, r, c), bin
      if (!(std::isfinite(f[4]) && f[4] >= 0.f)) op_bad(op, "a response that is not finite, or negative");
      if (k[1] < 0 || k[1] > 15 || k[3] < 0 || k[3] > 15) op_bad(op, "an octave outside 0..15");
      if (k[4] < 0 || k[4] > 7) op_bad(op, "a key layer outside 0..7");
      if (k[5] < 0 || k[5] >= (1 << 20) || k[6] < 0 || k[6] >= (1 << 20)) op_bad(op, "a key row or column outside [0, 2^20)");
      if (k[7] < 0 || k[7] > 255) op_bad(op, "an orientation bin outside 0..255");
      keys[(size_t)i] = ((uint64_t)k[3] << 56) | ((uint64_t)k[4] << 48) | ((uint64_t)k[5] << 28) | ((uint64_t)k[6] << 8) | (uint64_t)k[7];
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) op_bad(op, "two records with one key (octave, layer, row, column, bin)");
    need(ctx, "ctx");
    gtx::op_sift_select(ctx, oriented, n, max_features, rects, n_rects, count, finals, xy, kp5, octave);
  });
}

// ---- single routines on host arrays: the registration matcher, the detector's preprocess pass, the trackers' assignment solver,
// the host-side affine fit, the georeference chain and CLAHE
int gtx_op_match_2nn(gtx_ctx* ctx, const float* query, int nq, const float* train, int nt, int* idx1, int* idx2, float* d1,
                     float* d2, int iters, float* ms_per_pass) {
  return guarded([&] {
    need(ctx, "ctx"); need(query, "query"); need(train, "train"); need(idx1, "idx1"); need(idx2, "idx2"); need(d1, "d1"); need(d2, "d2");
    if (nq < 0 || nt < 0) gtx::fail(GTX_ERR_INVALID, "negative descriptor count");
    GTX_HIP(hipSetDevice(ctx->device));
    if (nq == 0) return;
    hipStream_t s = ctx->stream;
    const size_t qn = (size_t)nq * 128, tn = (size_t)std::max(nt, 1) * 128;
    gtx::DevBuf qf, tf, qh(qn * 2), th(tn * 2), ws(gtx::match2nn_workspace_bytes(nq, nt));
    gtx::DevBuf i1(nq * 4), i2(nq * 4), e1(nq * 4), e2(nq * 4);
    upload(qf, query, qn * 4);
    upload(tf, train, (size_t)nt * 128 * 4, tn * 4);
    gtx::descriptors_to_half(qf.as<float>(), qh.p, qn, s);
    gtx::descriptors_to_half(tf.as<float>(), th.p, (size_t)nt * 128, s);
    auto once = [&] {
      gtx::match2nn(qh.p, qf.as<float>(), nq, th.p, tf.as<float>(), nt, ws.p, i1.as<int>(), i2.as<int>(), e1.as<float>(), e2.as<float>(), s);
    };
    once();
    GTX_HIP(hipStreamSynchronize(s));
    if (iters > 0 && ms_per_pass) *ms_per_pass = time_launches(s, iters, once);
    download(idx1, i1, nq * 4); download(idx2, i2, nq * 4); download(d1, e1, nq * 4); download(d2, e2, nq * 4);
  });
}

int gtx_op_preprocess(gtx_ctx* ctx, int dtype, const uint8_t* frame, int h, int w, int net_h, int net_w,
                      void* out_img, uint8_t* out_gray, int gray_h, int gray_w) {
  return guarded([&] {
    need(ctx, "ctx"); need(frame, "frame"); need(out_img, "out_img");
    GTX_HIP(hipSetDevice(ctx->device));
    // Letterbox of the frame into exactly net_h x net_w (ultralytics geometry for that target).
    gtx::Letterbox lb{};
    lb.src_h = h; lb.src_w = w; lb.net_h = net_h; lb.net_w = net_w;
    const double r = std::min((double)net_h / h, (double)net_w / w);
    lb.new_w = (int)std::nearbyint(w * r);
    lb.new_h = (int)std::nearbyint(h * r);
    lb.top = (int)std::nearbyint((net_h - lb.new_h) / 2.0 - 0.1);
    lb.left = (int)std::nearbyint((net_w - lb.new_w) / 2.0 - 0.1);
    lb.gain = r;
    const size_t fb = (size_t)h * w * 3, npx = (size_t)net_h * net_w, ib = npx * 4;   // device image: RGB0 bytes
    gtx::DevBuf df, di(ib), dg;
    if (out_gray) dg.alloc((size_t)gray_h * gray_w);
    upload(df, frame, fb);
    gtx::launch_preprocess(dtype, df.as<uint8_t>(), 1, lb, di.p, out_gray ? dg.as<uint8_t>() : nullptr, gray_h, gray_w, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    // The network's view of the image (what the stem kernels make of the bytes through their tables): byte / 255 in fp32,
    // rounded to fp16 for dtype f16.
    std::vector<uint8_t> raw(ib);
    download(raw.data(), di, ib);
    for (size_t i = 0; i < npx * 4; ++i) {
      const float f = (float)raw[i] / 255.f;
      if (dtype == gtx::DT_F16) static_cast<_Float16*>(out_img)[i] = (_Float16)f;
      else static_cast<float*>(out_img)[i] = f;
    }
    if (out_gray) download(out_gray, dg, (size_t)gray_h * gray_w);
  });
}

int gtx_op_linear_assignment(const float* cost, int rows, int cols, double cost_limit, int* row_to_col, int* col_to_row) {
  return guarded([&] {
    if (rows < 0 || cols < 0) gtx::fail(GTX_ERR_INVALID, "linear assignment: negative size");
    if (rows > 0 && cols > 0) need(cost, "cost");
    if (rows > 0) need(row_to_col, "row_to_col");
    for (size_t i = 0; i < (size_t)rows * cols; ++i)
      if (!std::isfinite(cost[i])) gtx::fail(GTX_ERR_INVALID, "linear assignment: cost %zu is not finite", i);
    std::vector<int> x, y;
    if (cost_limit > 0 && std::isfinite(cost_limit)) {
      gtx::lap_limited(cost, rows, cols, cost_limit, x, y);
    } else {
      std::vector<double> c((size_t)rows * cols);
      for (size_t i = 0; i < c.size(); ++i) c[i] = cost[i];
      gtx::lap_full(c, rows, cols, x);
      y.assign(cols, -1);
      for (int r = 0; r < rows; ++r)
        if (x[r] >= 0) y[x[r]] = r;
    }
    for (int r = 0; r < rows; ++r) row_to_col[r] = x[r];
    if (col_to_row)
      for (int c = 0; c < cols; ++c) col_to_row[c] = y[c];
  });
}

int gtx_op_estimate_affine_partial(const float* p_xy, const float* q_xy, int n, unsigned seed, double A[6], int* valid, int* n_inliers) {
  return guarded([&] {
    need(A, "A"); need(valid, "valid");
    if (n > 0) { need(p_xy, "p_xy"); need(q_xy, "q_xy"); }
    if (n < 0) gtx::fail(GTX_ERR_INVALID, "estimate_affine_partial: n = %d", n);
    *valid = gtx::estimate_affine_partial(p_xy, q_xy, n, seed, A, n_inliers) ? 1 : 0;
  });
}

int gtx_op_homography_refit(const float* pairs, int n, int frame_w, int frame_h, double thr, int affine, const double H0[9], double H[9],
                            int* valid, int* n_inliers) {
  return guarded([&] {
    need(H0, "H0"); need(H, "H"); need(valid, "valid"); need(n_inliers, "n_inliers");
    if (n > 0) need(pairs, "pairs");
    if (n < 0) gtx::fail(GTX_ERR_INVALID, "homography_refit: n = %d", n);
    if (frame_w < 1 || frame_h < 1) gtx::fail(GTX_ERR_INVALID, "homography_refit: frame %d x %d", frame_w, frame_h);
    *n_inliers = 0;
    *valid = gtx::refine_homography(pairs, n, frame_w, frame_h, thr, affine != 0, H0, H, n_inliers) ? 1 : 0;
  });
}

// The inverse gtx_warp_frame[_dev] hands its kernel (tests/test_warp_ops_gpu.py feeds the oracle the same matrix). Host only.
int gtx_op_invert3x3(const double H[9], double inv[9]) {
  return guarded([&] {
    need(H, "H"); need(inv, "inv");
    if (!gtx::invert3x3(H, inv)) gtx::fail(GTX_ERR_INVALID, "invert3x3: the matrix is singular or not finite");
  });
}

int gtx_op_georef_points(gtx_ctx* ctx, const gtx_georef_chain* chain, const double* x, const double* y, int n,
                         double* ortho_x, double* ortho_y, double* lat, double* lon, double* east, double* north) {
  return guarded([&] {
    need(ctx, "ctx"); need(chain, "chain");
    if (n > 0) { need(x, "x"); need(y, "y"); }
    gtx::georef_points(ctx, *chain, x, y, n, ortho_x, ortho_y, lat, lon, east, north);
  });
}

// The georeference stage's per-track columns (tests/test_georef_tracks_gpu.py). Everything that decides an address is checked here:
// the plan against n (a permutation, bounds that tile it, counts and offsets that fit); what the plan says about the table's
// values (which rows are used, how long a gap-filled series is) the kernels count again themselves (georef.hip).
int gtx_op_georef_tracks(gtx_ctx* ctx, const gtx_georef_chain* chain, const gtx_georef_tracks_cfg* cfg, const double* x, const double* y,
                         const double* bbox_unstab, const double* veh_dim_px, const int32_t* frame_num, const int32_t* is_interpolated, int n,
                         const int32_t* order, const int32_t* seg, const int32_t* n_used, const int64_t* exp_off, const double* quads,
                         int n_quads, const double* weights, int n_weights, double* ortho_x, double* ortho_y, double* lat, double* lon,
                         double* east, double* north, uint8_t* visibility, double* length_m, double* width_m, double* speed, double* accel,
                         int32_t* quad) {
  return guarded([&] {
    const char* op = "georef_tracks";
    need(chain, "chain"); need(cfg, "cfg");
    if (n < 0) gtx::fail(GTX_ERR_INVALID, "georef_tracks: n = %d", n);
    if (n_weights < 1 || n_weights % 2 == 0 || n_weights > 4095)
      gtx::fail(GTX_ERR_INVALID, "georef_tracks: %d weights: an odd count of at most 4095 is needed (a centre tap and a radius)", n_weights);
    need(weights, "weights");
    for (int k = 0; k < n_weights; ++k)
      if (!std::isfinite(weights[k])) op_bad(op, "a weight is not finite");
    if (n_quads < 0 || n_quads > 512) gtx::fail(GTX_ERR_INVALID, "georef_tracks: %d quads: 0 .. 512 fit the lane kernel's LDS", n_quads);
    if (n_quads > 0) need(quads, "quads");
    if (cfg->boundary != 0 && cfg->boundary != 1) op_bad(op, "boundary must be 0 (reflect) or 1 (nearest)");
    if (cfg->frame_h <= 0 || cfg->frame_w <= 0 || cfg->visibility_margin < 0) op_bad(op, "frame size / visibility margin");
    if (!std::isfinite(cfg->fps) || !std::isfinite(cfg->conversion_factor)) op_bad(op, "fps / conversion_factor is not finite");
    if (!chain->projected) op_bad(op, "the chain must end in a projected system (dimensions and kinematics are in metres)");
    const int T = cfg->n_tracks;
    if (T < 0 || T > n || (n > 0 && T == 0)) gtx::fail(GTX_ERR_INVALID, "georef_tracks: plan: %d tracks for %d rows", T, n);
    std::vector<int32_t> eoff;
    if (n > 0) {
      need(x, "x"); need(y, "y"); need(bbox_unstab, "bbox_unstab"); need(veh_dim_px, "veh_dim_px"); need(frame_num, "frame_num");
      need(order, "order"); need(seg, "seg"); need(n_used, "n_used"); need(exp_off, "exp_off");
      std::vector<bool> seen((size_t)n, false);
      for (int i = 0; i < n; ++i) {
        if (order[i] < 0 || order[i] >= n || seen[(size_t)order[i]]) gtx::fail(GTX_ERR_INVALID, "georef_tracks: plan: order is not a permutation of the %d rows (entry %d)", n, i);
        seen[(size_t)order[i]] = true;
      }
      if (seg[0] != 0 || seg[T] != n) gtx::fail(GTX_ERR_INVALID, "georef_tracks: plan: seg runs %d .. %d, the table has %d rows", seg[0], seg[T], n);
      if (exp_off[0] != 0) op_bad(op, "plan: exp_off[0] must be 0");
      eoff.resize((size_t)T + 1);
      eoff[0] = 0;
      for (int t = 0; t < T; ++t) {
        const int rows = seg[t + 1] - seg[t];
        if (rows < 1 || seg[t + 1] > n) gtx::fail(GTX_ERR_INVALID, "georef_tracks: plan: track %d has the bounds %d .. %d", t, seg[t], seg[t + 1]);
        if (n_used[t] < 0 || n_used[t] > rows) gtx::fail(GTX_ERR_INVALID, "georef_tracks: plan: track %d uses %d of %d rows", t, n_used[t], rows);
        const int64_t len = exp_off[t + 1] - exp_off[t];
        if (n_used[t] < 3 ? len != 0 : len < n_used[t])
          gtx::fail(GTX_ERR_INVALID, "georef_tracks: plan: track %d with %d used rows has a series of %lld points", t, n_used[t], (long long)len);
        if (exp_off[t + 1] > (int64_t)1 << 30) op_bad(op, "plan: more than 2^30 points in the gap-filled series");
        eoff[(size_t)t + 1] = (int32_t)exp_off[t + 1];
      }
    }
    need(ctx, "ctx");
    gtx::GeorefTracksArgs a{};
    a.x = x; a.y = y; a.bbox = bbox_unstab; a.dims = veh_dim_px; a.frame = frame_num; a.interp = is_interpolated;
    a.order = order; a.seg = seg; a.n_used = n_used; a.exp_off = eoff.data();
    a.quads = quads; a.weights = weights; a.n = n; a.n_quads = n_quads; a.n_weights = n_weights;
    a.symmetric = 1;                                              // scipy.ndimage.correlate1d's test: |w[r + k] - w[r - k]| <= DBL_EPSILON
    for (int k = 1; k <= n_weights / 2; ++k)
      if (std::fabs(weights[n_weights / 2 + k] - weights[n_weights / 2 - k]) > 2.220446049250313e-16) { a.symmetric = 0; break; }
    a.ox = ortho_x; a.oy = ortho_y; a.lat = lat; a.lon = lon; a.east = east; a.north = north;
    a.vis = visibility; a.length_m = length_m; a.width_m = width_m; a.speed = speed; a.accel = accel; a.quad = quad;
    gtx::georef_tracks(ctx, *chain, *cfg, a);
  });
}

int gtx_georef_tracks_ms(float ms[GTX_GEOREF_TRACKS_MS]) {
  return guarded([&] {
    need(ms, "ms");
    gtx::georef_tracks_last_ms(ms);
  });
}

int gtx_op_clahe(gtx_ctx* ctx, const uint8_t* gray, int h, int w, uint8_t* out) {
  return guarded([&] {
    need(ctx, "ctx"); need(gray, "gray"); need(out, "out");
    gtx::clahe_image(ctx, gray, h, w, out);
  });
}

// ---- the JPEG encoder's chain on a host frame (tests/test_jpeg_encode_gpu.py)

int gtx_op_jpeg_encode(gtx_ctx* ctx, const uint8_t* bgr, int h, int w, int quality, int subsampling, void* record, size_t capacity, size_t* bytes) {
  bool fits = true;
  const int st = guarded([&] {
    gtx::JpegEncoder::check_args(h, w, quality, subsampling);
    need(bgr, "bgr"); need(bytes, "bytes");
    if (!record && capacity) op_bad("jpeg_encode", "record is NULL with a capacity");
    if (record && (reinterpret_cast<uintptr_t>(record) & 3)) op_bad("jpeg_encode", "the record buffer is not 4-byte aligned");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf d_bgr;
    upload(d_bgr, bgr, (size_t)h * w * 3);
    gtx::JpegEncoder enc(ctx, h, w, quality, subsampling);
    enc.submit(d_bgr.p);
    fits = enc.collect(record, capacity, bytes);
    if (!fits) {                                                  // the caller asks again with *bytes; nothing stays in flight here
      std::vector<uint32_t> tmp((*bytes + 3) / 4);
      (void)enc.collect(tmp.data(), tmp.size() * 4, bytes);
    }
  });
  return st != GTX_OK ? st : fits ? 0 : 1;
}

// ---- the GPU entropy coder on a host record (tests/test_jpeg_huff_ops_gpu.py)

int gtx_op_jpeg_huff(gtx_ctx* ctx, const void* record, size_t bytes, void* out, size_t capacity, size_t* n, uint32_t* block_bits) {
  bool fits = true;
  const int st = guarded([&] {
    need(record, "record"); need(n, "n");
    *n = 0;
    if (!out && capacity) op_bad("jpeg_huff", "out is NULL with a capacity");
    if (reinterpret_cast<uintptr_t>(record) & 3) op_bad("jpeg_huff", "the record is not 4-byte aligned");
    if (bytes < sizeof(gtx::jpeg::RecordHeader)) gtx::fail(GTX_ERR_INVALID, "JPEG record: too short or misaligned");
    gtx::jpeg::RecordHeader hd;
    memcpy(&hd, record, sizeof hd);
    if (hd.width > (uint32_t)gtx::jpeg::kMaxDim || hd.height > (uint32_t)gtx::jpeg::kMaxDim) gtx::fail(GTX_ERR_INVALID, "JPEG record: its frame size differs from h x w");
    char msg[256];
    if (gtx::jpeg::check_record(record, bytes, (int)hd.height, (int)hd.width, msg, sizeof msg) != 0) gtx::fail(GTX_ERR_INVALID, "%s", msg);
    const uint8_t* rec = static_cast<const uint8_t*>(record);
    const uint16_t* quant = reinterpret_cast<const uint16_t*>(rec + gtx::jpeg::kQuantOffset);
    for (uint32_t i = 0; i < 64 * hd.ncomp; ++i)
      if (quant[i] > 255) gtx::fail(GTX_ERR_INVALID, "JPEG record: a quantiser above 255 (baseline tables have 8-bit entries)");
    need(ctx, "ctx");
    // the record expanded to what jpeg_fdct_kernel leaves behind: dense runs [n_blocks][64] (zeros past a block's length) + lengths
    const uint32_t* off = reinterpret_cast<const uint32_t*>(rec + gtx::jpeg::kOffsetsOffset);
    const int16_t* coef = reinterpret_cast<const int16_t*>(rec + gtx::jpeg::kOffsetsOffset + 4 * ((size_t)hd.n_blocks + 1));
    std::vector<int16_t> dense((size_t)hd.n_blocks * 64, 0);
    std::vector<uint32_t> lens(hd.n_blocks);
    for (uint32_t b = 0; b < hd.n_blocks; ++b) {
      lens[b] = off[b + 1] - off[b];                              // 0..64, inside the stream: check_record
      memcpy(dense.data() + (size_t)b * 64, coef + off[b], lens[b] * sizeof(int16_t));
    }
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf d_dense, d_lens;
    upload(d_dense, dense.data(), dense.size() * sizeof(int16_t));
    upload(d_lens, lens.data(), lens.size() * sizeof(uint32_t));
    gtx::JpegHuff huff(ctx, hd, quant);
    huff.enqueue(d_dense.as<const int16_t>(), d_lens.as<const uint32_t>());
    fits = huff.finish(out, capacity, n, block_bits);
  });
  return st != GTX_OK ? st : fits ? 0 : 1;
}

// ---- the GPU entropy decoder on a host plan (tests/test_jpeg_entropy_ops_gpu.py)

int gtx_op_jpeg_entropy(gtx_ctx* ctx, const void* plan, size_t bytes, int sub_bits, int rounds, void* record, size_t capacity, size_t* record_bytes,
                        int* status, int* rounds_used) {
  bool fits = true;
  const int st = guarded([&] {
    need(plan, "plan"); need(record_bytes, "record_bytes"); need(status, "status"); need(rounds_used, "rounds_used");
    *record_bytes = 0, *status = 0, *rounds_used = 0;
    if (!record && capacity) op_bad("jpeg_entropy", "record is NULL with a capacity");
    if (record && (reinterpret_cast<uintptr_t>(record) & 3)) op_bad("jpeg_entropy", "the record buffer is not 4-byte aligned");
    if (sub_bits != 0 && !gtx::jpeg_entropy_sub_bits_ok(sub_bits)) op_bad("jpeg_entropy", "sub_bits is none of 0 (the production choice), 256, 512, 1024, 2048");
    if (rounds < 0 || rounds > gtx::kJpegEntropyMaxRounds) op_bad("jpeg_entropy", "rounds is outside 0 (the production choice), 1..64");
    char msg[256];
    if (gtx::jpeg::check_plan(plan, bytes, msg, sizeof msg) != 0) gtx::fail(GTX_ERR_INVALID, "%s", msg);
    gtx::jpeg::PlanHeader ph;
    memcpy(&ph, plan, sizeof ph);
    if (ph.stream_bytes > (1u << 28)) op_bad("jpeg_entropy", "more than 256 MB of entropy-coded data");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t nb = ph.n_blocks, bound = gtx::jpeg::record_bytes(nb, 64 * nb);
    gtx::DevBuf d_plan, d_rec(bound);
    upload(d_plan, plan, bytes);
    gtx::JpegEntropy dec(ctx, nb, ph.stream_bytes, sub_bits ? sub_bits : gtx::kJpegEntropySubBits);
    dec.enqueue(d_plan.as<const uint8_t>(), ph, sub_bits, rounds, d_rec.as<uint8_t>());
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    uint32_t res[2];
    GTX_HIP(hipMemcpy(res, dec.d_result(), sizeof res, hipMemcpyDeviceToHost));
    *status = (int)res[0], *rounds_used = (int)res[1];
    if (res[0] != 0) return;                                      // no record: the host parser says what is wrong with the frame
    gtx::jpeg::RecordHeader hd;
    GTX_HIP(hipMemcpy(&hd, d_rec.p, sizeof hd, hipMemcpyDeviceToHost));
    if (hd.n_blocks != nb || hd.n_coef > 64 * nb || hd.bytes != gtx::jpeg::record_bytes(nb, hd.n_coef))
      gtx::fail(GTX_ERR_INTERNAL, "jpeg_entropy: the device reports a record of %u bytes for %zu blocks", hd.bytes, nb);
    *record_bytes = hd.bytes;
    fits = capacity >= hd.bytes;
    if (fits) download(record, d_rec, hd.bytes);
  });
  return st != GTX_OK ? st : fits ? 0 : 1;
}

// ---- the restart-interval decoder on a host interval plan (tests/test_jpeg_restart_gpu.py)

int gtx_op_jpeg_restart(gtx_ctx* ctx, const void* plan, size_t bytes, void* record, size_t capacity, size_t* record_bytes, int* status) {
  bool fits = true;
  const int st = guarded([&] {
    need(plan, "plan"); need(record_bytes, "record_bytes"); need(status, "status");
    *record_bytes = 0, *status = 0;
    if (!record && capacity) op_bad("jpeg_restart", "record is NULL with a capacity");
    if (record && (reinterpret_cast<uintptr_t>(record) & 3)) op_bad("jpeg_restart", "the record buffer is not 4-byte aligned");
    char msg[256];
    if (gtx::jpeg::check_plan_intervals(plan, bytes, msg, sizeof msg) != 0) gtx::fail(GTX_ERR_INVALID, "%s", msg);
    gtx::jpeg::PlanHeader ph;
    memcpy(&ph, plan, sizeof ph);
    if (ph.stream_bytes > (1u << 28)) op_bad("jpeg_restart", "more than 256 MB of entropy-coded data");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t nb = ph.n_blocks, bound = gtx::jpeg::record_bytes(nb, 64 * nb);
    gtx::DevBuf d_plan, d_rec(bound);
    upload(d_plan, plan, bytes);
    gtx::JpegRestart dec(ctx, 1, nb);
    const uint8_t* plans[1] = {d_plan.as<const uint8_t>()};
    uint8_t* recs[1] = {d_rec.as<uint8_t>()};
    dec.enqueue(1, plans, &ph, recs);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    uint32_t res = 0;
    GTX_HIP(hipMemcpy(&res, dec.d_result(0), sizeof res, hipMemcpyDeviceToHost));
    *status = (int)res;
    if (res != 0) return;                                         // no record: the host parser says what is wrong with the frame
    gtx::jpeg::RecordHeader hd;
    GTX_HIP(hipMemcpy(&hd, d_rec.p, sizeof hd, hipMemcpyDeviceToHost));
    if (hd.n_blocks != nb || hd.n_coef > 64 * nb || hd.bytes != gtx::jpeg::record_bytes(nb, hd.n_coef))
      gtx::fail(GTX_ERR_INTERNAL, "jpeg_restart: the device reports a record of %u bytes for %zu blocks", hd.bytes, nb);
    *record_bytes = hd.bytes;
    fits = capacity >= hd.bytes;
    if (fits) download(record, d_rec, hd.bytes);
  });
  return st != GTX_OK ? st : fits ? 0 : 1;
}

// ---- the drawing kernel on a host frame (tests/test_draw_ops_gpu.py)

int gtx_op_draw(gtx_ctx* ctx, uint8_t* bgr, int h, int w, const int32_t* prims, int n, const void* atlas, size_t atlas_bytes) {
  return guarded([&] {
    gtx::draw_check_frame(h, w);
    need(bgr, "bgr");
    if (!atlas && atlas_bytes) op_bad("draw", "atlas is NULL with a size");
    gtx::draw_check_prims(prims, n, gtx::kDrawMaxPrims, atlas_bytes);
    gtx::Drawer::check_args(h, w, n > 0 ? n : 1, atlas, atlas_bytes);
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf d_bgr;
    upload(d_bgr, bgr, (size_t)h * w * 3);
    gtx::Drawer drawer(ctx, h, w, n > 0 ? n : 1, atlas, atlas_bytes);
    drawer.draw(d_bgr.p, prims, n);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(bgr, d_bgr, (size_t)h * w * 3);
  });
}

}  // extern "C"
