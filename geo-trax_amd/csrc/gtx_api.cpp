// C ABI of libgtx.so (see include/gtx.h). Everything here is a thin try/catch shim that turns
// gtx::Error into a status code + thread-local message.
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/gtx.h"
#include "api_guard.hpp"
#include "common.hpp"
#include "conv_igemm.hpp"
#include "det_kernels.hpp"
#include "detector.hpp"
#include "rtdetr.hpp"
#include "rtdetr_kernels.hpp"
#include "geometry.hpp"
#include "ecc.hpp"
#include "gmc.hpp"
#include "gmc_feat.hpp"
#include "jpeg.hpp"
#include "match_l2.hpp"
#include "register.hpp"
#include "sift.hpp"
#include "split_format.hpp"
#include "stabilizer.hpp"
#include "tracker.hpp"

namespace {
using gtx::g_last_error;
using gtx::guarded;

void need(const void* p, const char* what) {
  if (!p) gtx::fail(GTX_ERR_INVALID, "%s is NULL", what);
}
}  // namespace

extern "C" {

int gtx_abi_version(void) { return GTX_ABI_VERSION; }
const char* gtx_last_error(void) { return g_last_error.c_str(); }

int gtx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}

int gtx_ctx_create(int device, gtx_ctx** out) { return gtx_ctx_create_prio(device, 0, out); }

int gtx_ctx_create_prio(int device, int high_priority, gtx_ctx** out) {
  return guarded([&] {
    need(out, "out");
    int n = 0;
    GTX_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) gtx::fail(GTX_ERR_INVALID, "device %d not in [0,%d)", device, n);
    GTX_HIP(hipSetDevice(device));
    std::unique_ptr<gtx_ctx> c(new gtx_ctx);
    c->device = device;
    GTX_HIP(hipGetDeviceProperties(&c->prop, device));
    if (std::string(c->prop.gcnArchName).find("gfx950") == std::string::npos)
      gtx::fail(GTX_ERR_UNSUPPORTED, "libgtx is built for gfx950 only; device %d is %s", device, c->prop.gcnArchName);
    if (high_priority != 0) {        // > 0: the device's highest stream priority, < 0: its lowest
      int least = 0, greatest = 0;   // numerically lower = higher priority
      GTX_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
      GTX_HIP(hipStreamCreateWithPriority(&c->stream, hipStreamDefault, high_priority > 0 ? greatest : least));
    } else {
      GTX_HIP(hipStreamCreate(&c->stream));
    }
    *out = c.release();
  });
}

void gtx_ctx_destroy(gtx_ctx* ctx) { delete ctx; }

namespace {
// one wave that does nothing for `ticks` of the 100 MHz constant clock
__global__ void spin_kernel(unsigned long long ticks, unsigned long long* sink) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long t = t0;
  while (t - t0 < ticks) {
    __builtin_amdgcn_s_sleep(16);
    t = __builtin_amdgcn_s_memrealtime();
  }
  if (sink && threadIdx.x == 0 && ticks == ~0ull) *sink = t;
}
}  // namespace

int gtx_device_mem_info(int device, size_t* free_bytes, size_t* total_bytes) {
  return guarded([&] {
    need(free_bytes, "free_bytes"); need(total_bytes, "total_bytes");
    GTX_HIP(hipSetDevice(device));
    GTX_HIP(hipMemGetInfo(free_bytes, total_bytes));
  });
}

int gtx_streams_overlap(gtx_ctx* a, gtx_ctx* b, float spin_us, float* ms_single, float* ms_pair) {
  return guarded([&] {
    need(a, "a"); need(b, "b"); need(ms_single, "ms_single"); need(ms_pair, "ms_pair");
    if (a->device != b->device) gtx::fail(GTX_ERR_INVALID, "the two contexts are on devices %d and %d", a->device, b->device);
    GTX_HIP(hipSetDevice(a->device));
    const unsigned long long ticks = (unsigned long long)(std::max(spin_us, 1.f) * 100.f);
    auto timed = [&](bool both) {
      GTX_HIP(hipStreamSynchronize(a->stream));
      GTX_HIP(hipStreamSynchronize(b->stream));
      const auto t0 = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, a->stream, ticks, (unsigned long long*)nullptr);
      if (both) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, b->stream, ticks, (unsigned long long*)nullptr);
      GTX_HIP(hipGetLastError());
      GTX_HIP(hipStreamSynchronize(a->stream));
      GTX_HIP(hipStreamSynchronize(b->stream));
      return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    (void)timed(true);                       // the code object is loaded, both streams have run something
    float one = 1e30f, two = 1e30f;
    for (int i = 0; i < 3; ++i) {            // host-timed: the best of three is the one without a scheduling hiccup
      one = std::min(one, timed(false));
      two = std::min(two, timed(true));
    }
    *ms_single = one;
    *ms_pair = two;
  });
}

int gtx_device_open_null_stream(int device) {
  return guarded([&] {
    GTX_HIP(hipSetDevice(device));
    void* p = nullptr;
    GTX_HIP(hipMalloc(&p, 256));
    hipError_t e = hipMemset(p, 0, 4);            // synchronous: runs on (and thereby creates) the null stream
    (void)hipFree(p);
    GTX_HIP(e);
  });
}

int gtx_ctx_synchronize(gtx_ctx* ctx) {
  return guarded([&] {
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    GTX_HIP(hipStreamSynchronize(ctx->stream));
  });
}

int gtx_dev_alloc(gtx_ctx* ctx, size_t bytes, void** dptr) {
  return guarded([&] {
    need(ctx, "ctx");
    need(dptr, "dptr");
    GTX_HIP(hipSetDevice(ctx->device));
    GTX_HIP(hipMalloc(dptr, bytes ? bytes : 256));
  });
}
int gtx_dev_free(gtx_ctx* ctx, void* dptr) {
  return guarded([&] {
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    if (dptr) GTX_HIP(hipFree(dptr));
  });
}
int gtx_dev_upload(gtx_ctx* ctx, void* dptr, const void* host, size_t bytes) {
  return guarded([&] {
    need(ctx, "ctx"); need(dptr, "dptr"); need(host, "host");
    GTX_HIP(hipSetDevice(ctx->device));
    GTX_HIP(hipMemcpyAsync(dptr, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    GTX_HIP(hipStreamSynchronize(ctx->stream));
  });
}
int gtx_dev_download(gtx_ctx* ctx, void* host, const void* dptr, size_t bytes) {
  return guarded([&] {
    need(ctx, "ctx"); need(dptr, "dptr"); need(host, "host");
    GTX_HIP(hipSetDevice(ctx->device));
    GTX_HIP(hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    GTX_HIP(hipStreamSynchronize(ctx->stream));
  });
}

/* ------------------------------------------------------------------ operator level */

namespace {
struct ConvOpState {
  gtx::DevBuf x, w, b, r, y;
  gtx::ConvGroup g{};
  gtx::ConvConfig cfg{};
  int ho = 0, wo = 0;
};

void conv_setup(gtx_ctx* ctx, const gtx_conv_desc* d, const void* x, const float* w, const float* bias,
                const void* residual, const void* y_init, ConvOpState& st) {
  using namespace gtx;
  need(ctx, "ctx"); need(d, "desc");
  GTX_HIP(hipSetDevice(ctx->device));
  if (d->dtype != GTX_F16 && d->dtype != GTX_F32 && d->dtype != GTX_F32S) fail(GTX_ERR_INVALID, "bad dtype %d", d->dtype);
  const size_t es = dtype_size(d->dtype);
  const int pad = d->ksize / 2;
  st.ho = (d->h + 2 * pad - d->ksize) / d->stride + 1;
  st.wo = (d->w + 2 * pad - d->ksize) / d->stride + 1;
  st.cfg = conv_pick_config(d->dtype, d->ksize, d->stride, d->cin, d->cout);
  const bool pairs = d->dtype == GTX_F32S;       // host arrays are plain fp32; the device buffers hold the pair format (split_format.hpp)
  const int vn = pairs ? 8 : 16 / (int)es;
  GTX_CHECK(d->in_cstride % vn == 0 && d->in_coff % vn == 0 && d->out_cstride % (pairs ? 8 : 4) == 0 && d->out_coff % (pairs ? 8 : 4) == 0 &&
                (!pairs || d->cout % 8 == 0),
            "conv: channel strides/offsets must keep 16-byte (input) / 4-element (output) alignment, whole 8-channel groups for the split-f16x3 path");
  GTX_CHECK(d->in_coff + d->cin <= d->in_cstride && d->out_coff + d->cout <= d->out_cstride, "conv: slice outside buffer");
  const size_t xin = (size_t)d->n * d->h * d->w * d->in_cstride * es;
  const size_t yout = (size_t)d->n * st.ho * st.wo * d->out_cstride * es;
  st.x.alloc(xin);
  st.y.alloc(yout);
  // timing calls (no data handed in) run on pseudo-random activations and weights: zeros would flatter the matrix pipe
  // (no operand toggling, no power throttling) -- the layer sweeps of rounds 1 and 2 up to this change were taken on zeros
  unsigned long long lcg = 0x2545F4914F6CDD1Dull;
  const bool zeros = std::getenv("GTX_TIME_ZEROS") != nullptr;      // the old behaviour, to show the difference
  auto uni = [&]() { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return zeros ? 0.f : (float)((lcg >> 40) * (1.0 / 8388608.0) - 1.0); };
  auto upload = [&](void* dst, const void* src, size_t bytes) {           // plain fp32 host array -> pair format on the device
    if (!pairs) { GTX_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return; }
    std::vector<uint8_t> tmp(bytes);
    f32_to_pairs(static_cast<const float*>(src), tmp.data(), bytes / 4);
    GTX_HIP(hipMemcpy(dst, tmp.data(), bytes, hipMemcpyHostToDevice));
  };
  if (x) {
    upload(st.x.p, x, xin);
  } else if (es == 2) {
    std::vector<_Float16> hx(xin / 2);
    for (auto& v : hx) v = (_Float16)uni();
    GTX_HIP(hipMemcpy(st.x.p, hx.data(), xin, hipMemcpyHostToDevice));
  } else {
    std::vector<float> hx(xin / 4);
    for (auto& v : hx) v = uni();
    upload(st.x.p, hx.data(), xin);
  }
  if (y_init) upload(st.y.p, y_init, yout);
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
  st.w.alloc(packed.size());
  GTX_HIP(hipMemcpy(st.w.p, packed.data(), packed.size(), hipMemcpyHostToDevice));
  if (bias) {
    const size_t padded = (size_t)(d->cout + 63) / 64 * 64 * sizeof(float);      // whole cout tiles: the kernels load a tile's bias unconditionally
    st.b.alloc(padded);
    GTX_HIP(hipMemset(st.b.p, 0, padded));
    GTX_HIP(hipMemcpy(st.b.p, bias, d->cout * sizeof(float), hipMemcpyHostToDevice));
  }
  if (d->has_residual) {
    const size_t rb = (size_t)d->n * st.ho * st.wo * d->cout * es;
    st.r.alloc(rb);
    if (residual) upload(st.r.p, residual, rb);
    else GTX_HIP(hipMemset(st.r.p, 0, rb));
  }
  ConvProblem& p = st.g.p[0];
  p.in = st.x.p; p.out = st.y.p; p.wpack = st.w.p;
  p.bias = bias ? st.b.as<float>() : nullptr;
  p.res = d->has_residual ? st.r.p : nullptr;
  p.N = d->n; p.H = d->h; p.W = d->w; p.Ho = st.ho; p.Wo = st.wo; p.Cin = d->cin; p.Cout = d->cout;
  p.in_cstride = d->in_cstride; p.in_coff = d->in_coff;
  p.out_cstride = d->out_cstride; p.out_coff = d->out_coff;
  p.res_cstride = d->cout; p.res_coff = 0;
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
    if (d->dtype == GTX_F32S) {                       // pair format -> the caller's plain fp32 array
      std::vector<uint8_t> tmp(yb);
      GTX_HIP(hipMemcpy(tmp.data(), st.y.p, yb, hipMemcpyDeviceToHost));
      gtx::pairs_to_f32(tmp.data(), static_cast<float*>(y), yb / 4);
    } else {
      GTX_HIP(hipMemcpy(y, st.y.p, yb, hipMemcpyDeviceToHost));
    }
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
      const gtx::ConvConfig &a = st[0].cfg, &b = st[i].cfg;
      if (a.dtype != b.dtype || a.ks != b.ks || a.stride != b.stride || a.bn != b.bn || a.kc != b.kc || a.variant != b.variant || a.th != b.th)
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
      if (descs[i].dtype == GTX_F32S) {                 // pair format -> the caller's plain fp32 array
        std::vector<uint8_t> tmp(yb);
        GTX_HIP(hipMemcpy(tmp.data(), st[i].y.p, yb, hipMemcpyDeviceToHost));
        gtx::pairs_to_f32(tmp.data(), static_cast<float*>(ys[i]), yb / 4);
      } else {
        GTX_HIP(hipMemcpy(ys[i], st[i].y.p, yb, hipMemcpyDeviceToHost));
      }
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

int gtx_op_conv2d_time(gtx_ctx* ctx, const gtx_conv_desc* d, int iters, float* ms_per_launch, double* flops) {
  return guarded([&] {
    need(ms_per_launch, "ms_per_launch");
    if (iters < 1) gtx::fail(GTX_ERR_INVALID, "iters must be >= 1");
    ConvOpState st;
    conv_setup(ctx, d, nullptr, nullptr, nullptr, nullptr, nullptr, st);
    hipEvent_t e0, e1;
    GTX_HIP(hipEventCreate(&e0));
    GTX_HIP(hipEventCreate(&e1));
    auto once = [&] {
      gtx::conv_launch(st.g, st.cfg, ctx->stream);
      };
    for (int i = 0; i < 3; ++i) once();
    GTX_HIP(hipEventRecord(e0, ctx->stream));
    for (int i = 0; i < iters; ++i) once();
    GTX_HIP(hipEventRecord(e1, ctx->stream));
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    GTX_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_launch = ms / iters;
    if (flops) *flops = gtx::conv_flops(st.g.p[0], d->ksize);
  });
}

int gtx_op_sppf_pool(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, void* x_inout) {
  return guarded([&] {
    need(ctx, "ctx"); need(x_inout, "x");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t bytes = (size_t)n * h * w * 4 * c * gtx::dtype_size(dtype);
    gtx::DevBuf d(bytes);
    std::vector<uint8_t> tmp;
    if (dtype == GTX_F32S) {                          // plain fp32 host array <-> pair format on the device
      tmp.resize(bytes);
      gtx::f32_to_pairs(static_cast<const float*>(x_inout), tmp.data(), bytes / 4);
    }
    GTX_HIP(hipMemcpy(d.p, dtype == GTX_F32S ? tmp.data() : x_inout, bytes, hipMemcpyHostToDevice));
    gtx::launch_sppf_pool(dtype, d.p, n, h, w, c, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(dtype == GTX_F32S ? tmp.data() : x_inout, d.p, bytes, hipMemcpyDeviceToHost));
    if (dtype == GTX_F32S) gtx::pairs_to_f32(tmp.data(), static_cast<float*>(x_inout), bytes / 4);
  });
}

int gtx_op_upsample2x(gtx_ctx* ctx, int dtype, int n, int h, int w, int c, const void* x, int in_cstride,
                      int in_coff, void* y, int out_cstride, int out_coff) {
  return guarded([&] {
    need(ctx, "ctx"); need(x, "x"); need(y, "y");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t es = gtx::dtype_size(dtype);
    const size_t xb = (size_t)n * h * w * in_cstride * es, yb = (size_t)n * 4 * h * w * out_cstride * es;
    gtx::DevBuf dx(xb), dy(yb);
    GTX_HIP(hipMemcpy(dx.p, x, xb, hipMemcpyHostToDevice));
    GTX_HIP(hipMemcpy(dy.p, y, yb, hipMemcpyHostToDevice));
    gtx::launch_upsample2x(dtype, dx.p, n, h, w, c, in_cstride, in_coff, dy.p, out_cstride, out_coff, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(y, dy.p, yb, hipMemcpyDeviceToHost));
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
    gtx::DevBuf dx(xb), dy(yb), dw(9 * C * 4), db(C * 4), ds(4);
    std::vector<uint8_t> tx, ty;
    if (dtype == GTX_F32S) {                          // plain fp32 host arrays <-> pair format on the device
      tx.resize(xb); ty.resize(yb);
      gtx::f32_to_pairs(static_cast<const float*>(qkv), tx.data(), xb / 4);
      gtx::f32_to_pairs(static_cast<const float*>(out), ty.data(), yb / 4);
    }
    GTX_HIP(hipMemcpy(dx.p, dtype == GTX_F32S ? tx.data() : qkv, xb, hipMemcpyHostToDevice));
    GTX_HIP(hipMemcpy(dy.p, dtype == GTX_F32S ? ty.data() : out, yb, hipMemcpyHostToDevice));
    GTX_HIP(hipMemcpy(dw.p, pe_w, 9 * C * 4, hipMemcpyHostToDevice));
    GTX_HIP(hipMemcpy(db.p, pe_b, C * 4, hipMemcpyHostToDevice));
    GTX_HIP(hipMemset(ds.p, 0, 4));
    const gtx::RtMap in{dx.p, h, w, in_cstride, in_coff, heads * 128}, o{dy.p, h, w, out_cstride, out_coff, heads * 64};
    auto once = [&] { gtx::launch_psa_attention(dtype, in, o, n, heads, dw.as<float>(), db.as<float>(), ds.as<int>(), ctx->stream, form); };
    once();
    if (iters > 0 && ms_per_launch) {
      hipEvent_t e0, e1;
      GTX_HIP(hipEventCreate(&e0));
      GTX_HIP(hipEventCreate(&e1));
      for (int i = 0; i < 3; ++i) once();
      GTX_HIP(hipEventRecord(e0, ctx->stream));
      for (int i = 0; i < iters; ++i) once();
      GTX_HIP(hipEventRecord(e1, ctx->stream));
      GTX_HIP(hipStreamSynchronize(ctx->stream));
      float ms = 0.f;
      GTX_HIP(hipEventElapsedTime(&ms, e0, e1));
      (void)hipEventDestroy(e0);
      (void)hipEventDestroy(e1);
      *ms_per_launch = ms / iters;
    }
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(dtype == GTX_F32S ? ty.data() : out, dy.p, yb, hipMemcpyDeviceToHost));
    if (dtype == GTX_F32S) gtx::pairs_to_f32(ty.data(), static_cast<float*>(out), yb / 4);
    if (saturated) GTX_HIP(hipMemcpy(saturated, ds.p, 4, hipMemcpyDeviceToHost));
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
    gtx::DevBuf dx(xb), dy(yb), dr(res ? yb : 16), dw(wb), db((size_t)c * 4), ds(4);
    std::vector<uint8_t> tx, ty;
    auto up = [&](gtx::DevBuf& d, const void* src, size_t bytes) {
      if (dtype == GTX_F32S) {                        // plain fp32 host arrays <-> pair format on the device
        tx.resize(bytes);
        gtx::f32_to_pairs(static_cast<const float*>(src), tx.data(), bytes / 4);
        src = tx.data();
      }
      GTX_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    };
    up(dx, x, xb);
    if (res) up(dr, res, yb);
    GTX_HIP(hipMemcpy(dw.p, wt, wb, hipMemcpyHostToDevice));
    GTX_HIP(hipMemcpy(db.p, bias, (size_t)c * 4, hipMemcpyHostToDevice));
    GTX_HIP(hipMemset(ds.p, 0, 4));
    GTX_HIP(hipMemset(dy.p, 0, yb));
    const gtx::RtMap in{dx.p, h, w, c, 0, c}, o{dy.p, ho, wo, c, 0, c}, r{dr.p, ho, wo, c, 0, c};
    gtx::launch_rt_dwconv(dtype, in, o, n, k, stride, dw.as<float>(), db.as<float>(), act, ds.as<int>(), ctx->stream, res ? &r : nullptr);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    if (dtype == GTX_F32S) {
      ty.resize(yb);
      GTX_HIP(hipMemcpy(ty.data(), dy.p, yb, hipMemcpyDeviceToHost));
      gtx::pairs_to_f32(ty.data(), static_cast<float*>(out), yb / 4);
    } else {
      GTX_HIP(hipMemcpy(out, dy.p, yb, hipMemcpyDeviceToHost));
    }
    if (saturated) GTX_HIP(hipMemcpy(saturated, ds.p, 4, hipMemcpyDeviceToHost));
  });
}

// ---- RT-DETR's token-side kernels, one hook per launcher (tests/test_rtdetr_ops_gpu.py). Every size is checked here, before
// anything touches the GPU: whatever a launcher's own GTX_CHECK would refuse, and whatever would let a kernel read or write
// outside the arrays it is given.
namespace {
void rt_bad(const char* op, const char* what) { gtx::fail(GTX_ERR_INVALID, "%s: %s", op, what); }

// Up to three levels of NHWC maps [n][h][w][cstride] with `c` channels read from coff
struct RtLevelSet {
  gtx::RtLevels L{};
  gtx::DevBuf buf[3];
  int S = 0;
};
void rt_levels_check(const char* op, int fmt, int n, int n_levels, const void* const* maps, const int* h, const int* w, const int* cstride,
                     const int* coff, int c, bool allow_split) {
  need(maps, "maps"); need(h, "h"); need(w, "w"); need(cstride, "cstride"); need(coff, "coff");
  if (!(fmt == GTX_F16 || fmt == GTX_F32 || (allow_split && fmt == GTX_F32S))) rt_bad(op, "unsupported map format");
  if (n < 1 || n_levels < 1 || n_levels > 3 || c < 1) rt_bad(op, "bad sizes");
  long S = 0;
  for (int l = 0; l < n_levels; ++l) {
    need(maps[l], "maps[l]");
    if (h[l] < 1 || w[l] < 1 || coff[l] < 0 || (long)coff[l] + c > cstride[l]) rt_bad(op, "a level's channel slice does not fit its stride");
    if (fmt == GTX_F32S && (cstride[l] % 8 || coff[l] % 8)) rt_bad(op, "pair-format maps need channel strides and offsets that are multiples of 8");
    S += (long)h[l] * w[l];
    if (S > (1l << 24) || (double)n * h[l] * w[l] * cstride[l] > 1e9) rt_bad(op, "maps too large");
  }
}
void rt_levels_upload(RtLevelSet& s, int fmt, int n, int n_levels, const void* const* maps, const int* h, const int* w, const int* cstride,
                      const int* coff) {
  s.L.n_levels = n_levels;
  std::vector<uint8_t> tmp;
  for (int l = 0; l < n_levels; ++l) {
    const size_t bytes = (size_t)n * h[l] * w[l] * cstride[l] * gtx::dtype_size(fmt);
    s.buf[l].alloc(bytes);
    const void* src = maps[l];
    if (fmt == GTX_F32S) {                            // plain fp32 host arrays -> pair format on the device
      tmp.resize(bytes);
      gtx::f32_to_pairs(static_cast<const float*>(src), tmp.data(), bytes / 4);
      src = tmp.data();
    }
    GTX_HIP(hipMemcpy(s.buf[l].p, src, bytes, hipMemcpyHostToDevice));
    s.L.ptr[l] = s.buf[l].p; s.L.h[l] = h[l]; s.L.w[l] = w[l]; s.L.cstride[l] = cstride[l]; s.L.coff[l] = coff[l];
    s.S += h[l] * w[l];
  }
}
void rt_upload(gtx::DevBuf& d, const void* src, size_t bytes) {
  d.alloc(bytes);
  GTX_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
}
}  // namespace

int gtx_op_rt_linear(gtx_ctx* ctx, int M, int K, int Nout, const float* x, int ldx, const float* x2, int ldx2, int x2_cols, const float* w,
                     const float* bias, const float* res, int ldr, float* y, int ldy, int ycol, int act) {
  return guarded([&] {
    const char* op = "rt_linear";
    if (M < 1 || M > (1 << 20) || K < 16 || K % 16 || K > (1 << 16) || Nout < 16 || Nout % 16 || Nout > (1 << 16)) rt_bad(op, "M >= 1, K and Nout positive multiples of 16");
    if (ldx < K || ldx % 4 || ldx > (1 << 20)) rt_bad(op, "ldx must hold K values and be a multiple of 4");
    if (x2 && (ldx2 < K || ldx2 % 4 || ldx2 > (1 << 20) || x2_cols < 0 || (x2_cols % 64 && x2_cols < Nout)))
      rt_bad(op, "the second addend needs ldx2 >= K, a multiple of 4, and x2_cols a multiple of 64 or all of Nout");
    if (res && (ldr < Nout || ldr > (1 << 20))) rt_bad(op, "ldr must hold Nout values");
    if (ycol < 0 || ldy > (1 << 20) || (long)ycol + Nout > ldy) rt_bad(op, "the output columns do not fit ldy");
    if (act != 0 && act != 2 && act != 3) rt_bad(op, "act: 0 none, 2 ReLU, 3 GELU");
    need(ctx, "ctx"); need(x, "x"); need(w, "w"); need(y, "y");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf dx, dx2, dw, db, dr, dy;
    rt_upload(dx, x, (size_t)M * ldx * 4);
    if (x2) rt_upload(dx2, x2, (size_t)M * ldx2 * 4);
    rt_upload(dw, w, (size_t)Nout * K * 4);
    if (bias) rt_upload(db, bias, (size_t)Nout * 4);
    if (res) rt_upload(dr, res, (size_t)M * ldr * 4);
    rt_upload(dy, y, (size_t)M * ldy * 4);
    gtx::RtLinear p{};
    p.x = dx.as<float>(); p.ldx = ldx;
    p.x2 = x2 ? dx2.as<float>() : nullptr; p.ldx2 = ldx2; p.x2_cols = x2_cols;
    p.w = dw.as<float>(); p.bias = bias ? db.as<float>() : nullptr;
    p.res = res ? dr.as<float>() : nullptr; p.ldr = ldr;
    p.y = dy.as<float>() + ycol; p.ldy = ldy;
    p.M = M; p.K = K; p.Nout = Nout; p.act = act;
    gtx::launch_rt_linear(p, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(y, dy.p, (size_t)M * ldy * 4, hipMemcpyDeviceToHost));
  });
}

int gtx_op_rt_layernorm(gtx_ctx* ctx, int rows, int C, int in_fmt, const void* in, int in_cstride, int in_coff, int out_fmt, void* out,
                        int out_cstride, int out_coff, const float* gamma, const float* beta, int* saturated) {
  return guarded([&] {
    const char* op = "rt_layernorm";
    if (rows < 1 || rows > (1 << 22) || C < 8 || C % 8 || C > 1024) rt_bad(op, "rows >= 1, C a multiple of 8 up to 1024");
    const bool pair_ok = (in_fmt == GTX_F32 && (out_fmt == GTX_F32 || out_fmt == GTX_F32S || out_fmt == GTX_F16)) ||
                         (in_fmt == GTX_F32S && out_fmt == GTX_F32S) || (in_fmt == GTX_F16 && out_fmt == GTX_F16);
    if (!pair_ok) rt_bad(op, "formats: F32 -> F32 / F32S / F16, F32S -> F32S, F16 -> F16");
    if (in_coff < 0 || in_coff % 8 || in_cstride % 8 || in_cstride > (1 << 16) || (long)in_coff + C > in_cstride || out_coff < 0 || out_coff % 8 ||
        out_cstride % 8 || out_cstride > (1 << 16) || (long)out_coff + C > out_cstride)
      rt_bad(op, "channel strides / offsets must be multiples of 8 and hold C channels");
    need(ctx, "ctx"); need(in, "in"); need(out, "out"); need(gamma, "gamma"); need(beta, "beta");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t xb = (size_t)rows * in_cstride * gtx::dtype_size(in_fmt), yb = (size_t)rows * out_cstride * gtx::dtype_size(out_fmt);
    gtx::DevBuf dx(xb), dy(yb), dg, dbt, ds(4);
    std::vector<uint8_t> tx, ty;
    if (in_fmt == GTX_F32S) {                         // plain fp32 host arrays <-> pair format on the device
      tx.resize(xb);
      gtx::f32_to_pairs(static_cast<const float*>(in), tx.data(), xb / 4);
    }
    if (out_fmt == GTX_F32S) {
      ty.resize(yb);
      gtx::f32_to_pairs(static_cast<const float*>(out), ty.data(), yb / 4);
    }
    GTX_HIP(hipMemcpy(dx.p, in_fmt == GTX_F32S ? tx.data() : in, xb, hipMemcpyHostToDevice));
    GTX_HIP(hipMemcpy(dy.p, out_fmt == GTX_F32S ? ty.data() : out, yb, hipMemcpyHostToDevice));
    rt_upload(dg, gamma, (size_t)C * 4);
    rt_upload(dbt, beta, (size_t)C * 4);
    GTX_HIP(hipMemset(ds.p, 0, 4));
    const gtx::RtRows ri{dx.p, in_cstride, in_coff, in_fmt}, ro{dy.p, out_cstride, out_coff, out_fmt};
    gtx::launch_rt_layernorm(ri, ro, rows, C, dg.as<float>(), dbt.as<float>(), ds.as<int>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(out_fmt == GTX_F32S ? ty.data() : out, dy.p, yb, hipMemcpyDeviceToHost));
    if (out_fmt == GTX_F32S) gtx::pairs_to_f32(ty.data(), static_cast<float*>(out), yb / 4);
    if (saturated) GTX_HIP(hipMemcpy(saturated, ds.p, 4, hipMemcpyDeviceToHost));
  });
}

int gtx_op_rt_mha(gtx_ctx* ctx, int n, int T, int C, int heads, const float* qkv, int ld, float* out, int ldo, int form) {
  return guarded([&] {
    const char* op = "rt_mha";
    if (n < 1 || n > 1024 || T < 1 || T > (1 << 20) || heads < 1 || C < 1 || C % heads) rt_bad(op, "bad sizes");
    const int d = C / heads;
    if (d != 8 && d != 16 && d != 32) rt_bad(op, "head dimension 8, 16 or 32");
    if (ld < 3 * C || ld % 4 || ld > (1 << 16) || ldo < C || ldo % 4 || ldo > (1 << 16)) rt_bad(op, "ld >= 3 C, ldo >= C, both multiples of 4");
    if (form != 0 && form != 1) rt_bad(op, "form: 0 the library's rule, 1 the generic kernel");
    need(ctx, "ctx"); need(qkv, "qkv"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf dq, dout;
    rt_upload(dq, qkv, (size_t)n * T * ld * 4);
    rt_upload(dout, out, (size_t)n * T * ldo * 4);
    gtx::launch_rt_mha(dq.as<float>(), ld, n, T, C, heads, dout.as<float>(), ldo, ctx->stream, form);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(out, dout.p, (size_t)n * T * ldo * 4, hipMemcpyDeviceToHost));
  });
}

int gtx_op_rt_topk(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* scores, const int* h, const int* w, const int* cstride,
                   const int* coff, int nc, int nq, int* idx) {
  return guarded([&] {
    const char* op = "rt_topk";
    rt_levels_check(op, fmt, n, n_levels, scores, h, w, cstride, coff, nc, false);
    long S = 0;
    for (int l = 0; l < n_levels; ++l) S += (long)h[l] * w[l];
    if (nq < 1 || nq > 1024 || S < nq) rt_bad(op, "1..1024 queries, no more than there are anchors");
    need(ctx, "ctx"); need(idx, "idx");
    GTX_HIP(hipSetDevice(ctx->device));
    RtLevelSet lv;
    rt_levels_upload(lv, fmt, n, n_levels, scores, h, w, cstride, coff);
    gtx::DevBuf keys((size_t)n * lv.S * 4), di((size_t)n * nq * 4);
    gtx::launch_rt_topk(fmt, lv.L, nc, n, nq, keys.as<unsigned>(), di.as<int>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(idx, di.p, (size_t)n * nq * 4, hipMemcpyDeviceToHost));
  });
}

int gtx_op_rt_gather_refer(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* enc, const int* h, const int* w, const int* cstride,
                           const int* coff, int C, int nq, const int* idx, const float* delta, int ldd, int mode, float* embed, float* anchors,
                           float* refer) {
  return guarded([&] {
    const char* op = "rt_gather_refer";
    if (mode != 0 && mode != 1) rt_bad(op, "mode 0 (gather + anchors) or 1 (inverse sigmoid of refer)");
    if (n < 1 || nq < 1 || (long)n * nq > (1 << 20) || ldd < 4 || ldd > (1 << 16)) rt_bad(op, "bad sizes");
    need(delta, "delta"); need(refer, "refer");
    const int M = n * nq;
    if (mode == 0) {
      rt_levels_check(op, fmt, n, n_levels, enc, h, w, cstride, coff, C, true);
      need(idx, "idx"); need(embed, "embed"); need(anchors, "anchors");
      long S = 0;
      for (int l = 0; l < n_levels; ++l) S += (long)h[l] * w[l];
      for (int m = 0; m < M; ++m)
        if (idx[m] < 0 || idx[m] >= S) rt_bad(op, "an anchor index is outside the level set");
    }
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf dd, dr((size_t)M * 16 * 4);
    rt_upload(dd, delta, (size_t)M * ldd * 4);
    if (mode == 1) {
      GTX_HIP(hipMemcpy(dr.p, refer, (size_t)M * 16 * 4, hipMemcpyHostToDevice));
      gtx::launch_rt_refer(dd.as<float>(), ldd, nullptr, dr.as<float>(), M, 1, ctx->stream);
    } else {
      RtLevelSet lv;
      rt_levels_upload(lv, fmt, n, n_levels, enc, h, w, cstride, coff);
      gtx::DevBuf di, de((size_t)M * C * 4), da((size_t)M * 4 * 4);
      rt_upload(di, idx, (size_t)M * 4);
      GTX_HIP(hipMemset(dr.p, 0, (size_t)M * 16 * 4));
      gtx::launch_rt_gather(fmt, lv.L, C, n, nq, di.as<int>(), de.as<float>(), da.as<float>(), ctx->stream);
      gtx::launch_rt_refer(dd.as<float>(), ldd, da.as<float>(), dr.as<float>(), M, 0, ctx->stream);
      GTX_HIP(hipStreamSynchronize(ctx->stream));
      GTX_HIP(hipMemcpy(embed, de.p, (size_t)M * C * 4, hipMemcpyDeviceToHost));
      GTX_HIP(hipMemcpy(anchors, da.p, (size_t)M * 4 * 4, hipMemcpyDeviceToHost));
    }
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(refer, dr.p, (size_t)M * 16 * 4, hipMemcpyDeviceToHost));
  });
}

int gtx_op_rt_deform(gtx_ctx* ctx, int fmt, int n, int n_levels, const void* const* value, const int* h, const int* w, const int* cstride,
                     const int* coff, int hd, int nh, int npts, int nq, const float* offaw, const float* refer, float* out) {
  return guarded([&] {
    const char* op = "rt_deform";
    if (hd < 1 || hd > 1024 || nh < 1 || hd % nh || npts < 1 || npts > 64 || nq < 1 || n < 1 || (long)n * nq > (1 << 20)) rt_bad(op, "bad sizes");
    rt_levels_check(op, fmt, n, n_levels, value, h, w, cstride, coff, hd, true);
    need(ctx, "ctx"); need(offaw, "offaw"); need(refer, "refer"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    const int M = n * nq;
    RtLevelSet lv;
    rt_levels_upload(lv, fmt, n, n_levels, value, h, w, cstride, coff);
    gtx::DevBuf dof, dr, dout((size_t)M * hd * 4);
    rt_upload(dof, offaw, (size_t)M * nh * n_levels * npts * 3 * 4);
    rt_upload(dr, refer, (size_t)M * 16 * 4);
    gtx::launch_rt_deform(fmt, lv.L, hd, nh, npts, dof.as<float>(), dr.as<float>(), n, nq, dout.as<float>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(out, dout.p, (size_t)M * hd * 4, hipMemcpyDeviceToHost));
  });
}

int gtx_op_rt_post(gtx_ctx* ctx, int n, int nq, int nc, const float* logits, int ldl, const float* refer, float conf, uint64_t class_mask0,
                   uint64_t class_mask1, int frame_w, int frame_h, int max_det, float* out_rows, int* out_n, float* raw) {
  return guarded([&] {
    const char* op = "rt_post";
    if (nq < 1 || nq > 512) rt_bad(op, "1..512 queries");
    if (nc < 1 || nc > 128) rt_bad(op, "1..128 classes (the class mask has two 64-bit words)");
    if (n < 1 || n > 4096 || ldl < nc || ldl > (1 << 16) || max_det < 1 || max_det > (1 << 16) || frame_w < 1 || frame_h < 1) rt_bad(op, "bad sizes");
    need(ctx, "ctx"); need(logits, "logits"); need(refer, "refer"); need(out_rows, "out_rows"); need(out_n, "out_n");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t M = (size_t)n * nq, rawb = M * (4 + nc) * 4, rowb = (size_t)n * max_det * 6 * 4;
    gtx::DevBuf dl, dr, drows, dn((size_t)n * 4), draw(raw ? rawb : 16);
    rt_upload(dl, logits, M * ldl * 4);
    rt_upload(dr, refer, M * 16 * 4);
    rt_upload(drows, out_rows, rowb);
    GTX_HIP(hipMemset(dn.p, 0, (size_t)n * 4));
    const unsigned long long mask[2] = {class_mask0, class_mask1};
    gtx::launch_rt_post(dl.as<float>(), ldl, dr.as<float>(), n, nq, nc, conf, mask, frame_w, frame_h, max_det, drows.as<float>(), dn.as<int>(),
                        raw ? draw.as<float>() : nullptr, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    GTX_HIP(hipMemcpy(out_rows, drows.p, rowb, hipMemcpyDeviceToHost));
    GTX_HIP(hipMemcpy(out_n, dn.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (raw) GTX_HIP(hipMemcpy(raw, draw.p, rawb, hipMemcpyDeviceToHost));
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
  if (dtype != GTX_F16 && dtype != GTX_F32) rt_bad(op, "maps are GTX_F16 or GTX_F32");
  if (n_levels > gtx::kMaxLevels) rt_bad(op, "at most 4 levels");
  if (n < 1 || n > 64 || n_levels < 1) rt_bad(op, "bad sizes");
  if (gate && (nc < 1 || nc > 128)) rt_bad(op, "1..128 classes (the class mask has two 64-bit words)");
  need(lv, "lv");
  const int al = dtype == GTX_F16 ? 8 : 4;          // elements in 16 bytes
  long A = 0;
  for (int l = 0; l < n_levels; ++l) {
    const gtx_head_level& L = lv[l];
    need(L.feat, "lv[l].feat");
    if (L.h < 1 || L.w < 1 || L.cb < 0 || L.cc < 0 || L.cstride < 1 || L.cstride > (1 << 16) || (long)L.cb + L.cc > L.cstride)
      rt_bad(op, "a level's channels do not fit its stride");
    if ((double)n * L.h * L.w * L.cstride > 2.5e8) rt_bad(op, "maps too large");
    A += (long)L.h * L.w;
    if (gate) {
      need(L.wc, "lv[l].wc"); need(L.bc, "lv[l].bc");
      if (L.cc < 8 || L.cc % 8) rt_bad(op, "cc must be a positive multiple of 8 (the kernel reads 8-channel chunks)");
      if (L.cb % al || L.cstride % al) rt_bad(op, "cb and cstride must keep the class features 16-byte aligned");
    }
    if (boxes) {
      need(L.wb, "lv[l].wb"); need(L.bb, "lv[l].bb");
      if (L.cb < 1 || L.cb > 128) rt_bad(op, "1..128 box channels");
      if (L.cb > lv[0].cb) rt_bad(op, "no level's cb may exceed level 0's (the kernel's LDS layout)");
    }
  }
  if (A > (1l << 22)) rt_bad(op, "too many anchors");
  return A;
}
void head_upload(HeadSet& s, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, bool gate, bool boxes) {
  s.hp.n_levels = n_levels;
  s.hp.nc = nc;
  int anchor = 0;
  for (int l = 0; l < n_levels; ++l) {
    const gtx_head_level& L = lv[l];
    gtx::HeadLevel& H = s.hp.lv[l];
    rt_upload(s.feat[l], L.feat, (size_t)n * L.h * L.w * L.cstride * gtx::dtype_size(dtype));
    H.feat = s.feat[l].p; H.h = L.h; H.w = L.w; H.cstride = L.cstride; H.cb = L.cb; H.cc = L.cc; H.stride = L.stride;
    H.anchor_begin = anchor;
    anchor += L.h * L.w;
    if (gate) {
      rt_upload(s.wc[l], L.wc, (size_t)nc * L.cc * 4);
      rt_upload(s.bc[l], L.bc, (size_t)nc * 4);
      H.wc = s.wc[l].as<float>(); H.bc = s.bc[l].as<float>();
    }
    if (boxes) {
      rt_upload(s.wb[l], L.wb, (size_t)L.cb * 64 * 4);
      rt_upload(s.bb[l], L.bb, 64 * 4);
      H.wb = s.wb[l].as<float>(); H.bb = s.bb[l].as<float>();
    }
  }
  s.hp.n_anchors = anchor;
}
// the first min(count, cap) entries of every image index an anchor below `anchors`
void cand_check(const char* op, int n, int cap, const int* count, const int* anchor, long anchors) {
  need(count, "count"); need(anchor, "anchor");
  for (int b = 0; b < n; ++b) {
    if (count[b] < 0) rt_bad(op, "a negative count");
    const int m = std::min(count[b], cap);
    for (int i = 0; i < m; ++i)
      if (anchor[(size_t)b * cap + i] < 0 || anchor[(size_t)b * cap + i] >= anchors) rt_bad(op, "an anchor index is outside the level set");
  }
}
void geometry_check(const char* op, int src_h, int src_w, int net_h, int net_w, double gain) {
  if (src_h < 1 || src_w < 1 || net_h < 1 || net_w < 1 || src_h > (1 << 16) || src_w > (1 << 16) || net_h > (1 << 16) || net_w > (1 << 16) || !(gain > 0.0))
    rt_bad(op, "bad letterbox geometry");
}
gtx::Letterbox geometry(int src_h, int src_w, int net_h, int net_w, double gain) {
  gtx::Letterbox lb{};
  lb.src_h = src_h; lb.src_w = src_w; lb.net_h = net_h; lb.net_w = net_w; lb.gain = gain;
  return lb;
}
void fill_ff(gtx::DevBuf& d, size_t bytes) {
  d.alloc(bytes);
  GTX_HIP(hipMemset(d.p, 0xFF, bytes));
}
void download(void* host, const gtx::DevBuf& d, size_t bytes) { GTX_HIP(hipMemcpy(host, d.p, bytes, hipMemcpyDeviceToHost)); }
}  // namespace

int gtx_op_head_gate(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int nc, float conf, uint64_t class_mask0,
                     uint64_t class_mask1, int cap, int lvl_cap, int* count, float* cand_score, int* cand_anchor, int* cand_cls, int* lvl_count,
                     int* lvl_list) {
  return guarded([&] {
    const char* op = "head_gate";
    head_check(op, dtype, n, n_levels, lv, nc, true, false);
    if (cap < 1 || cap > (1 << 22) || lvl_cap < 0 || lvl_cap > (1 << 22)) rt_bad(op, "cap >= 1, lvl_cap >= 0");
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

int gtx_op_head_boxes(gtx_ctx* ctx, int dtype, int n, int n_levels, const gtx_head_level* lv, int cap, const int* count, const int* cand_anchor,
                      float* cand_box) {
  return guarded([&] {
    const char* op = "head_boxes";
    const long A = head_check(op, dtype, n, n_levels, lv, 0, false, true);
    if (cap < 1 || cap > (1 << 22)) rt_bad(op, "cap >= 1");
    cand_check(op, n, cap, count, cand_anchor, A);
    need(cand_box, "cand_box"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    HeadSet hs;
    head_upload(hs, dtype, n, n_levels, lv, 0, false, true);
    const size_t m = (size_t)n * cap;
    gtx::DevBuf dc, da, db;
    rt_upload(dc, count, (size_t)n * 4); rt_upload(da, cand_anchor, m * 4); fill_ff(db, m * 16);
    gtx::NmsBuffers nb{};
    nb.cap = cap;
    nb.count = dc.as<int>(); nb.cand_anchor = da.as<int>(); nb.cand_box = db.as<float>();
    gtx::launch_head_boxes(dtype, hs.hp, n, nb, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(cand_box, db, m * 16);
  });
}

int gtx_op_nms(gtx_ctx* ctx, int n, int cap, const int* count, const float* cand_score, const int* cand_anchor, const int* cand_cls,
               const float* cand_box, float iou_thr, int agnostic, int max_nms, int nms_cap, int max_det, int src_h, int src_w, int net_h, int net_w,
               double gain, int which, float* out_rows, int* out_n, int* out_anchor) {
  return guarded([&] {
    const char* op = "nms";
    if (n < 1 || n > 64 || cap < 1 || cap > (1 << 20) || max_det < 1 || max_det > (1 << 16) || max_nms < 1) rt_bad(op, "bad sizes");
    if (nms_cap < 64 || nms_cap % 64 || nms_cap > 32768 || (double)n * nms_cap * (nms_cap / 64) * 8 > 3e8) rt_bad(op, "nms_cap: a multiple of 64, the mask within 300 MB");
    if (which < 0 || which > 2) rt_bad(op, "which: 0 both paths, 1 the single-workgroup kernel, 2 the general kernels");
    geometry_check(op, src_h, src_w, net_h, net_w, gain);
    cand_check(op, n, cap, count, cand_anchor, gtx::nms_max_anchors());
    need(cand_score, "cand_score"); need(cand_cls, "cand_cls"); need(cand_box, "cand_box"); need(out_rows, "out_rows"); need(out_n, "out_n");
    need(out_anchor, "out_anchor");
    for (int b = 0; b < n; ++b)
      for (int i = 0; i < std::min(count[b], cap); ++i) {
        if (!(cand_score[(size_t)b * cap + i] > 0.f)) rt_bad(op, "scores must be positive (the sort key is their bit pattern)");
        if (cand_cls[(size_t)b * cap + i] < 0 || cand_cls[(size_t)b * cap + i] > 127) rt_bad(op, "classes 0..127");
      }
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t m = (size_t)n * cap, sm = (size_t)n * nms_cap, rows = (size_t)n * max_det;
    gtx::DevBuf dc, ds, da, dk, db, dsn((size_t)n * 4), sb(sm * 16), ss(sm * 4), sc(sm * 4), sa(sm * 4), dm(sm * (nms_cap / 64) * 8), dn, dr, doa;
    rt_upload(dc, count, (size_t)n * 4); rt_upload(ds, cand_score, m * 4); rt_upload(da, cand_anchor, m * 4); rt_upload(dk, cand_cls, m * 4);
    rt_upload(db, cand_box, m * 16);
    rt_upload(dn, out_n, (size_t)n * 4); rt_upload(dr, out_rows, rows * 24); rt_upload(doa, out_anchor, rows * 4);
    GTX_HIP(hipMemset(dsn.p, 0, (size_t)n * 4));       // which == 2 alone: an image left to the other path has nothing sorted
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
    if (cap < 1 || cap > (1 << 22)) rt_bad(op, "cap >= 1");
    if (sel_cap < gtx::kV10Keep || sel_cap > 512) rt_bad(op, "sel_cap in [300, 512]");
    if (lvl_cap != 0 && (lvl_cap < gtx::kV10Keep || lvl_cap > (1 << 16))) rt_bad(op, "lvl_cap: 0 (not kept) or >= 300");
    cand_check(op, n, cap, count, cand_anchor, A);
    need(cand_score, "cand_score");
    for (int b = 0; b < n; ++b)
      for (int i = 0; i < std::min(count[b], cap); ++i)
        if (!(cand_score[(size_t)b * cap + i] > 0.f)) rt_bad(op, "scores must be positive (the select key is their bit pattern)");
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
    rt_upload(dc, count, (size_t)n * 4); rt_upload(ds, cand_score, m * 4); rt_upload(da, cand_anchor, m * 4);
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
    if (n < 1 || n > 64 || sel_cap < 1 || sel_cap > 512 || max_det < 1 || max_det > (1 << 16)) rt_bad(op, "sel_cap in [1, 512], max_det >= 1");
    geometry_check(op, src_h, src_w, net_h, net_w, gain);
    need(sel_count, "sel_count"); need(sel_score, "sel_score"); need(sel_anchor, "sel_anchor"); need(sel_cls, "sel_cls"); need(sel_box, "sel_box");
    need(out_rows, "out_rows"); need(out_n, "out_n"); need(out_anchor, "out_anchor");
    for (int b = 0; b < n; ++b)
      if (sel_count[b] < 0) rt_bad(op, "a negative count");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t sm = (size_t)n * sel_cap, rows = (size_t)n * max_det;
    gtx::DevBuf qc, qs, qa, qk, qb, dn, dr, doa;
    rt_upload(qc, sel_count, (size_t)n * 4); rt_upload(qs, sel_score, sm * 4); rt_upload(qa, sel_anchor, sm * 4); rt_upload(qk, sel_cls, sm * 4);
    rt_upload(qb, sel_box, sm * 16);
    rt_upload(dn, out_n, (size_t)n * 4); rt_upload(dr, out_rows, rows * 24); rt_upload(doa, out_anchor, rows * 4);
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
    if (dtype != GTX_F16 && dtype != GTX_F32 && dtype != GTX_F32S) rt_bad(op, "unsupported map format");
    if (n_levels > gtx::kMaxLevels) rt_bad(op, "at most 4 levels");
    if (n < 1 || n > 64 || n_levels < 1 || dim < 1 || dim > (1 << 12) || max_det < 1 || max_det > (1 << 16)) rt_bad(op, "bad sizes");
    need(maps, "maps"); need(h, "h"); need(w, "w"); need(cstride, "cstride"); need(coff, "coff"); need(c, "c");
    long A = 0;
    for (int l = 0; l < n_levels; ++l) {
      need(maps[l], "maps[l]");
      if (h[l] < 1 || w[l] < 1 || coff[l] < 0 || c[l] < 1 || cstride[l] > (1 << 16) || (long)coff[l] + c[l] > cstride[l]) rt_bad(op, "a level's channel slice does not fit its stride");
      if (c[l] % dim) rt_bad(op, "every level's channel count must be a multiple of dim");
      if (dtype == GTX_F32S && cstride[l] % 8) rt_bad(op, "pair-format maps need channel strides that are multiples of 8");
      if ((double)n * h[l] * w[l] * cstride[l] > 2.5e8) rt_bad(op, "maps too large");
      A += (long)h[l] * w[l];
    }
    if (A > (1l << 22)) rt_bad(op, "too many anchors");
    cand_check(op, n, max_det, out_n, out_anchor, A);
    need(out, "out"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::FeatLevels fl{};
    gtx::DevBuf buf[gtx::kMaxLevels], dn, doa, dout;
    std::vector<uint8_t> tmp;
    int anchor = 0;
    for (int l = 0; l < n_levels; ++l) {
      const size_t bytes = (size_t)n * h[l] * w[l] * cstride[l] * gtx::dtype_size(dtype);
      const void* src = maps[l];
      if (dtype == GTX_F32S) {                          // plain fp32 host arrays -> pair format on the device
        tmp.resize(bytes);
        gtx::f32_to_pairs(static_cast<const float*>(src), tmp.data(), bytes / 4);
        src = tmp.data();
      }
      rt_upload(buf[l], src, bytes);
      fl.feat[l] = buf[l].p; fl.h[l] = h[l]; fl.w[l] = w[l]; fl.cstride[l] = cstride[l]; fl.coff[l] = coff[l]; fl.c[l] = c[l];
      fl.anchor_begin[l] = anchor;
      anchor += h[l] * w[l];
    }
    fl.n_levels = n_levels;
    fl.dim = dim;
    const size_t rows = (size_t)n * max_det;
    rt_upload(dn, out_n, (size_t)n * 4); rt_upload(doa, out_anchor, rows * 4); rt_upload(dout, out, rows * dim * 4);
    gtx::NmsBuffers nb{};
    nb.max_det = max_det;
    nb.out_n = dn.as<int>(); nb.out_anchor = doa.as<int>();
    gtx::launch_obj_feats(dtype, fl, n, nb, dout.as<float>(), ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    download(out, dout, rows * dim * 4);
  });
}

struct gtx_gmc {
  gtx_ctx* ctx;
  std::unique_ptr<gtx::Gmc> impl;
};

int gtx_gmc_create(gtx_ctx* ctx, int frame_h, int frame_w, int seed, gtx_gmc** out) {
  return guarded([&] {
    need(ctx, "ctx"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<gtx_gmc> g(new gtx_gmc);
    g->ctx = ctx;
    g->impl.reset(new gtx::Gmc(ctx->device, ctx->stream, frame_h / 2, frame_w / 2, seed));
    *out = g.release();
  });
}
void gtx_gmc_destroy(gtx_gmc* g) { delete g; }
int gtx_gmc_reset(gtx_gmc* g) {
  return guarded([&] { need(g, "gmc"); g->impl->reset(); });
}
int gtx_gmc_apply(gtx_gmc* g, const uint8_t* frame_bgr, int h, int w, double A[6], int* valid, int stats[3]) {
  return guarded([&] {
    need(g, "gmc"); need(frame_bgr, "frame"); need(A, "A");
    g->impl->submit_frame(frame_bgr, h, w);
    g->impl->collect(A, valid, stats);
  });
}
int gtx_gmc_submit_gray_dev(gtx_gmc* g, const void* gray_dptr, int gh, int gw) {
  return guarded([&] { need(g, "gmc"); need(gray_dptr, "gray"); g->impl->submit_gray_dev(gray_dptr, gh, gw); });
}
int gtx_gmc_restart(gtx_gmc* g) {
  return guarded([&] { need(g, "gmc"); g->impl->restart(); });
}
int gtx_gmc_submit_frame_dev(gtx_gmc* g, const void* frame_bgr_dptr, int h, int w, int restart) {
  return guarded([&] { need(g, "gmc"); need(frame_bgr_dptr, "frame"); g->impl->submit_frame_dev(frame_bgr_dptr, h, w, restart != 0); });
}
int gtx_gmc_collect(gtx_gmc* g, double A[6], int* valid, int stats[3]) {
  return guarded([&] { need(g, "gmc"); need(A, "A"); g->impl->collect(A, valid, stats); });
}
int gtx_gmc_points(gtx_gmc* g, int which, int cap, int* n, float* xy, int* status) {
  return guarded([&] { need(g, "gmc"); need(n, "n"); g->impl->debug_points(which, cap, n, xy, status); });
}
int gtx_gmc_counts(gtx_gmc* g, int counts[4]) {
  return guarded([&] { need(g, "gmc"); need(counts, "counts"); g->impl->debug_counts(counts); });
}

// ---- the sparse-optical-flow GMC's kernels one launcher at a time (tests/test_gmc_ops_gpu.py). Sizes, and every coordinate a
// kernel would turn into an address, are checked before anything touches the GPU.
int gtx_op_gmc_corners(gtx_ctx* ctx, const uint8_t* gray, int h, int w, int cap, int* n, float* xy, int counts[4]) {
  return guarded([&] {
    const char* op = "gmc_corners";
    if (h < 16 || w < 16 || h > 8192 || w > 8192) rt_bad(op, "a gray image of 16..8192 pixels a side");
    if (cap < 1000) rt_bad(op, "room for 1000 corners");
    need(gray, "gray"); need(n, "n"); need(xy, "xy"); need(counts, "counts"); need(ctx, "ctx");
    gtx::op_gmc_corners(ctx, gray, h, w, n, xy, counts);
  });
}

int gtx_op_gmc_lk(gtx_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int h, int w, const float* pts, int n, float* next, int* status) {
  return guarded([&] {
    const char* op = "gmc_lk";
    if (h < 16 || w < 16 || h > 8192 || w > 8192) rt_bad(op, "gray images of 16..8192 pixels a side (every pyramid level at least two wide)");
    if (n < 0 || n > 1000) rt_bad(op, "0 <= n <= 1000 points");
    need(prev, "prev"); need(cur, "cur");
    if (n > 0) { need(pts, "pts"); need(next, "next"); need(status, "status"); }
    for (int i = 0; i < n; ++i) {
      const float x = pts[2 * i], y = pts[2 * i + 1];
      if (!(x >= 0.f && x <= (float)(w - 1) && y >= 0.f && y <= (float)(h - 1))) rt_bad(op, "a point outside the image (or not a number)");
    }
    need(ctx, "ctx");
    gtx::op_gmc_lk(ctx, prev, cur, h, w, pts, n, next, status);
  });
}

int gtx_op_gmc_ransac(gtx_ctx* ctx, const float* pairs, int n, uint32_t seed, int* best_count, int* winner, double model[4], int* count) {
  return guarded([&] {
    const char* op = "gmc_ransac";
    if (n < 0 || n > 1024) rt_bad(op, "0 <= n <= 1024 pairs (the compaction step's list)");
    if (n > 0) need(pairs, "pairs");
    for (int i = 0; i < 4 * n; ++i)
      if (!std::isfinite(pairs[i])) rt_bad(op, "a coordinate that is not a finite number");
    need(best_count, "best_count"); need(winner, "winner"); need(model, "model"); need(count, "count"); need(ctx, "ctx");
    gtx::op_gmc_ransac(ctx, pairs, n, seed, best_count, winner, model, count);
  });
}

struct gtx_fgmc {
  gtx_ctx* ctx;
  std::unique_ptr<gtx::FeatGmc> impl;
};

int gtx_fgmc_create(gtx_ctx* ctx, int frame_h, int frame_w, int max_features, int seed, gtx_fgmc** out) {
  return guarded([&] {
    need(ctx, "ctx"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<gtx_fgmc> g(new gtx_fgmc);
    g->ctx = ctx;
    g->impl.reset(new gtx::FeatGmc(ctx, frame_h, frame_w, max_features, seed));
    *out = g.release();
  });
}
void gtx_fgmc_destroy(gtx_fgmc* g) { delete g; }
int gtx_fgmc_reset(gtx_fgmc* g) {
  return guarded([&] { need(g, "gmc"); g->impl->reset(); });
}
int gtx_fgmc_restart(gtx_fgmc* g) {
  return guarded([&] { need(g, "gmc"); g->impl->restart(); });
}
int gtx_fgmc_submit_gray_dev(gtx_fgmc* g, const void* gray_dptr, int gh, int gw) {
  return guarded([&] { need(g, "gmc"); need(gray_dptr, "gray"); g->impl->submit_gray_dev(gray_dptr, gh, gw); });
}
int gtx_fgmc_submit_gray(gtx_fgmc* g, const uint8_t* gray, int gh, int gw) {
  return guarded([&] { need(g, "gmc"); need(gray, "gray"); g->impl->submit_gray(gray, gh, gw); });
}
int gtx_fgmc_submit_frame_dev(gtx_fgmc* g, const void* frame_bgr_dptr, int h, int w, int restart) {
  return guarded([&] { need(g, "gmc"); need(frame_bgr_dptr, "frame"); g->impl->submit_frame_dev(frame_bgr_dptr, h, w, restart != 0); });
}
int gtx_fgmc_collect(gtx_fgmc* g, double A[6], int* valid, int stats[3]) {
  return guarded([&] { need(g, "gmc"); need(A, "A"); g->impl->collect(A, valid, stats); });
}
int gtx_fgmc_pairs(gtx_fgmc* g, int cap, int* n, float* pairs4) {
  return guarded([&] { need(g, "gmc"); need(n, "n"); g->impl->debug_pairs(cap, n, pairs4); });
}
int gtx_fgmc_matches(gtx_fgmc* g, int cap, int* n_q, int* n_t, int* best_idx, int* best_d, int* second_d, float* q_xy, float* t_xy) {
  return guarded([&] { need(g, "gmc"); need(n_q, "n_q"); need(n_t, "n_t"); g->impl->debug_matches(cap, n_q, n_t, best_idx, best_d, second_d, q_xy, t_xy); });
}
int gtx_gray_half_dev(gtx_ctx* ctx, const void* frame_bgr_dptr, int h, int w, void* gray_dptr) {
  return guarded([&] {
    need(ctx, "ctx"); need(frame_bgr_dptr, "frame"); need(gray_dptr, "gray");
    if (h < 2 || w < 2) gtx::fail(GTX_ERR_INVALID, "gtx_gray_half_dev: frame %dx%d", w, h);
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::gmc_launch_gray_half(static_cast<const uint8_t*>(frame_bgr_dptr), w, static_cast<uint8_t*>(gray_dptr), h / 2, w / 2, ctx->stream);
    GTX_HIP(hipGetLastError());
  });
}

struct gtx_ecc {
  gtx_ctx* ctx;
  std::unique_ptr<gtx::Ecc> impl;
};

int gtx_ecc_create(gtx_ctx* ctx, int frame_h, int frame_w, int max_iters, double eps, gtx_ecc** out) {
  return guarded([&] {
    need(ctx, "ctx"); need(out, "out");
    GTX_HIP(hipSetDevice(ctx->device));
    std::unique_ptr<gtx_ecc> e(new gtx_ecc);
    e->ctx = ctx;
    e->impl.reset(new gtx::Ecc(ctx->device, ctx->stream, frame_h, frame_w, max_iters, eps));
    *out = e.release();
  });
}
void gtx_ecc_destroy(gtx_ecc* e) { delete e; }
int gtx_ecc_reset(gtx_ecc* e) {
  return guarded([&] { need(e, "ecc"); e->impl->reset(); });
}
int gtx_ecc_replace_template(gtx_ecc* e, int replace) {
  return guarded([&] { need(e, "ecc"); e->impl->set_replace_template(replace != 0); });
}
int gtx_ecc_exact_positions(gtx_ecc* e, int exact) {
  return guarded([&] { need(e, "ecc"); e->impl->set_exact_positions(exact != 0); });
}
int gtx_ecc_submit(gtx_ecc* e, const uint8_t* frame_bgr, int h, int w) {
  return guarded([&] { need(e, "ecc"); need(frame_bgr, "frame"); e->impl->submit_frame(frame_bgr, h, w); });
}
int gtx_ecc_submit_dev(gtx_ecc* e, gtx_ctx* producer, const void* frame_bgr_dptr, int h, int w) {
  return guarded([&] {
    need(e, "ecc"); need(frame_bgr_dptr, "frame");
    if (producer && producer->device != e->ctx->device) gtx::fail(-1, "gtx_ecc_submit_dev: the producer's context is on another device");
    e->impl->submit_frame_dev(frame_bgr_dptr, h, w, producer ? producer->stream : e->ctx->stream);
  });
}
int gtx_ecc_collect(gtx_ecc* e, double A[6], int info[2], double* rho) {
  return guarded([&] { need(e, "ecc"); need(A, "A"); e->impl->collect(A, info, rho); });
}
int gtx_ecc_image(gtx_ecc* e, int which, float* out) {
  return guarded([&] { need(e, "ecc"); need(out, "out"); e->impl->debug_image(which, out); });
}

struct gtx_sift {
  gtx_ctx* ctx;
  std::unique_ptr<gtx::Sift> impl;
};

int gtx_register_images(gtx_ctx* ctx, const gtx_reg_config* cfg, const uint8_t* src, int sh, int sw, const uint8_t* dst, int dh, int dw,
                        double H[9], int* valid, int stats[4], float timings_ms[4]) {
  return guarded([&] {
    need(ctx, "ctx"); need(cfg, "cfg"); need(src, "src"); need(dst, "dst"); need(H, "H"); need(valid, "valid"); need(stats, "stats");
    gtx::register_images(ctx, *cfg, src, sh, sw, dst, dh, dw, H, valid, stats, timings_ms);
  });
}
int gtx_sift_create(gtx_ctx* ctx, int max_h, int max_w, gtx_sift** out) {
  return guarded([&] {
    need(ctx, "ctx"); need(out, "out");
    std::unique_ptr<gtx_sift> s(new gtx_sift);
    s->ctx = ctx;
    s->impl.reset(new gtx::Sift(ctx->device, ctx->stream, max_h, max_w));
    *out = s.release();
  });
}
void gtx_sift_destroy(gtx_sift* s) { delete s; }
int gtx_sift_detect(gtx_sift* s, const uint8_t* image, int h, int w, int max_features, int root, float root_eps, int cap, int* n,
                    float* kp5, int* octave, float* desc) {
  return guarded([&] {
    need(s, "sift"); need(image, "image"); need(n, "n");
    s->impl->detect_and_compute(image, h, w, max_features, root != 0, root_eps);
    std::vector<gtx::SiftKeypoint> k;
    std::vector<float> d;
    s->impl->download(k, d);
    *n = (int)k.size();
    const int m = std::min<int>(cap, (int)k.size());
    for (int i = 0; i < m; ++i) {
      if (kp5) { kp5[5 * i] = k[i].x; kp5[5 * i + 1] = k[i].y; kp5[5 * i + 2] = k[i].size; kp5[5 * i + 3] = k[i].angle; kp5[5 * i + 4] = k[i].response; }
      if (octave) octave[i] = k[i].octave;
    }
    if (desc && m > 0) std::memcpy(desc, d.data(), (size_t)m * 128 * sizeof(float));
  });
}
int gtx_sift_stage_ms(gtx_sift* s, float out[4]) {
  return guarded([&] { need(s, "sift"); need(out, "out"); s->impl->stage_ms(out); });
}
int gtx_sift_pyramid(gtx_sift* s, int kind, int octave, int layer, int cap, float* out, int* h, int* w, int* n_octaves) {
  return guarded([&] {
    need(s, "sift"); need(h, "h"); need(w, "w");
    if (n_octaves) *n_octaves = s->impl->n_octaves();
    std::vector<float> img;
    s->impl->pyramid_image(kind, octave, layer, img, h, w);
    if (out) {
      if ((size_t)cap < img.size()) gtx::fail(GTX_ERR_INVALID, "pyramid image has %zu pixels, buffer holds %d", img.size(), cap);
      std::memcpy(out, img.data(), img.size() * sizeof(float));
    }
  });
}

int gtx_op_match_2nn(gtx_ctx* ctx, const float* query, int nq, const float* train, int nt, int* idx1, int* idx2, float* d1,
                     float* d2, int iters, float* ms_per_pass) {
  return guarded([&] {
    need(ctx, "ctx"); need(query, "query"); need(train, "train"); need(idx1, "idx1"); need(idx2, "idx2"); need(d1, "d1"); need(d2, "d2");
    if (nq < 0 || nt < 0) gtx::fail(GTX_ERR_INVALID, "negative descriptor count");
    GTX_HIP(hipSetDevice(ctx->device));
    if (nq == 0) return;
    hipStream_t s = ctx->stream;
    const size_t qn = (size_t)nq * 128, tn = (size_t)std::max(nt, 1) * 128;
    gtx::DevBuf qf(qn * 4), tf(tn * 4), qh(qn * 2), th(tn * 2), ws(gtx::match2nn_workspace_bytes(nq, nt));
    gtx::DevBuf i1(nq * 4), i2(nq * 4), e1(nq * 4), e2(nq * 4);
    GTX_HIP(hipMemcpy(qf.p, query, qn * 4, hipMemcpyHostToDevice));
    if (nt > 0) GTX_HIP(hipMemcpy(tf.p, train, (size_t)nt * 128 * 4, hipMemcpyHostToDevice));
    gtx::descriptors_to_half(qf.as<float>(), qh.p, qn, s);
    gtx::descriptors_to_half(tf.as<float>(), th.p, (size_t)nt * 128, s);
    gtx::match2nn(qh.p, qf.as<float>(), nq, th.p, tf.as<float>(), nt, ws.p, i1.as<int>(), i2.as<int>(), e1.as<float>(), e2.as<float>(), s);
    GTX_HIP(hipStreamSynchronize(s));
    if (iters > 0 && ms_per_pass) {
      hipEvent_t a, b;
      GTX_HIP(hipEventCreate(&a)); GTX_HIP(hipEventCreate(&b));
      GTX_HIP(hipEventRecord(a, s));
      for (int i = 0; i < iters; ++i)
        gtx::match2nn(qh.p, qf.as<float>(), nq, th.p, tf.as<float>(), nt, ws.p, i1.as<int>(), i2.as<int>(), e1.as<float>(), e2.as<float>(), s);
      GTX_HIP(hipEventRecord(b, s));
      GTX_HIP(hipEventSynchronize(b));
      float ms = 0.f;
      GTX_HIP(hipEventElapsedTime(&ms, a, b));
      *ms_per_pass = ms / iters;
      (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    }
    GTX_HIP(hipMemcpy(idx1, i1.p, nq * 4, hipMemcpyDeviceToHost));
    GTX_HIP(hipMemcpy(idx2, i2.p, nq * 4, hipMemcpyDeviceToHost));
    GTX_HIP(hipMemcpy(d1, e1.p, nq * 4, hipMemcpyDeviceToHost));
    GTX_HIP(hipMemcpy(d2, e2.p, nq * 4, hipMemcpyDeviceToHost));
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
    gtx::DevBuf df(fb), di(ib), dg;
    if (out_gray) dg.alloc((size_t)gray_h * gray_w);
    GTX_HIP(hipMemcpy(df.p, frame, fb, hipMemcpyHostToDevice));
    gtx::launch_preprocess(dtype, df.as<uint8_t>(), 1, lb, di.p, out_gray ? dg.as<uint8_t>() : nullptr, gray_h, gray_w, ctx->stream);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    // The network's view of the image (what the stem kernels make of the bytes through their tables): byte / 255 in fp32,
    // rounded to fp16 for dtype f16.
    std::vector<uint8_t> raw(ib);
    GTX_HIP(hipMemcpy(raw.data(), di.p, ib, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npx * 4; ++i) {
      const float f = (float)raw[i] / 255.f;
      if (dtype == gtx::DT_F16) static_cast<_Float16*>(out_img)[i] = (_Float16)f;
      else static_cast<float*>(out_img)[i] = f;
    }
    if (out_gray) GTX_HIP(hipMemcpy(out_gray, dg.p, (size_t)gray_h * gray_w, hipMemcpyDeviceToHost));
  });
}

/* ------------------------------------------------------------------ detector */

int gtx_detector_create(gtx_ctx* ctx, const gtx_det_config* cfg, gtx_detector** out) {
  return guarded([&] {
    need(cfg, "cfg"); need(out, "out");
    // the class filter is a two-word mask: class 128 would shift past it. The YOLO path already refuses nc > 128 when it builds its
    // head (net_runtime.cpp); RT-DETR had no such check, so for it this one is new
    if (cfg->nc < 1 || cfg->nc > 128) gtx::fail(GTX_ERR_UNSUPPORTED, "gtx_det_config.nc %d: 1..128 classes", cfg->nc);
    need(ctx, "ctx");
    std::unique_ptr<gtx_detector> d(new gtx_detector);
    if (cfg->arch == 1 && cfg->end2end) gtx::fail(-3, "gtx_det_config.end2end: the one-to-one head belongs to YOLOv10 (arch 0); RT-DETR has no NMS to leave out");
    if (cfg->arch == 1) d->impl.reset(new gtx::RtDetr(ctx, *cfg));
    else if (cfg->arch == 0) d->impl.reset(new gtx::Detector(ctx, *cfg));
    else gtx::fail(-3, "gtx_det_config.arch %d: 0 (YOLOv8) or 1 (RT-DETR)", cfg->arch);
    *out = d.release();
  });
}
void gtx_detector_destroy(gtx_detector* det) { delete det; }

int gtx_detector_set_tensor(gtx_detector* det, const char* name, const float* data, int ndim, const int64_t* shape) {
  return guarded([&] {
    need(det, "det"); need(name, "name"); need(data, "data"); need(shape, "shape");
    det->impl->set_tensor(name, data, ndim, shape);
  });
}
int gtx_detector_finalize(gtx_detector* det) {
  return guarded([&] { need(det, "det"); det->impl->finalize(); });
}
int gtx_detector_input_size(gtx_detector* det, int* net_h, int* net_w) {
  return guarded([&] { need(det, "det"); need(net_h, "net_h"); need(net_w, "net_w"); det->impl->input_size(net_h, net_w); });
}
int gtx_detector_detect(gtx_detector* det, const uint8_t* frame_bgr, int h, int w, int* n_out, float* xyxy,
                        float* conf, int* cls, float speed_ms[3]) {
  return guarded([&] {
    need(det, "det"); need(frame_bgr, "frame"); need(n_out, "n_out"); need(xyxy, "xyxy"); need(conf, "conf"); need(cls, "cls");
    det->impl->live()->detect_host(frame_bgr, h, w, n_out, xyxy, conf, cls, speed_ms);
  });
}
int gtx_detector_detect_dev(gtx_detector* det, const void* frame_dptr, int h, int w, int* n_out, float* xyxy,
                            float* conf, int* cls, float speed_ms[3]) {
  return guarded([&] {
    need(det, "det"); need(frame_dptr, "frame"); need(n_out, "n_out"); need(xyxy, "xyxy"); need(conf, "conf"); need(cls, "cls");
    det->impl->live()->detect_dev(frame_dptr, 1, h, w, n_out, xyxy, conf, cls, speed_ms);
  });
}
int gtx_detector_detect_batch_dev(gtx_detector* det, const void* frames_dptr, int nb, int h, int w, int* n_out,
                                  float* xyxy, float* conf, int* cls, float speed_ms[3]) {
  return guarded([&] {
    need(det, "det"); need(frames_dptr, "frames"); need(n_out, "n_out"); need(xyxy, "xyxy"); need(conf, "conf"); need(cls, "cls");
    det->impl->live()->detect_dev(frames_dptr, nb, h, w, n_out, xyxy, conf, cls, speed_ms);
  });
}
int gtx_detector_submit_dev(gtx_detector* det, const void* frames_dptr, int nb, int h, int w) {
  return guarded([&] { need(det, "det"); need(frames_dptr, "frames"); det->impl->live()->submit_dev(frames_dptr, nb, h, w); });
}
int gtx_detector_collect(gtx_detector* det, int* n_out, float* xyxy, float* conf, int* cls, float speed_ms[3]) {
  return guarded([&] {
    need(det, "det"); need(n_out, "n_out"); need(xyxy, "xyxy"); need(conf, "conf"); need(cls, "cls");
    det->impl->live()->collect(n_out, xyxy, conf, cls, speed_ms);
  });
}
const void* gtx_detector_gray(gtx_detector* det, int b, int* gray_h, int* gray_w) {
  if (!det) return nullptr;
  return det->impl->live()->gray(b, gray_h, gray_w);
}
int gtx_detector_raw_output(gtx_detector* det, int b, float* out, int* n_anchors) {
  return guarded([&] { need(det, "det"); need(out, "out"); det->impl->live()->raw_output(b, out, n_anchors); });
}
int gtx_detector_raw_logits(gtx_detector* det, int b, float* out, int* n_anchors) {
  return guarded([&] { need(det, "det"); need(out, "out"); det->impl->live()->raw_output(b, out, n_anchors, true); });
}
int gtx_detector_layer_output(gtx_detector* det, int b, const char* layer, float* out, int* h, int* w, int* c) {
  return guarded([&] { need(det, "det"); need(layer, "layer"); det->impl->live()->layer_output(b, layer, out, h, w, c); });
}
int gtx_detector_saturated(gtx_detector* det, int clear, int* flag) {
  return guarded([&] { need(det, "det"); need(flag, "flag"); *flag = det->impl->saturated(clear != 0) ? 1 : 0; });
}
int gtx_detector_fell_back(gtx_detector* det, int* fell_back) {
  return guarded([&] { need(det, "det"); need(fell_back, "fell_back"); *fell_back = det->impl->fell_back() ? 1 : 0; });
}
int gtx_detector_pad_skip(gtx_detector* det, int* on, int* skipped, int* total) {
  return guarded([&] { need(det, "det"); det->impl->pad_skip(on, skipped, total); });
}
int gtx_detector_sparse_box(gtx_detector* det, int* on, int* overflows) {
  return guarded([&] { need(det, "det"); det->impl->sparse_box(on, overflows); });
}
int gtx_detector_features(gtx_detector* det, int b, float* out, int cap, int* n, int* dim) {
  return guarded([&] { need(det, "det"); det->impl->live()->features(b, out, cap, n, dim); });
}
int gtx_detector_trace(gtx_detector* det, int every_n) {
  return guarded([&] { need(det, "det"); det->impl->live()->set_trace(every_n); });
}
int gtx_detector_profile(gtx_detector* det, int nb, int iters, int cap, char* names, int* launches, float* total_ms,
                         double* flops, double* bytes, int* n_families) {
  return guarded([&] {
    need(det, "det"); need(names, "names"); need(launches, "launches"); need(total_ms, "total_ms");
    need(flops, "flops"); need(bytes, "bytes"); need(n_families, "n_families");
    std::vector<std::string> nm;
    std::vector<int> la;
    std::vector<float> ms;
    std::vector<double> fl, by;
    if (iters <= 0) det->impl->live()->trace_report(nm, la, ms, fl, by);   // iters = 0: the live trace totals
    else det->impl->live()->profile(nb, iters, nm, la, ms, fl, by);
    const int n = std::min<int>(cap, (int)nm.size());
    for (int i = 0; i < n; ++i) {
      std::strncpy(names + (size_t)i * 96, nm[i].c_str(), 95);
      names[(size_t)i * 96 + 95] = 0;
      launches[i] = la[i]; total_ms[i] = ms[i]; flops[i] = fl[i]; bytes[i] = by[i];
    }
    *n_families = n;
  });
}

/* ------------------------------------------------------------------ tracker */

int gtx_tracker_create(const gtx_tracker_config* cfg, gtx_tracker** out) {
  return guarded([&] {
    need(cfg, "cfg"); need(out, "out");
    std::unique_ptr<gtx_tracker> t(new gtx_tracker);
    if (cfg->type == 2 || cfg->type == 3) t->oc.reset(new gtx::OcSortTracker(*cfg));
    else if (cfg->type == 0 || cfg->type == 1 || cfg->type == 4) t->impl.reset(new gtx::ByteTracker(*cfg));
    else if (cfg->type == 5) t->tt.reset(new gtx::TrackTrackTracker(*cfg));
    else gtx::fail(GTX_ERR_INVALID, "tracker type %d (0 bytetrack, 1 botsort, 2 ocsort, 3 deepocsort, 4 fasttrack, 5 tracktrack)", cfg->type);
    *out = t.release();
  });
}
void gtx_tracker_destroy(gtx_tracker* trk) { delete trk; }
int gtx_tracker_reset(gtx_tracker* trk) {
  return guarded([&] { need(trk, "trk"); if (trk->oc) trk->oc->reset(); else if (trk->tt) trk->tt->reset(); else trk->impl->reset(); });
}
int gtx_tracker_update(gtx_tracker* trk, int n, const float* xyxy, const float* conf, const int* cls,
                       const double* gmc_affine, int cap, int* n_out, float* out_xyxy, int* out_id, float* out_score,
                       int* out_cls, int* out_det_idx) {
  return guarded([&] {
    need(trk, "trk"); need(n_out, "n_out");
    if (n > 0) { need(xyxy, "xyxy"); need(conf, "conf"); need(cls, "cls"); }
    if (trk->oc) trk->oc->update(n, xyxy, conf, cls, gmc_affine, cap, n_out, out_xyxy, out_id, out_score, out_cls, out_det_idx);
    else if (trk->tt) trk->tt->update(n, xyxy, conf, cls, gmc_affine, cap, n_out, out_xyxy, out_id, out_score, out_cls, out_det_idx);
    else trk->impl->update(n, xyxy, conf, cls, gmc_affine, cap, n_out, out_xyxy, out_id, out_score, out_cls, out_det_idx);
  });
}

int gtx_tracker_update_feats(gtx_tracker* trk, int n, const float* xyxy, const float* conf, const int* cls, const double* gmc_affine,
                             const float* feats, int feat_dim, int cap, int* n_out, float* out_xyxy, int* out_id, float* out_score,
                             int* out_cls, int* out_det_idx) {
  return guarded([&] {
    need(trk, "trk"); need(n_out, "n_out");
    if (n > 0) { need(xyxy, "xyxy"); need(conf, "conf"); need(cls, "cls"); }
    if (trk->oc) trk->oc->update(n, xyxy, conf, cls, gmc_affine, cap, n_out, out_xyxy, out_id, out_score, out_cls, out_det_idx, feats, feat_dim);
    else if (trk->tt) trk->tt->update(n, xyxy, conf, cls, gmc_affine, cap, n_out, out_xyxy, out_id, out_score, out_cls, out_det_idx, feats, feat_dim);
    else trk->impl->update(n, xyxy, conf, cls, gmc_affine, cap, n_out, out_xyxy, out_id, out_score, out_cls, out_det_idx, feats, feat_dim);
  });
}

int gtx_tracker_replay(gtx_tracker* trk, const double* recs, int n_recs, int stride, int max_det, int with_gmc, int row_cap,
                       int* rows_per_frame, float* row_xyxy, int* row_id, float* row_score, int* row_cls, int* row_det_idx) {
  return guarded([&] {
    need(trk, "trk"); need(rows_per_frame, "rows_per_frame");
    if (n_recs > 0) need(recs, "recs");
    if (row_cap > 0) {          // every row array is written unconditionally below
      need(row_xyxy, "row_xyxy"); need(row_id, "row_id"); need(row_score, "row_score"); need(row_cls, "row_cls"); need(row_det_idx, "row_det_idx");
    }
    const int tail = (with_gmc ? 7 : 0) + 10;
    if (max_det < 0 || stride != 1 + 6 * max_det + tail) gtx::fail(GTX_ERR_INVALID, "replay: stride %d does not match max_det %d", stride, max_det);
    std::vector<float> xyxy((size_t)4 * std::max(max_det, 1)), conf(std::max(max_det, 1));
    std::vector<int> cls(std::max(max_det, 1));
    int used = 0;
    for (int f = 0; f < n_recs; ++f) {
      const double* rec = recs + (size_t)f * stride;
      if (!std::isfinite(rec[0])) gtx::fail(GTX_ERR_INVALID, "replay: record %d has a non-finite detection count", f);
      const int n = (int)std::min(std::max(rec[0], 0.0), (double)max_det);
      for (int i = 0; i < n; ++i) {
        const double* d = rec + 1 + 6 * i;
        xyxy[4 * i] = (float)d[0]; xyxy[4 * i + 1] = (float)d[1]; xyxy[4 * i + 2] = (float)d[2]; xyxy[4 * i + 3] = (float)d[3];
        conf[i] = (float)d[4];
        cls[i] = (int)d[5];
      }
      const double* gmc = (with_gmc && rec[stride - 17] > 0) ? rec + stride - 16 : nullptr;
      int k = 0;
      const int room = row_cap - used;
      float* ox = row_xyxy + (size_t)4 * used;
      if (room <= 0 && n > 0) gtx::fail(GTX_ERR_INVALID, "replay: more than %d track rows", row_cap);
      if (trk->oc)
        trk->oc->update(n, xyxy.data(), conf.data(), cls.data(), gmc, room, &k, ox, row_id + used, row_score + used, row_cls + used, row_det_idx + used);
      else if (trk->tt)
        trk->tt->update(n, xyxy.data(), conf.data(), cls.data(), gmc, room, &k, ox, row_id + used, row_score + used, row_cls + used, row_det_idx + used);
      else
        trk->impl->update(n, xyxy.data(), conf.data(), cls.data(), gmc, room, &k, ox, row_id + used, row_score + used, row_cls + used, row_det_idx + used);
      rows_per_frame[f] = k;
      used += k;
    }
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

/* ------------------------------------------------------------------ stabilizer */

int gtx_stabilizer_create(gtx_ctx* ctx, const gtx_stab_config* cfg, gtx_stabilizer** out) {
  return guarded([&] {
    need(ctx, "ctx"); need(cfg, "cfg"); need(out, "out");
    std::unique_ptr<gtx_stabilizer> s(new gtx_stabilizer);
    s->impl.reset(new gtx::Stabilizer(ctx, *cfg));
    *out = s.release();
  });
}
void gtx_stabilizer_destroy(gtx_stabilizer* st) { delete st; }
int gtx_stabilizer_set_ref_frame(gtx_stabilizer* st, const uint8_t* frame_bgr, int h, int w, const float* boxes_xywh, int n) {
  return guarded([&] { need(st, "st"); need(frame_bgr, "frame"); st->impl->set_ref_frame(frame_bgr, h, w, boxes_xywh, n); });
}
int gtx_stabilizer_set_ref_gray_dev(gtx_stabilizer* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n) {
  return guarded([&] { need(st, "st"); need(gray_dptr, "gray"); st->impl->set_ref_gray_dev(gray_dptr, gh, gw, boxes_xywh, n); });
}
int gtx_stabilizer_stabilize(gtx_stabilizer* st, const uint8_t* frame_bgr, int h, int w, const float* boxes_xywh, int n,
                             double H[9], int* valid, int stats[4]) {
  return guarded([&] {
    need(st, "st"); need(frame_bgr, "frame"); need(H, "H"); need(valid, "valid");
    st->impl->stabilize(frame_bgr, h, w, boxes_xywh, n, H, valid, stats);
  });
}
int gtx_stabilizer_stabilize_gray_dev(gtx_stabilizer* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh,
                                      int n, double H[9], int* valid, int stats[4]) {
  return guarded([&] {
    need(st, "st"); need(gray_dptr, "gray"); need(H, "H"); need(valid, "valid");
    st->impl->stabilize_gray_dev(gray_dptr, gh, gw, boxes_xywh, n, H, valid, stats);
  });
}
int gtx_stabilizer_promote_cur(gtx_stabilizer* st) {
  return guarded([&] { need(st, "st"); st->impl->promote_cur_to_ref(); });
}
int gtx_stabilizer_submit_gray_dev(gtx_stabilizer* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n) {
  return guarded([&] { need(st, "st"); need(gray_dptr, "gray"); st->impl->submit_gray_dev(gray_dptr, gh, gw, boxes_xywh, n); });
}
int gtx_stabilizer_collect(gtx_stabilizer* st, double H[9], int* valid, int stats[4]) {
  return guarded([&] { need(st, "st"); need(H, "H"); need(valid, "valid"); st->impl->collect(H, valid, stats); });
}
int gtx_stabilizer_keypoints(gtx_stabilizer* st, int which, int cap, int* n, float* xy, int* level, int* angle_bin, uint8_t* desc) {
  return guarded([&] { need(st, "st"); need(n, "n"); st->impl->keypoints(which, cap, n, xy, level, angle_bin, desc); });
}
int gtx_stabilizer_matches(gtx_stabilizer* st, int cap, int* n, int* cur_idx, int* ref_idx, int* dist) {
  return guarded([&] { need(st, "st"); need(n, "n"); st->impl->matches(cap, n, cur_idx, ref_idx, dist); });
}

int gtx_stabilizer_last_ms(gtx_stabilizer* st, float* ms) {
  return guarded([&] { need(st, "st"); need(ms, "ms"); *ms = st->impl->last_ms(); });
}

int gtx_stabilizer_keep_pass(gtx_stabilizer* st, int on) {
  return guarded([&] { need(st, "st"); st->impl->keep_pass(on != 0); });
}
int gtx_stabilizer_level(gtx_stabilizer* st, int which, int i, int* h, int* w, uint8_t* out, int64_t cap) {
  return guarded([&] {
    need(st, "st"); need(h, "h"); need(w, "w");
    if (cap < 0) gtx::fail(GTX_ERR_INVALID, "stabilizer level: negative cap");
    st->impl->level(which, i, h, w, out, (size_t)cap);
  });
}
int gtx_stabilizer_candidates(gtx_stabilizer* st, int which, int i, int cap, int* n, int* pix, int* score, int* n_elig, int* n_kp, int* n_dropped) {
  return guarded([&] { need(st, "st"); need(n, "n"); st->impl->candidates(which, i, cap, n, pix, score, n_elig, n_kp, n_dropped); });
}

// ---- the stabilizer's matcher and RANSAC kernel, one launch each (tests/test_orb_ops_gpu.py). As for the hooks above: sizes are
// checked before anything touches the GPU.
int gtx_op_orb_match(gtx_ctx* ctx, const uint8_t* desc_q, int nq, int slots_q, const uint8_t* desc_t, int nt, int slots_t, float ratio, int keep_all,
                     const float* xy_q, const float* xy_t, int* best_idx, int* best_d, int* second_d, int* m_q, int* m_t, int* m_d, float* m_pts,
                     int* n_match) {
  return guarded([&] {
    const char* op = "orb_match";
    if (nq < 1 || nt < 0 || slots_q < nq || slots_t < std::max(nt, 1) || slots_q > (1 << 16) || slots_t > (1 << 20)) rt_bad(op, "1 <= nq <= slots_q <= 65536, 0 <= nt <= slots_t <= 2^20, slots_t >= 1");
    if ((double)gtx::cdiv(slots_t, 256) * slots_q > 6.4e7) rt_bad(op, "the per-chunk partials would pass 768 MB");
    if (!(ratio >= 0.f && ratio <= 4.f)) rt_bad(op, "ratio in [0, 4]");
    need(desc_q, "desc_q"); need(xy_q, "xy_q");
    if (nt > 0) { need(desc_t, "desc_t"); need(xy_t, "xy_t"); }
    need(best_idx, "best_idx"); need(best_d, "best_d"); need(second_d, "second_d"); need(m_q, "m_q"); need(m_t, "m_t"); need(m_d, "m_d");
    need(m_pts, "m_pts"); need(n_match, "n_match"); need(ctx, "ctx");
    gtx::op_orb_match(ctx, desc_q, nq, slots_q, desc_t, nt, slots_t, ratio, keep_all != 0, xy_q, xy_t, best_idx, best_d, second_d, m_q, m_t, m_d, m_pts,
                      n_match);
  });
}

int gtx_op_orb_ransac(gtx_ctx* ctx, const float* pts, int n, uint32_t seed, int n_hyp, int frame_w, int frame_h, float thr, int affine, int* best,
                      int64_t* cost, double H[9]) {
  return guarded([&] {
    const char* op = "orb_ransac";
    if (n < 0 || n > (1 << 20)) rt_bad(op, "0 <= n <= 2^20 point pairs");
    if (n_hyp < 1 || n_hyp > 65536) rt_bad(op, "1..65536 hypotheses (the winner's index has 16 bits of the key)");
    if (frame_w < 1 || frame_h < 1 || frame_w > (1 << 16) || frame_h > (1 << 16)) rt_bad(op, "bad frame size");
    if (!(thr > 0.f && thr <= 64.f)) rt_bad(op, "threshold in (0, 64] px (a match costs at most thr^2 * 1024, the sum has 47 bits)");
    if (affine != 0 && affine != 1) rt_bad(op, "affine is 0 or 1");
    if (n > 0) need(pts, "pts");
    need(best, "best"); need(cost, "cost"); need(H, "H"); need(ctx, "ctx");
    long long c = 0;
    gtx::op_orb_ransac(ctx, pts, n, seed, n_hyp, frame_w, frame_h, thr, affine, best, &c, H);
    *cost = c;
  });
}

int gtx_stabilizer_pattern(gtx_stabilizer* st, int8_t* out) {
  return guarded([&] {
    need(out, "out");
    if (st) { st->impl->pattern(out); return; }
    std::vector<int8_t> t;                        // no object: the built-in table (host only, needs no device)
    gtx::stabilizer_pattern_table(t);
    std::memcpy(out, t.data(), t.size());
  });
}

/* ------------------------------------------------------------------ geometry */

int gtx_warp_boxes(const double H[9], const float* xywh_in, int n, float* xywh_out) {
  return guarded([&] {
    need(H, "H");
    if (n > 0) { need(xywh_in, "xywh_in"); need(xywh_out, "xywh_out"); }
    gtx::warp_boxes(H, xywh_in, n, xywh_out);
  });
}
int gtx_perspective_points(const double H[9], const double* x, const double* y, int n, double* ox, double* oy) {
  return guarded([&] {
    need(H, "H");
    if (n > 0) { need(x, "x"); need(y, "y"); need(ox, "ox"); need(oy, "oy"); }
    gtx::perspective_points(H, x, y, n, ox, oy);
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
int gtx_op_georef_points(gtx_ctx* ctx, const gtx_georef_chain* chain, const double* x, const double* y, int n,
                         double* ortho_x, double* ortho_y, double* lat, double* lon, double* east, double* north) {
  return guarded([&] {
    need(ctx, "ctx"); need(chain, "chain");
    if (n > 0) { need(x, "x"); need(y, "y"); }
    gtx::georef_points(ctx, *chain, x, y, n, ortho_x, ortho_y, lat, lon, east, north);
  });
}
int gtx_yuv420_to_bgr_dev(gtx_ctx* ctx, const void* yuv_dptr, int h, int w, void* bgr_dptr) {
  return guarded([&] {
    need(ctx, "ctx"); need(yuv_dptr, "yuv"); need(bgr_dptr, "bgr");
    gtx::yuv420_to_bgr_dev(ctx, yuv_dptr, h, w, bgr_dptr);
  });
}

size_t gtx_jpeg_record_bound(int h, int w) {
  return (h <= 0 || w <= 0 || h > gtx::jpeg::kMaxDim || w > gtx::jpeg::kMaxDim) ? 0 : gtx::jpeg::record_bound(h, w);
}

int gtx_jpeg_parse(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs, void* record, size_t capacity,
                   size_t* needed) {
  int rc = 0;
  const int st = guarded([&] {
    need(bytes, "bytes"); need(needed, "needed");
    if (!record && capacity) gtx::fail(GTX_ERR_INVALID, "jpeg_parse: record is NULL with a capacity of %zu", capacity);
    gtx::jpeg::Info info;
    char msg[512];
    rc = gtx::jpeg::parse(static_cast<const uint8_t*>(bytes), n, (long long)frame, &info, record, capacity, needed, msg, sizeof msg);
    if (h) *h = info.height;
    if (w) *w = info.width;
    if (ncomp) *ncomp = info.ncomp;
    if (hs) *hs = info.hs;
    if (vs) *vs = info.vs;
    if (rc < 0) gtx::fail(rc, "%s", msg);
  });
  return st != GTX_OK ? st : rc;
}

int gtx_jpeg_probe(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs) {
  return guarded([&] {
    need(bytes, "bytes");
    gtx::jpeg::Info info;
    char msg[512];
    const int rc = gtx::jpeg::probe(static_cast<const uint8_t*>(bytes), n, (long long)frame, &info, msg, sizeof msg);
    if (h) *h = info.height;
    if (w) *w = info.width;
    if (ncomp) *ncomp = info.ncomp;
    if (hs) *hs = info.hs;
    if (vs) *vs = info.vs;
    if (rc < 0) gtx::fail(rc, "%s", msg);
  });
}

int gtx_jpeg_decode_dev(gtx_ctx* ctx, const void* record, size_t bytes, int h, int w, void* bgr_dptr) {
  return guarded([&] {
    need(record, "record");
    char msg[256];
    if (gtx::jpeg::check_record(record, bytes, h, w, msg, sizeof msg) != 0) gtx::fail(GTX_ERR_INVALID, "%s", msg);
    need(ctx, "ctx"); need(bgr_dptr, "bgr");
    gtx::jpeg::RecordHeader hd;
    memcpy(&hd, record, sizeof hd);
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf d_rec(bytes), d_planes(gtx::jpeg::planes_bytes(hd));
    GTX_HIP(hipMemcpyAsync(d_rec.p, record, bytes, hipMemcpyHostToDevice, ctx->stream));
    gtx::jpeg_decode_launch(ctx, d_rec.p, hd, d_planes.p, bgr_dptr);
    GTX_HIP(hipStreamSynchronize(ctx->stream));                 // the scratch buffers go out of scope here
  });
}

int gtx_jpeg_kernel_ms(gtx_ctx* ctx, const void* record, size_t bytes, int h, int w, void* bgr_dptr, const void* yuv_dptr, int reps, float ms[3]) {
  return guarded([&] {
    need(record, "record"); need(ms, "ms");
    char msg[256];
    if (gtx::jpeg::check_record(record, bytes, h, w, msg, sizeof msg) != 0) gtx::fail(GTX_ERR_INVALID, "%s", msg);
    if (reps < 1 || reps > 10000) gtx::fail(GTX_ERR_INVALID, "jpeg_kernel_ms: %d repetitions", reps);
    need(ctx, "ctx"); need(bgr_dptr, "bgr");
    gtx::jpeg::RecordHeader hd;
    memcpy(&hd, record, sizeof hd);
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf d_rec(bytes), d_planes(gtx::jpeg::planes_bytes(hd));
    GTX_HIP(hipMemcpyAsync(d_rec.p, record, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipEvent_t e[4];
    for (auto& x : e) GTX_HIP(hipEventCreate(&x));
    double sum[3] = {0, 0, 0};
    try {
      for (int r = -1; r < reps; ++r) {                          // one untimed pass first
        GTX_HIP(hipEventRecord(e[0], ctx->stream));
        gtx::jpeg_decode_launch(ctx, d_rec.p, hd, d_planes.p, bgr_dptr, e[1]);
        GTX_HIP(hipEventRecord(e[2], ctx->stream));
        if (yuv_dptr) gtx::yuv420_to_bgr_dev(ctx, yuv_dptr, h, w, bgr_dptr);
        GTX_HIP(hipEventRecord(e[3], ctx->stream));
        GTX_HIP(hipEventSynchronize(e[3]));
        if (r < 0) continue;
        for (int k = 0; k < 3; ++k) {
          float t = 0;
          GTX_HIP(hipEventElapsedTime(&t, e[k], e[k + 1]));
          sum[k] += t;
        }
      }
    } catch (...) {
      for (auto x : e) (void)hipEventDestroy(x);
      throw;
    }
    for (auto x : e) (void)hipEventDestroy(x);
    for (int k = 0; k < 3; ++k) ms[k] = (float)(sum[k] / reps);
    if (!yuv_dptr) ms[2] = 0.f;
  });
}

int gtx_warp_frame_dev(gtx_ctx* ctx, const void* src_dptr, int h, int w, const double H[9], void* dst_dptr) {
  return guarded([&] {
    need(ctx, "ctx"); need(src_dptr, "src"); need(H, "H"); need(dst_dptr, "dst");
    if (src_dptr == dst_dptr) gtx::fail(GTX_ERR_INVALID, "warp_frame: source and destination must be distinct buffers");
    gtx::warp_frame_dev(ctx, src_dptr, h, w, H, dst_dptr);
  });
}

int gtx_op_clahe(gtx_ctx* ctx, const uint8_t* gray, int h, int w, uint8_t* out) {
  return guarded([&] {
    need(ctx, "ctx"); need(gray, "gray"); need(out, "out");
    gtx::clahe_image(ctx, gray, h, w, out);
  });
}

int gtx_warp_frame(gtx_ctx* ctx, const uint8_t* src_bgr, int h, int w, const double H[9], uint8_t* dst_bgr) {
  return guarded([&] {
    need(ctx, "ctx"); need(src_bgr, "src"); need(H, "H"); need(dst_bgr, "dst");
    gtx::warp_frame(ctx, src_bgr, h, w, H, dst_bgr);
  });
}

}  // extern "C"
