// C ABI of libgtx.so (see include/gtx.h): the product's objects (context, device memory, detector, tracker, stabilizer, GMC, ECC,
// SIFT, registration, warp, YUV, JPEG). Everything here is a thin try/catch shim that turns gtx::Error into a status code +
// thread-local message. The operator hooks (gtx_op_*) are in gtx_ops.cpp; feeder.cpp, reid.cpp and table_writer.cpp define their own.
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/gtx.h"
#include "api_guard.hpp"
#include "common.hpp"
#include "detector.hpp"
#include "draw.hpp"
#include "rtdetr.hpp"
#include "geometry.hpp"
#include "ecc.hpp"
#include "gmc.hpp"
#include "gmc_feat.hpp"
#include "jpeg.hpp"
#include "jpeg_enc.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_restart.hpp"
#include "register.hpp"
#include "sift.hpp"
#include "sift_stab.hpp"
#include "stabilizer.hpp"
#include "tracker.hpp"

namespace {
using gtx::g_last_error;
using gtx::guarded;
using gtx::need;
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
int gtx_dev_copy(gtx_ctx* ctx, void* dst_dptr, const void* src_dptr, size_t bytes) {
  return guarded([&] {
    need(ctx, "ctx"); need(dst_dptr, "dst"); need(src_dptr, "src");
    GTX_HIP(hipSetDevice(ctx->device));
    if (bytes) GTX_HIP(hipMemcpyAsync(dst_dptr, src_dptr, bytes, hipMemcpyDeviceToDevice, ctx->stream));
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

int gtx_sift_stab_create(gtx_ctx* ctx, const gtx_sift_stab_config* cfg, gtx_sift_stab** out) {
  return guarded([&] {
    need(ctx, "ctx"); need(cfg, "cfg"); need(out, "out");
    std::unique_ptr<gtx_sift_stab> s(new gtx_sift_stab);
    s->impl.reset(new gtx::SiftStab(ctx, *cfg));
    *out = s.release();
  });
}
void gtx_sift_stab_destroy(gtx_sift_stab* st) { delete st; }
int gtx_sift_stab_set_ref_gray_dev(gtx_sift_stab* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n) {
  return guarded([&] { need(st, "st"); need(gray_dptr, "gray"); st->impl->set_ref_gray_dev(gray_dptr, gh, gw, boxes_xywh, n); });
}
int gtx_sift_stab_submit_gray_dev(gtx_sift_stab* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n) {
  return guarded([&] { need(st, "st"); need(gray_dptr, "gray"); st->impl->submit_gray_dev(gray_dptr, gh, gw, boxes_xywh, n); });
}
int gtx_sift_stab_collect(gtx_sift_stab* st, double H[9], int* valid, int stats[4]) {
  return guarded([&] { need(st, "st"); need(H, "H"); need(valid, "valid"); st->impl->collect(H, valid, stats); });
}
int gtx_sift_stab_stabilize_gray_dev(gtx_sift_stab* st, const void* gray_dptr, int gh, int gw, const float* boxes_xywh, int n, double H[9],
                                     int* valid, int stats[4]) {
  return guarded([&] {
    need(st, "st"); need(gray_dptr, "gray"); need(H, "H"); need(valid, "valid");
    st->impl->submit_gray_dev(gray_dptr, gh, gw, boxes_xywh, n);
    st->impl->collect(H, valid, stats);
  });
}
int gtx_sift_stab_last_ms(gtx_sift_stab* st, float* ms) {
  return guarded([&] { need(st, "st"); need(ms, "ms"); *ms = st->impl->last_ms(); });
}
int gtx_sift_stab_keypoints(gtx_sift_stab* st, int which, int cap, int* n, float* kp5, int* octave, float* desc) {
  return guarded([&] { need(st, "st"); need(n, "n"); st->impl->keypoints(which, cap, n, kp5, octave, desc); });
}
int gtx_sift_stab_pairs(gtx_sift_stab* st, int cap, int* n, float* pts) {
  return guarded([&] { need(st, "st"); need(n, "n"); st->impl->pairs(cap, n, pts); });
}
int gtx_sift_stab_counters(gtx_sift_stab* st, int out[4]) {
  return guarded([&] { need(st, "st"); need(out, "out"); st->impl->counters(out); });
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

size_t gtx_jpeg_plan_bound(int h, int w) {
  return (h <= 0 || w <= 0 || h > gtx::jpeg::kMaxDim || w > gtx::jpeg::kMaxDim) ? 0 : gtx::jpeg::plan_bound(h, w);
}

int gtx_jpeg_plan(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs, void* out, size_t capacity, size_t* needed) {
  int rc = 0;
  const int st = guarded([&] {
    need(bytes, "bytes"); need(needed, "needed");
    if (!out && capacity) gtx::fail(GTX_ERR_INVALID, "jpeg_plan: out is NULL with a capacity of %zu", capacity);
    gtx::jpeg::Info info;
    char msg[512];
    rc = gtx::jpeg::plan(static_cast<const uint8_t*>(bytes), n, (long long)frame, &info, out, capacity, needed, msg, sizeof msg);
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

int gtx_jpeg_entropy_ms(gtx_ctx* ctx, const void* plan, size_t bytes, int sub_bits, int rounds, int reps, float ms[2], int* status, int* rounds_used) {
  return guarded([&] {
    need(plan, "plan"); need(ms, "ms"); need(status, "status"); need(rounds_used, "rounds_used");
    char msg[256];
    if (gtx::jpeg::check_plan(plan, bytes, msg, sizeof msg) != 0) gtx::fail(GTX_ERR_INVALID, "%s", msg);
    if (sub_bits != 0 && !gtx::jpeg_entropy_sub_bits_ok(sub_bits)) gtx::fail(GTX_ERR_INVALID, "jpeg_entropy_ms: sub_bits %d", sub_bits);
    if (rounds < 0 || rounds > gtx::kJpegEntropyMaxRounds) gtx::fail(GTX_ERR_INVALID, "jpeg_entropy_ms: %d rounds", rounds);
    if (reps < 1 || reps > 10000) gtx::fail(GTX_ERR_INVALID, "jpeg_entropy_ms: %d repetitions", reps);
    gtx::jpeg::PlanHeader ph;
    memcpy(&ph, plan, sizeof ph);
    if (ph.stream_bytes > (1u << 28)) gtx::fail(GTX_ERR_INVALID, "jpeg_entropy_ms: more than 256 MB of entropy-coded data");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t nb = ph.n_blocks;
    const gtx::jpeg::RecordHeader hd = gtx::JpegEntropy::record_header(ph);
    gtx::DevBuf d_plan(bytes), d_rec(gtx::jpeg::record_bytes(nb, 64 * nb)), d_planes(gtx::jpeg::planes_bytes(hd)), d_bgr((size_t)ph.height * ph.width * 3);
    GTX_HIP(hipMemcpyAsync(d_plan.p, plan, bytes, hipMemcpyHostToDevice, ctx->stream));
    gtx::JpegEntropy dec(ctx, nb, ph.stream_bytes, sub_bits ? sub_bits : gtx::kJpegEntropySubBits);
    hipEvent_t e[3];
    for (auto& x : e) GTX_HIP(hipEventCreate(&x));
    double sum[2] = {0, 0};
    try {
      for (int r = -1; r < reps; ++r) {                          // one untimed pass first
        GTX_HIP(hipEventRecord(e[0], ctx->stream));
        dec.enqueue(d_plan.as<const uint8_t>(), ph, sub_bits, rounds, d_rec.as<uint8_t>());
        GTX_HIP(hipEventRecord(e[1], ctx->stream));
        gtx::jpeg_decode_launch(ctx, d_rec.p, hd, d_planes.p, d_bgr.p);
        GTX_HIP(hipEventRecord(e[2], ctx->stream));
        GTX_HIP(hipEventSynchronize(e[2]));
        if (r < 0) continue;
        for (int k = 0; k < 2; ++k) {
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
    for (int k = 0; k < 2; ++k) ms[k] = (float)(sum[k] / reps);
    uint32_t res[2];
    GTX_HIP(hipMemcpy(res, dec.d_result(), sizeof res, hipMemcpyDeviceToHost));
    *status = (int)res[0], *rounds_used = (int)res[1];
  });
}

size_t gtx_jpeg_plan_intervals_bound(int h, int w) {
  return (h <= 0 || w <= 0 || h > gtx::jpeg::kMaxDim || w > gtx::jpeg::kMaxDim) ? 0 : gtx::jpeg::plan_intervals_bound(h, w);
}

int gtx_jpeg_plan_intervals(const void* bytes, size_t n, int64_t frame, int* h, int* w, int* ncomp, int* hs, int* vs, void* out, size_t capacity,
                            size_t* needed) {
  int rc = 0;
  const int st = guarded([&] {
    need(bytes, "bytes"); need(needed, "needed");
    if (!out && capacity) gtx::fail(GTX_ERR_INVALID, "jpeg_plan_intervals: out is NULL with a capacity of %zu", capacity);
    gtx::jpeg::Info info;
    char msg[512];
    rc = gtx::jpeg::plan_intervals(static_cast<const uint8_t*>(bytes), n, (long long)frame, &info, out, capacity, needed, msg, sizeof msg);
    if (h) *h = info.height;
    if (w) *w = info.width;
    if (ncomp) *ncomp = info.ncomp;
    if (hs) *hs = info.hs;
    if (vs) *vs = info.vs;
    if (rc < 0) gtx::fail(rc, "%s", msg);
  });
  return st != GTX_OK ? st : rc;
}

int gtx_jpeg_restart_ms(gtx_ctx* ctx, const void* plan, size_t bytes, int copies, int reps, float ms[2], int* status) {
  return guarded([&] {
    need(plan, "plan"); need(ms, "ms"); need(status, "status");
    char msg[256];
    if (gtx::jpeg::check_plan_intervals(plan, bytes, msg, sizeof msg) != 0) gtx::fail(GTX_ERR_INVALID, "%s", msg);
    if (copies < 1 || copies > 64) gtx::fail(GTX_ERR_INVALID, "jpeg_restart_ms: %d copies", copies);
    if (reps < 1 || reps > 10000) gtx::fail(GTX_ERR_INVALID, "jpeg_restart_ms: %d repetitions", reps);
    gtx::jpeg::PlanHeader ph;
    memcpy(&ph, plan, sizeof ph);
    if (ph.stream_bytes > (1u << 28)) gtx::fail(GTX_ERR_INVALID, "jpeg_restart_ms: more than 256 MB of entropy-coded data");
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    const size_t nb = ph.n_blocks, rec_bytes = (gtx::jpeg::record_bytes(nb, 64 * nb) + 255) / 256 * 256, plan_bytes = (bytes + 255) / 256 * 256;
    const gtx::jpeg::RecordHeader hd = gtx::JpegEntropy::record_header(ph);
    gtx::DevBuf d_plan((size_t)copies * plan_bytes), d_rec((size_t)copies * rec_bytes), d_planes(gtx::jpeg::planes_bytes(hd)), d_bgr((size_t)ph.height * ph.width * 3);
    std::vector<const uint8_t*> plans((size_t)copies);
    std::vector<uint8_t*> recs((size_t)copies);
    std::vector<gtx::jpeg::PlanHeader> phs((size_t)copies, ph);
    for (int k = 0; k < copies; ++k) {
      plans[(size_t)k] = d_plan.as<const uint8_t>() + (size_t)k * plan_bytes, recs[(size_t)k] = d_rec.as<uint8_t>() + (size_t)k * rec_bytes;
      GTX_HIP(hipMemcpyAsync(d_plan.as<uint8_t>() + (size_t)k * plan_bytes, plan, bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    gtx::JpegRestart dec(ctx, copies, nb);
    hipEvent_t e[3];
    for (auto& x : e) GTX_HIP(hipEventCreate(&x));
    double sum[2] = {0, 0};
    try {
      for (int r = -1; r < reps; ++r) {                          // one untimed pass first
        GTX_HIP(hipEventRecord(e[0], ctx->stream));
        dec.enqueue(copies, plans.data(), phs.data(), recs.data());
        GTX_HIP(hipEventRecord(e[1], ctx->stream));
        for (int k = 0; k < copies; ++k) gtx::jpeg_decode_launch(ctx, recs[(size_t)k], hd, d_planes.p, d_bgr.p);
        GTX_HIP(hipEventRecord(e[2], ctx->stream));
        GTX_HIP(hipEventSynchronize(e[2]));
        if (r < 0) continue;
        for (int k = 0; k < 2; ++k) {
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
    for (int k = 0; k < 2; ++k) ms[k] = (float)(sum[k] / reps / copies);
    uint32_t res = 0;
    GTX_HIP(hipMemcpy(&res, dec.d_result(0), sizeof res, hipMemcpyDeviceToHost));
    *status = (int)res;
  });
}

int gtx_jpeg_emit_restart(const void* record, size_t bytes, int restart_mcus, void* out, size_t capacity, size_t* n) {
  int rc = 0;
  const int st = guarded([&] {
    need(record, "record"); need(n, "n");
    if (!out && capacity) gtx::fail(GTX_ERR_INVALID, "jpeg_emit_restart: out is NULL with a capacity of %zu", capacity);
    if (reinterpret_cast<uintptr_t>(record) & 3) gtx::fail(GTX_ERR_INVALID, "jpeg_emit_restart: the record is not 4-byte aligned");
    if (restart_mcus < 0 || restart_mcus > 65535) gtx::fail(GTX_ERR_INVALID, "jpeg_emit_restart: a restart interval of %d MCUs (0..65535)", restart_mcus);
    char msg[256];
    rc = gtx::jpeg::emit_restart(record, bytes, (unsigned)restart_mcus, static_cast<uint8_t*>(out), capacity, n, msg, sizeof msg);
    if (rc < 0) gtx::fail(rc, "%s", msg);
  });
  return st != GTX_OK ? st : rc;
}

int gtx_jpeg_enc_create(gtx_ctx* ctx, int h, int w, int quality, int subsampling, gtx_jpeg_enc** out) {
  return guarded([&] {
    need(out, "out");
    *out = nullptr;
    gtx::JpegEncoder::check_args(h, w, quality, subsampling);
    need(ctx, "ctx");
    std::unique_ptr<gtx_jpeg_enc> e(new gtx_jpeg_enc);
    e->impl.reset(new gtx::JpegEncoder(ctx, h, w, quality, subsampling));
    *out = e.release();
  });
}

void gtx_jpeg_enc_destroy(gtx_jpeg_enc* enc) { delete enc; }

int gtx_jpeg_enc_submit_dev(gtx_jpeg_enc* enc, const void* bgr_dptr) {
  return guarded([&] {
    need(enc, "enc"); need(bgr_dptr, "bgr");
    enc->impl->submit(bgr_dptr);
  });
}

int gtx_jpeg_enc_collect(gtx_jpeg_enc* enc, void* record, size_t capacity, size_t* bytes) {
  bool fits = true;
  const int st = guarded([&] {
    need(enc, "enc"); need(bytes, "bytes");
    fits = enc->impl->collect(record, capacity, bytes);
  });
  return st != GTX_OK ? st : fits ? 0 : 1;
}

int gtx_jpeg_enc_last_ms(gtx_jpeg_enc* enc, float* ms) {
  return guarded([&] {
    need(enc, "enc"); need(ms, "ms");
    *ms = enc->impl->last_ms();
  });
}

int gtx_jpeg_enc_set_entropy(gtx_jpeg_enc* enc, int gpu) {
  return guarded([&] {
    need(enc, "enc");
    if (gpu) {
      enc->impl->use_gpu_entropy();
    } else if (enc->impl->gpu_entropy()) {
      gtx::fail(GTX_ERR_INVALID, "jpeg_enc_set_entropy: the encoder is on the GPU entropy route already");
    }
  });
}

int gtx_jpeg_enc_collect_jpeg(gtx_jpeg_enc* enc, void* out, size_t capacity, size_t* n) {
  bool fits = true;
  const int st = guarded([&] {
    need(enc, "enc"); need(n, "n");
    fits = enc->impl->collect_jpeg(out, capacity, n);
  });
  return st != GTX_OK ? st : fits ? 0 : 1;
}

int gtx_jpeg_enc_entropy_ms(gtx_jpeg_enc* enc, float* ms) {
  return guarded([&] {
    need(enc, "enc"); need(ms, "ms");
    *ms = enc->impl->entropy_ms();
  });
}

size_t gtx_jpeg_picture_bound(int h, int w) {
  return (h <= 0 || w <= 0 || h > gtx::jpeg::kMaxDim || w > gtx::jpeg::kMaxDim) ? 0 : gtx::jpeg_picture_bound(gtx::jpeg::max_blocks(h, w));
}

int gtx_jpeg_header(const void* record, size_t bytes, void* out, size_t capacity, size_t* n) {
  int rc = 0;
  const int st = guarded([&] {
    need(record, "record"); need(n, "n");
    *n = 0;
    if (!out && capacity) gtx::fail(GTX_ERR_INVALID, "jpeg_header: out is NULL with a capacity of %zu", capacity);
    if (reinterpret_cast<uintptr_t>(record) & 3) gtx::fail(GTX_ERR_INVALID, "jpeg_header: the record is not 4-byte aligned");
    if (bytes < gtx::jpeg::kOffsetsOffset) gtx::fail(GTX_ERR_INVALID, "JPEG record: too short for its header and quantisers");
    gtx::jpeg::RecordHeader hd, want;
    memcpy(&hd, record, sizeof hd);
    if (hd.magic != gtx::jpeg::kMagic || !gtx::jpeg::make_header((int)hd.height, (int)hd.width, (int)hd.ncomp, (int)hd.hs, (int)hd.vs, &want))
      gtx::fail(GTX_ERR_INVALID, "JPEG record: not a record, or a size or sampling outside the accepted set");
    const uint16_t* quant = reinterpret_cast<const uint16_t*>(static_cast<const uint8_t*>(record) + gtx::jpeg::kQuantOffset);
    for (uint32_t i = 0; i < 64 * hd.ncomp; ++i)
      if (quant[i] > 255) gtx::fail(GTX_ERR_INVALID, "JPEG record: a quantiser above 255 (baseline tables have 8-bit entries)");
    uint8_t tmp[gtx::jpeg::kMaxHeaderBytes];
    *n = gtx::jpeg::header(hd, quant, tmp, sizeof tmp);
    if (*n > sizeof tmp) gtx::fail(GTX_ERR_INTERNAL, "jpeg_header: a header of %zu bytes", *n);
    if (capacity < *n) {
      rc = 1;
      return;
    }
    memcpy(out, tmp, *n);
  });
  return st != GTX_OK ? st : rc;
}

int gtx_jpeg_emit(const void* record, size_t bytes, void* out, size_t capacity, size_t* n) {
  int rc = 0;
  const int st = guarded([&] {
    need(record, "record"); need(n, "n");
    if (!out && capacity) gtx::fail(GTX_ERR_INVALID, "jpeg_emit: out is NULL with a capacity of %zu", capacity);
    if (reinterpret_cast<uintptr_t>(record) & 3) gtx::fail(GTX_ERR_INVALID, "jpeg_emit: the record is not 4-byte aligned");
    char msg[256];
    rc = gtx::jpeg::emit(record, bytes, static_cast<uint8_t*>(out), capacity, n, msg, sizeof msg);
    if (rc < 0) gtx::fail(rc, "%s", msg);
  });
  return st != GTX_OK ? st : rc;
}

int gtx_drawer_create(gtx_ctx* ctx, int h, int w, int max_prims, const void* atlas, size_t atlas_bytes, gtx_drawer** out) {
  return guarded([&] {
    need(out, "out");
    *out = nullptr;
    gtx::Drawer::check_args(h, w, max_prims, atlas, atlas_bytes);
    need(ctx, "ctx");
    std::unique_ptr<gtx_drawer> d(new gtx_drawer);
    d->impl.reset(new gtx::Drawer(ctx, h, w, max_prims, atlas, atlas_bytes));
    *out = d.release();
  });
}

void gtx_drawer_destroy(gtx_drawer* drawer) { delete drawer; }

int gtx_drawer_draw_dev(gtx_drawer* drawer, void* frame_dptr, const int32_t* prims, int n) {
  return guarded([&] {
    need(drawer, "drawer");
    drawer->impl->draw(frame_dptr, prims, n);
  });
}

int gtx_drawer_last_ms(gtx_drawer* drawer, float* ms) {
  return guarded([&] {
    need(drawer, "drawer"); need(ms, "ms");
    *ms = drawer->impl->last_ms();
  });
}

int gtx_warp_frame_dev(gtx_ctx* ctx, const void* src_dptr, int h, int w, const double H[9], void* dst_dptr) {
  return guarded([&] {
    need(ctx, "ctx"); need(src_dptr, "src"); need(H, "H"); need(dst_dptr, "dst");
    if (src_dptr == dst_dptr) gtx::fail(GTX_ERR_INVALID, "warp_frame: source and destination must be distinct buffers");
    gtx::warp_frame_dev(ctx, src_dptr, h, w, H, dst_dptr);
  });
}


int gtx_warp_frame(gtx_ctx* ctx, const uint8_t* src_bgr, int h, int w, const double H[9], uint8_t* dst_bgr) {
  return guarded([&] {
    need(ctx, "ctx"); need(src_bgr, "src"); need(H, "H"); need(dst_bgr, "dst");
    gtx::warp_frame(ctx, src_bgr, h, w, H, dst_bgr);
  });
}

}  // extern "C"
