// Host half of the plot stage's trajectory maps: validation of sizes and of a primitive list (nothing is uploaded, and nothing is
// dropped, when a record is bad: the call fails with the record's index), the quantisation and the conservative boxes of
// geotrax_amd/plot_draw.py, the launch sequence of csrc/plot_draw.hip with its exactly sized tile lists, the canvas object and
// the C entry points gtx_plot_canvas_* / gtx_op_plot_*. plot_check_* and plot_quantise touch no GPU and
// compile alone with -DGTX_PLOT_HOST_ONLY, for a stand-alone host check.
#include "plot_draw.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/gtx.h"
#include "jpeg_parse.hpp"

namespace gtx {

namespace {
constexpr double kCoordMin = -32768.0, kCoordMax = 32767.0, kMaxSpan = 2048.0, kMinWidth = 0.25, kMaxWidth = 64.0;
inline bool coord_ok(float v) { return std::isfinite(v) && v >= kCoordMin && v <= kCoordMax; }
inline int16_t clamp16(long long v) { return (int16_t)std::min(std::max(v, -32768LL), 32767LL); }
inline long long floor_div16(long long v) { return v >= 0 ? v / 16 : -((-v + 15) / 16); }
}  // namespace

void plot_check_canvas(int h, int w) {
  if (h < 1 || w < 1 || h > jpeg::kMaxDim || w > jpeg::kMaxDim)
    fail(GTX_ERR_INVALID, "plot: a %d x %d canvas is outside 1..%d (what the JPEG encoder accepts)", w, h, jpeg::kMaxDim);
}

void plot_check_pitch(int h, int w, size_t pitch, size_t buf_bytes) {
  plot_check_canvas(h, w);
  if (pitch < (size_t)w * 3 || pitch > ((size_t)1 << 20)) fail(GTX_ERR_INVALID, "plot: a pitch of %zu bytes for rows of %d pixels", pitch, w);
  if (buf_bytes < (size_t)(h - 1) * pitch + (size_t)w * 3) fail(GTX_ERR_INVALID, "plot: %zu bytes do not hold %d rows at a pitch of %zu", buf_bytes, h, pitch);
}

void plot_check_reduce(int h, int w, int channels, int k) {
  if (h < 1 || w < 1 || h > (1 << 20) || w > (1 << 20)) fail(GTX_ERR_INVALID, "plot: a %d x %d image", w, h);
  if (channels != 1 && channels != 3 && channels != 4) fail(GTX_ERR_INVALID, "plot: %d channels (1 = gray, 3 = RGB, 4 = RGBA)", channels);
  if (k < 1 || k > kPlotMaxFactor) fail(GTX_ERR_INVALID, "plot: factor %d is outside 1..%d", k, kPlotMaxFactor);
  plot_check_canvas((h + k - 1) / k, (w + k - 1) / k);
}

void plot_check_prims(const void* prims, int n) {
  if (n < 0) fail(GTX_ERR_INVALID, "plot: n = %d", n);
  if (n > kPlotMaxPrims) fail(GTX_ERR_INVALID, "plot: %d primitives, a call takes %d", n, kPlotMaxPrims);
  if (n > 0 && !prims) fail(GTX_ERR_INVALID, "plot: prims is NULL with n = %d", n);
  PlotPrimHost prev{};
  for (int i = 0; i < n; ++i) {
    PlotPrimHost p;
    std::memcpy(&p, static_cast<const uint8_t*>(prims) + sizeof p * (size_t)i, sizeof p);
    if (!coord_ok(p.x0) || !coord_ok(p.y0) || !coord_ok(p.x1) || !coord_ok(p.y1))
      fail(GTX_ERR_INVALID, "plot: primitive %d: a coordinate is not finite or outside [-32768, 32767]", i);
    if (std::fabs((double)p.x1 - p.x0) > kMaxSpan || std::fabs((double)p.y1 - p.y0) > kMaxSpan)
      fail(GTX_ERR_INVALID, "plot: primitive %d: the segment spans more than %.0f pixels", i, kMaxSpan);
    if (!(p.width >= kMinWidth && p.width <= kMaxWidth)) fail(GTX_ERR_INVALID, "plot: primitive %d: width %g is outside %g..%g", i, (double)p.width, kMinWidth, kMaxWidth);
    if (p.alpha < 1 || p.alpha > 256) fail(GTX_ERR_INVALID, "plot: primitive %d: alpha %d is outside 1..256", i, p.alpha);
    if (p.bgr < 0 || p.bgr > 0xFFFFFF) fail(GTX_ERR_INVALID, "plot: primitive %d: colour 0x%x", i, (unsigned)p.bgr);
    if (i > 0 && p.poly == prev.poly && (p.width != prev.width || p.bgr != prev.bgr || p.alpha != prev.alpha))
      fail(GTX_ERR_INVALID, "plot: primitive %d: width, colour or alpha differ from the polyline's first record", i);
    prev = p;
  }
}

void plot_quantise(const void* prims, int n, PlotPrim* q, PlotBox* boxes) {
  int run = -1;
  int32_t prev_poly = 0;
  for (int i = 0; i < n; ++i) {
    PlotPrimHost p;
    std::memcpy(&p, static_cast<const uint8_t*>(prims) + sizeof p * (size_t)i, sizeof p);
    if (i == 0 || p.poly != prev_poly) ++run;
    prev_poly = p.poly;
    auto fx = [](float v) { return (int32_t)std::floor((double)v * 16.0 + 0.5); };
    PlotPrim d;
    d.x0 = fx(p.x0), d.y0 = fx(p.y0), d.x1 = fx(p.x1), d.y1 = fx(p.y1);
    d.R = (int32_t)std::floor((double)p.width * 256.0 + 0.5) + 256;
    d.bgr = p.bgr, d.alpha = p.alpha, d.run = run;
    q[i] = d;
    const long long pad = (d.R + 31) / 32;
    boxes[i] = PlotBox{clamp16(floor_div16(std::min(d.x0, d.x1) - pad)), clamp16(floor_div16(std::min(d.y0, d.y1) - pad)),
                       clamp16(floor_div16(std::max(d.x0, d.x1) + pad)), clamp16(floor_div16(std::max(d.y0, d.y1) + pad))};
  }
}

}  // namespace gtx

// ------------------------------------------------------------------------------------------------------------- the GPU side
#ifndef GTX_PLOT_HOST_ONLY

#include "api_guard.hpp"
#include "net_runtime.hpp"
#include "op_staging.hpp"

namespace gtx {

namespace {
struct Events {
  hipEvent_t e[5] = {};
  explicit Events(bool on) {
    if (on)
      for (auto& x : e) GTX_HIP(hipEventCreate(&x));
  }
  ~Events() {
    for (auto& x : e)
      if (x) (void)hipEventDestroy(x);
  }
  void mark(int k, hipStream_t s) {
    if (e[k]) GTX_HIP(hipEventRecord(e[k], s));
  }
  double ms(int a, int b) {
    float v = 0.f;
    if (e[a] && e[b]) GTX_HIP(hipEventElapsedTime(&v, e[a], e[b]));
    return v;
  }
};
}  // namespace

PlotListStats plot_draw(gtx_ctx* ctx, uint8_t* d_canvas, int h, int w, size_t pitch, const void* prims, int n, bool timed) {
  PlotListStats st;
  st.prims = n;
  const int tiles_x = cdiv(w, kPlotTileW), tiles_y = cdiv(h, kPlotTileH), n_tiles = tiles_x * tiles_y;
  st.tiles = n_tiles;
  if (n == 0) return st;
  std::vector<PlotPrim> q((size_t)n);
  std::vector<PlotBox> boxes((size_t)n);
  plot_quantise(prims, n, q.data(), boxes.data());
  GTX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  DevBuf d_prims, d_boxes, d_counts, d_cursor, d_offsets((size_t)(n_tiles + 1) * 4), d_small, d_list, d_sorted;
  upload(d_prims, q.data(), q.size() * sizeof(PlotPrim));
  upload(d_boxes, boxes.data(), boxes.size() * sizeof(PlotBox));
  zeros(d_counts, (size_t)n_tiles * 4);
  zeros(d_cursor, (size_t)n_tiles * 4);
  zeros(d_small, 16);                                               // the 64-bit total, then the longest list
  Events ev(timed);
  ev.mark(0, s);
  plot_count_launch(s, d_boxes.as<PlotBox>(), n, h, w, d_counts.as<uint32_t>(), d_small.as<unsigned long long>());
  plot_scan_launch(s, d_counts.as<uint32_t>(), n_tiles, d_offsets.as<uint32_t>(), d_small.as<uint32_t>() + 2);
  ev.mark(1, s);
  struct { unsigned long long total; uint32_t longest, pad; } small{};
  GTX_HIP(hipMemcpyAsync(&small, d_small.p, sizeof small, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipStreamSynchronize(s));
  if (small.total > 0x7FFFFFFFull) fail(GTX_ERR_INVALID, "plot: the tile lists would hold %llu entries; draw the list in parts", small.total);
  st.entries = (double)small.total, st.max_per_tile = small.longest;
  if (small.total == 0) return st;                                  // every primitive lies off the canvas
  const uint32_t entries = (uint32_t)small.total;
  d_list.alloc((size_t)entries * 4);
  d_sorted.alloc((size_t)entries * 4);
  ev.mark(2, s);
  plot_fill_launch(s, d_boxes.as<PlotBox>(), n, h, w, d_offsets.as<uint32_t>(), d_cursor.as<uint32_t>(), d_list.as<uint32_t>(), entries);
  plot_sort_launch(s, d_offsets.as<uint32_t>(), n_tiles, d_list.as<uint32_t>(), d_sorted.as<uint32_t>(), entries);
  ev.mark(3, s);
  plot_paint_launch(s, d_canvas, h, w, pitch, d_prims.as<PlotPrim>(), d_boxes.as<PlotBox>(), n, d_offsets.as<uint32_t>(), d_sorted.as<uint32_t>(), entries);
  ev.mark(4, s);
  GTX_HIP(hipStreamSynchronize(s));                                 // the lists are freed on the way out
  st.bin_ms = ev.ms(0, 1) + ev.ms(2, 3), st.paint_ms = ev.ms(3, 4);
  return st;
}

PlotCanvas::PlotCanvas(gtx_ctx* ctx, const uint8_t* image, int h, int w, int channels, int k) : ctx_(ctx), h_((h + k - 1) / k), w_((w + k - 1) / k) {
  GTX_HIP(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  Events ev(true);
  DevBuf d_src((size_t)h * w * channels);
  d_canvas_.alloc((size_t)h_ * w_ * 3);
  ev.mark(0, s);
  GTX_HIP(hipMemcpyAsync(d_src.p, image, (size_t)h * w * channels, hipMemcpyHostToDevice, s));
  ev.mark(1, s);
  plot_reduce_launch(s, d_src.as<uint8_t>(), h, w, channels, k, d_canvas_.as<uint8_t>());
  ev.mark(2, s);
  GTX_HIP(hipStreamSynchronize(s));                                 // the source image is freed on the way out
  upload_ms_ = ev.ms(0, 1), reduce_ms_ = ev.ms(1, 2);
}

void PlotCanvas::draw(const void* prims, int n) {
  plot_check_prims(prims, n);
  last_ = plot_draw(ctx_, d_canvas_.as<uint8_t>(), h_, w_, (size_t)w_ * 3, prims, n, true);
}

void PlotCanvas::read(uint8_t* bgr) {
  GTX_HIP(hipSetDevice(ctx_->device));
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  download(bgr, d_canvas_, (size_t)h_ * w_ * 3);
}

void PlotCanvas::stats(double out[8]) const {
  const double v[8] = {upload_ms_, reduce_ms_, last_.bin_ms, last_.paint_ms, last_.tiles, last_.entries, last_.max_per_tile, last_.prims};
  std::memcpy(out, v, sizeof v);
}

}  // namespace gtx

extern "C" {

using gtx::guarded;
using gtx::need;

int gtx_plot_canvas_create(gtx_ctx* ctx, const uint8_t* image, int h, int w, int channels, int k, gtx_plot_canvas** out) {
  return guarded([&] {
    need(out, "out");
    *out = nullptr;
    gtx::plot_check_reduce(h, w, channels, k);
    need(image, "image"); need(ctx, "ctx");
    std::unique_ptr<gtx_plot_canvas> c(new gtx_plot_canvas);
    c->impl.reset(new gtx::PlotCanvas(ctx, image, h, w, channels, k));
    *out = c.release();
  });
}

void gtx_plot_canvas_destroy(gtx_plot_canvas* canvas) { delete canvas; }

int gtx_plot_canvas_size(gtx_plot_canvas* canvas, int* h, int* w) {
  return guarded([&] {
    need(canvas, "canvas"); need(h, "h"); need(w, "w");
    *h = canvas->impl->h(), *w = canvas->impl->w();
  });
}

int gtx_plot_canvas_draw(gtx_plot_canvas* canvas, const void* prims, int n) {
  return guarded([&] {
    need(canvas, "canvas");
    canvas->impl->draw(prims, n);
  });
}

int gtx_plot_canvas_read(gtx_plot_canvas* canvas, uint8_t* bgr) {
  return guarded([&] {
    need(canvas, "canvas"); need(bgr, "bgr");
    canvas->impl->read(bgr);
  });
}

int gtx_plot_canvas_dptr(gtx_plot_canvas* canvas, void** dptr) {
  return guarded([&] {
    need(canvas, "canvas"); need(dptr, "dptr");
    *dptr = canvas->impl->dptr();
  });
}

int gtx_plot_canvas_stats(gtx_plot_canvas* canvas, double out[8]) {
  return guarded([&] {
    need(canvas, "canvas"); need(out, "out");
    canvas->impl->stats(out);
  });
}

// ---- the binning and paint launches on a host canvas (tests/test_plot_draw_gpu.py)

int gtx_op_plot_draw(gtx_ctx* ctx, uint8_t* buf, size_t buf_bytes, int h, int w, size_t pitch, const void* prims, int n) {
  return guarded([&] {
    gtx::plot_check_pitch(h, w, pitch, buf_bytes);
    need(buf, "buf");
    gtx::plot_check_prims(prims, n);
    need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf d_buf;
    gtx::upload(d_buf, buf, buf_bytes);
    (void)gtx::plot_draw(ctx, d_buf.as<uint8_t>(), h, w, pitch, prims, n, false);
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    gtx::download(buf, d_buf, buf_bytes);
  });
}

// ---- the reduce launch on a host image (tests/test_plot_draw_gpu.py)

int gtx_op_plot_reduce(gtx_ctx* ctx, const uint8_t* image, int h, int w, int channels, int k, uint8_t* bgr_out) {
  return guarded([&] {
    gtx::plot_check_reduce(h, w, channels, k);
    need(image, "image"); need(bgr_out, "bgr_out"); need(ctx, "ctx");
    GTX_HIP(hipSetDevice(ctx->device));
    gtx::DevBuf d_src, d_dst((size_t)((h + k - 1) / k) * ((w + k - 1) / k) * 3);
    gtx::upload(d_src, image, (size_t)h * w * channels);
    gtx::plot_reduce_launch(ctx->stream, d_src.as<uint8_t>(), h, w, channels, k, d_dst.as<uint8_t>());
    GTX_HIP(hipStreamSynchronize(ctx->stream));
    gtx::download(bgr_out, d_dst, (size_t)((h + k - 1) / k) * ((w + k - 1) / k) * 3);
  });
}

}  // extern "C"
#endif  // GTX_PLOT_HOST_ONLY
