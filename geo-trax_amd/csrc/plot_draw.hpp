// The plot stage's trajectory maps (csrc/plot_draw.hip, csrc/plot_draw.cpp): an image reduced into a BGR canvas in HBM, and
// semi-transparent strokes and discs painted into it through per-tile lists. The pixel rule is written down once, in
// geotrax_amd/plot_draw.py (the numpy twin, all integer); this header names the records and the launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

#include "common.hpp"

struct gtx_ctx;

namespace gtx {

constexpr int kPlotTileW = 64, kPlotTileH = 16;   // pixels of a paint workgroup's tile (a lane owns 4 consecutive pixels of one row), as draw.hip's
constexpr int kPlotChunk = 256;                   // list entries a paint workgroup stages in LDS at a time = its size (no limit on a list's length)
constexpr int kPlotMaxPrims = 1 << 22;            // per draw call
constexpr int kPlotMaxFactor = 256;               // reduce: 255 k^2 stays far inside int32
constexpr int kPlotScanPerLane = 8;               // tiles one lane of the single-workgroup prefix sum owns per round

struct PlotPrimHost { float x0, y0, x1, y1, width; int32_t bgr, alpha, poly; };                 // 32 bytes: the ABI's record
struct alignas(16) PlotPrim { int32_t x0, y0, x1, y1, R, bgr, alpha, run; };                    // quantised (plot_draw.py `quantise`)
struct alignas(8) PlotBox { int16_t x0, y0, x1, y1; };                                          // inclusive pixels, conservative

// Host only, no GPU. Each throws GTX_ERR_INVALID; plot_check_prims names the first bad record's index.
void plot_check_canvas(int h, int w);                                    // 1..jpeg::kMaxDim per side: what the JPEG encoder accepts
void plot_check_pitch(int h, int w, size_t pitch, size_t buf_bytes);
void plot_check_reduce(int h, int w, int channels, int k);               // the reduced picture must pass plot_check_canvas
void plot_check_prims(const void* prims, int n);
void plot_quantise(const void* prims, int n, PlotPrim* q, PlotBox* boxes);

struct PlotListStats { double bin_ms = 0, paint_ms = 0, tiles = 0, entries = 0, max_per_tile = 0, prims = 0; };

// The launches, all on `stream`. Every index that becomes an address is checked in the kernels against h, w, pitch, n and the
// list sizes, whatever the host has validated.
void plot_reduce_launch(hipStream_t stream, const uint8_t* src, int h, int w, int channels, int k, uint8_t* dst_bgr);
void plot_count_launch(hipStream_t stream, const PlotBox* boxes, int n, int h, int w, uint32_t* counts, unsigned long long* total);
void plot_scan_launch(hipStream_t stream, const uint32_t* counts, int n_tiles, uint32_t* offsets /* n_tiles + 1 */, uint32_t* max_count);
void plot_fill_launch(hipStream_t stream, const PlotBox* boxes, int n, int h, int w, const uint32_t* offsets, uint32_t* cursor, uint32_t* list,
                      uint32_t entries);
void plot_sort_launch(hipStream_t stream, const uint32_t* offsets, int n_tiles, const uint32_t* list, uint32_t* sorted, uint32_t entries);
void plot_paint_launch(hipStream_t stream, uint8_t* canvas, int h, int w, size_t pitch, const PlotPrim* prims, const PlotBox* boxes, int n,
                       const uint32_t* offsets, const uint32_t* sorted, uint32_t entries);

// Validates, quantises, uploads and runs count -> scan -> (the total comes back: the lists are sized exactly) -> fill -> sort ->
// paint on the context's stream; waits for the total only. n == 0: nothing is launched.
PlotListStats plot_draw(gtx_ctx* ctx, uint8_t* d_canvas, int h, int w, size_t pitch, const void* prims, int n, bool timed);

class PlotCanvas {
 public:
  PlotCanvas(gtx_ctx* ctx, const uint8_t* image, int h, int w, int channels, int k);
  int h() const { return h_; }
  int w() const { return w_; }
  void* dptr() const { return d_canvas_.p; }
  void draw(const void* prims, int n);
  void read(uint8_t* bgr);
  void stats(double out[8]) const;

 private:
  gtx_ctx* ctx_;
  int h_, w_;
  DevBuf d_canvas_;
  double upload_ms_ = 0, reduce_ms_ = 0;
  PlotListStats last_;
};

}  // namespace gtx

struct gtx_plot_canvas {
  std::unique_ptr<gtx::PlotCanvas> impl;
};
