// The drawing for the visualize stage (csrc/draw.hip, csrc/draw.cpp): boxes, label fills, glyphs and tail rings painted into a BGR
// frame that stays in HBM. The pixel rule is written down once, in geotrax_amd/draw.py (the numpy twin); this header only
// names the record's fields.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>

#include "common.hpp"

struct gtx_ctx;

namespace gtx {

constexpr int kDrawFill = 0, kDrawSegment = 1, kDrawRing = 2, kDrawGlyph = 3;
constexpr int kDrawChunk = 256;                 // primitives one workgroup tests at a time = its size
constexpr int kDrawTileW = 64, kDrawTileH = 16; // pixels of a workgroup's tile (a lane owns 4 consecutive pixels of one row)
constexpr int kDrawMaxPrims = 1 << 20;          // per drawer
constexpr int kDrawMaxSide = 16384;             // frame sides, as the JPEG sink's
constexpr int kDrawStagingRing = 4;             // pinned staging buffers: calls that may be queued before one has to wait

struct alignas(16) DrawPrim { int32_t kind, x0, y0, x1, y1, p0, p1, bgr; };   // 32 bytes: the ABI's record
struct alignas(8) DrawBox { int16_t x0, y0, x1, y1; };                       // inclusive, conservative (draw.py bounding_boxes)

// Host only, no GPU. Each throws GTX_ERR_INVALID; check_prims names the first bad record's index.
void draw_check_frame(int h, int w);
void draw_check_prims(const int32_t* prims, int n, int max_prims, size_t atlas_bytes);
DrawBox draw_box(const DrawPrim& p);

// Enqueues the kernel on the stream (n > 0). d_prims: n records, d_boxes: their boxes, d_atlas: atlas_bytes bytes (may be null
// when atlas_bytes == 0). The kernel checks every index it turns into an address against h, w, n and atlas_bytes itself.
void draw_launch(hipStream_t stream, void* frame, int h, int w, const DrawPrim* d_prims, const DrawBox* d_boxes, int n,
                 const uint8_t* d_atlas, size_t atlas_bytes);

class Drawer {
 public:
  Drawer(gtx_ctx* ctx, int h, int w, int max_prims, const void* atlas, size_t atlas_bytes);
  ~Drawer();
  static void check_args(int h, int w, int max_prims, const void* atlas, size_t atlas_bytes);   // host only
  void draw(void* frame_dptr, const int32_t* prims, int n);       // validates, stages, enqueues; no wait. n == 0: nothing is launched
  float last_ms();                                                // the last draw()'s launch between two events (waits); 0 if it launched nothing

 private:
  void release();
  gtx_ctx* ctx_;
  int h_, w_, max_prims_;
  size_t atlas_bytes_;
  DevBuf d_atlas_, d_stage_;                                      // d_stage_: a call's n records, then its n boxes
  uint8_t* h_stage_[kDrawStagingRing] = {};                       // pinned, same layout
  hipEvent_t copied_[kDrawStagingRing] = {};                      // recorded after a slot's upload: the slot may be written again
  bool used_[kDrawStagingRing] = {};
  int next_ = 0;
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
  bool timed_ = false;
};

}  // namespace gtx

struct gtx_drawer {
  std::unique_ptr<gtx::Drawer> impl;
};
