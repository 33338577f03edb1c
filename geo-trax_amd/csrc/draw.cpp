// Host half of the drawing stage: validation of a primitive list (nothing is launched, and nothing is dropped, when a record is
// bad: the call fails with the record's index), the conservative boxes the kernel culls by (geotrax_amd/draw.py
// bounding_boxes), and the Drawer that stages a list through a small ring of pinned buffers and enqueues csrc/draw.hip.
#include "draw.hpp"

#include <algorithm>
#include <cstring>

#include "net_runtime.hpp"

namespace gtx {

namespace {
constexpr long long kCoordMin = -32768, kCoordMax = 32767;
inline bool coord_ok(int32_t v) { return v >= kCoordMin && v <= kCoordMax; }
inline int16_t clamp16(long long v) { return (int16_t)std::min(std::max(v, kCoordMin), kCoordMax); }
}  // namespace

void draw_check_frame(int h, int w) {
  if (h < 1 || w < 1 || h > kDrawMaxSide || w > kDrawMaxSide) fail(GTX_ERR_INVALID, "draw: a %d x %d frame is outside 1..%d", w, h, kDrawMaxSide);
}

void draw_check_prims(const int32_t* prims, int n, int max_prims, size_t atlas_bytes) {
  if (n < 0) fail(GTX_ERR_INVALID, "draw: n = %d", n);
  if (n > max_prims) fail(GTX_ERR_INVALID, "draw: %d primitives, the drawer holds %d", n, max_prims);
  if (n > 0 && !prims) fail(GTX_ERR_INVALID, "draw: prims is NULL with n = %d", n);
  for (int i = 0; i < n; ++i) {
    DrawPrim p;
    std::memcpy(&p, prims + 8 * (size_t)i, sizeof p);
    if (p.kind < kDrawFill || p.kind > kDrawGlyph) fail(GTX_ERR_INVALID, "draw: primitive %d: kind %d is not one of 0..3", i, p.kind);
    if (!coord_ok(p.x0) || !coord_ok(p.y0) || !coord_ok(p.x1) || !coord_ok(p.y1))
      fail(GTX_ERR_INVALID, "draw: primitive %d: a coordinate of (%d, %d, %d, %d) is outside [-32768, 32767]", i, p.x0, p.y0, p.x1, p.y1);
    if ((p.kind == kDrawSegment || p.kind == kDrawRing) && p.p0 < 1) fail(GTX_ERR_INVALID, "draw: primitive %d: thickness %d is below 1", i, p.p0);
    if (p.kind == kDrawRing && p.x1 < 0) fail(GTX_ERR_INVALID, "draw: primitive %d: radius %d is negative", i, p.x1);
    if (p.kind == kDrawGlyph) {
      const bool shape = p.x1 > 0 && p.y1 > 0 && p.p1 > 0 && p.p0 >= 0;
      // x1, y1 <= 32767 and p0, p1 < 2^31: the sum stays far inside int64
      const long long end = (long long)p.p0 + (long long)(p.y1 - 1) * p.p1 + p.x1;
      if (!shape || (unsigned long long)end > atlas_bytes)
        fail(GTX_ERR_INVALID, "draw: primitive %d: a %d x %d glyph cell at offset %d with pitch %d leaves the atlas of %zu bytes", i, p.x1, p.y1, p.p0,
             p.p1, atlas_bytes);
    }
  }
}

DrawBox draw_box(const DrawPrim& p) {
  long long x0 = std::min(p.x0, p.x1), x1 = std::max(p.x0, p.x1), y0 = std::min(p.y0, p.y1), y1 = std::max(p.y0, p.y1);
  if (p.kind == kDrawSegment) {
    const long long g = ((long long)p.p0 + 1) / 2 + 1;
    x0 -= g; y0 -= g; x1 += g; y1 += g;
  } else if (p.kind == kDrawRing) {
    const long long e = (long long)p.x1 + ((long long)p.p0 + 1) / 2;
    x0 = p.x0 - e; x1 = p.x0 + e; y0 = p.y0 - e; y1 = p.y0 + e;
  } else if (p.kind == kDrawGlyph) {
    x0 = p.x0; y0 = p.y0; x1 = (long long)p.x0 + p.x1 - 1; y1 = (long long)p.y0 + p.y1 - 1;
  }
  return DrawBox{clamp16(x0), clamp16(y0), clamp16(x1), clamp16(y1)};
}

void Drawer::check_args(int h, int w, int max_prims, const void* atlas, size_t atlas_bytes) {
  draw_check_frame(h, w);
  if (max_prims < 1 || max_prims > kDrawMaxPrims) fail(GTX_ERR_INVALID, "draw: max_prims %d is outside 1..%d", max_prims, kDrawMaxPrims);
  if (!atlas && atlas_bytes) fail(GTX_ERR_INVALID, "draw: atlas is NULL with %zu bytes", atlas_bytes);
  if (atlas_bytes > ((size_t)1 << 31)) fail(GTX_ERR_INVALID, "draw: an atlas of %zu bytes is larger than a record's offset can reach", atlas_bytes);
}

Drawer::Drawer(gtx_ctx* ctx, int h, int w, int max_prims, const void* atlas, size_t atlas_bytes)
    : ctx_(ctx), h_(h), w_(w), max_prims_(max_prims), atlas_bytes_(atlas_bytes) {
  check_args(h, w, max_prims, atlas, atlas_bytes);
  GTX_HIP(hipSetDevice(ctx_->device));
  const size_t stage = (size_t)max_prims * (sizeof(DrawPrim) + sizeof(DrawBox));
  try {
    d_atlas_.alloc(atlas_bytes);
    if (atlas_bytes) GTX_HIP(hipMemcpy(d_atlas_.p, atlas, atlas_bytes, hipMemcpyHostToDevice));
    d_stage_.alloc(stage);
    for (int k = 0; k < kDrawStagingRing; ++k) {
      GTX_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_stage_[k]), stage, hipHostMallocDefault));
      GTX_HIP(hipEventCreateWithFlags(&copied_[k], wait_event_flags(false)));
    }
    GTX_HIP(hipEventCreate(&e0_));
    GTX_HIP(hipEventCreate(&e1_));
  } catch (...) {
    release();
    throw;
  }
}

Drawer::~Drawer() { release(); }

void Drawer::release() {
  if (ctx_ && ctx_->stream) (void)hipStreamSynchronize(ctx_->stream);   // a queued upload may still read a pinned slot
  for (int k = 0; k < kDrawStagingRing; ++k) {
    if (h_stage_[k]) (void)hipHostFree(h_stage_[k]);
    if (copied_[k]) (void)hipEventDestroy(copied_[k]);
    h_stage_[k] = nullptr;
    copied_[k] = nullptr;
  }
  if (e0_) (void)hipEventDestroy(e0_);
  if (e1_) (void)hipEventDestroy(e1_);
  e0_ = e1_ = nullptr;
}

void Drawer::draw(void* frame_dptr, const int32_t* prims, int n) {
  timed_ = false;                                                   // a refused or empty list launches nothing: last_ms() reads 0
  if (!frame_dptr) fail(GTX_ERR_INVALID, "draw: frame is NULL");
  draw_check_prims(prims, n, max_prims_, atlas_bytes_);
  if (n == 0) return;
  GTX_HIP(hipSetDevice(ctx_->device));
  const int slot = next_;
  next_ = (next_ + 1) % kDrawStagingRing;
  if (used_[slot]) GTX_HIP(hipEventSynchronize(copied_[slot]));     // the upload that read this slot kDrawStagingRing calls ago
  uint8_t* hs = h_stage_[slot];
  const size_t rec_bytes = (size_t)n * sizeof(DrawPrim);
  std::memcpy(hs, prims, rec_bytes);
  const DrawPrim* hp = reinterpret_cast<const DrawPrim*>(hs);
  DrawBox* hb = reinterpret_cast<DrawBox*>(hs + rec_bytes);
  for (int i = 0; i < n; ++i) hb[i] = draw_box(hp[i]);
  // one buffer in HBM: the stream orders this upload behind the launch that read the list before
  GTX_HIP(hipMemcpyAsync(d_stage_.p, hs, rec_bytes + (size_t)n * sizeof(DrawBox), hipMemcpyHostToDevice, ctx_->stream));
  GTX_HIP(hipEventRecord(copied_[slot], ctx_->stream));
  used_[slot] = true;
  GTX_HIP(hipEventRecord(e0_, ctx_->stream));
  draw_launch(ctx_->stream, frame_dptr, h_, w_, d_stage_.as<DrawPrim>(), reinterpret_cast<const DrawBox*>(d_stage_.as<uint8_t>() + rec_bytes), n,
              d_atlas_.as<uint8_t>(), atlas_bytes_);
  GTX_HIP(hipEventRecord(e1_, ctx_->stream));
  timed_ = true;
}

float Drawer::last_ms() {
  if (!timed_) return 0.f;
  float ms = 0.f;
  GTX_HIP(hipSetDevice(ctx_->device));
  GTX_HIP(hipEventSynchronize(e1_));
  GTX_HIP(hipEventElapsedTime(&ms, e0_, e1_));
  return ms;
}

}  // namespace gtx
