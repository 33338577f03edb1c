// The drawing kernel for the visualize stage: what cv2.rectangle / cv2.line / cv2.polylines / cv2.circle / cv2.putText do to the frame
// in the reference's annotate_frame and draw_oriented_box (geotrax/visualize.py:662-940), as one launch on a frame that stays in HBM.
// The pixel rule (coverage per primitive kind, the blend, painter's order, the conservative boxes) is specified in
// geotrax_amd/draw.py; tests/test_draw_ops_gpu.py holds this kernel to that twin byte for byte. This file is compiled with
// -ffp-contract=off: the float64 sequence of the SEGMENT coverage is the stated one, one rounding per operation.
//
// One workgroup = one 64 x 16 tile of the frame, one lane = 4 consecutive pixels of a row, carried in registers. The workgroup
// walks the primitive list in chunks of its own size: each lane tests one primitive's box (8 bytes) against the tile, a ballot
// and a prefix over the four waves' counts put the hits into LDS in index order (no atomics: the order is the list's), and every
// lane then paints its pixels with that chunk's hits. A tile loads its pixels when the first hit arrives and stores them once at
// the end; a tile nothing reaches touches no pixel. Every index that becomes an address is checked here against h, w, n and
// atlas_bytes, whatever the host has validated.
//
// Cost: every tile reads every primitive's box, ceil(n / 256) chunks with two barriers each, so the launch grows as tiles x n
// (a 4K frame with 6 000 primitives: 8 100 tiles x 6 000 x 8 bytes = 390 MB of L2 reads, 0.12 ms). A coarse pass that bins the
// primitives per group of tiles first would remove that product; it has not been needed yet.
#include <hip/hip_runtime.h>

#include "draw.hpp"

namespace gtx {

namespace {

// Coverage 0..256 of primitive p at pixel (x, y): geotrax_amd/draw.py `coverage`, operation by operation.
__device__ __forceinline__ int draw_coverage(const DrawPrim& p, int x, int y, const uint8_t* __restrict__ atlas, size_t atlas_bytes) {
  switch (p.kind) {
    case kDrawFill:
      return (x >= min(p.x0, p.x1) && x <= max(p.x0, p.x1) && y >= min(p.y0, p.y1) && y <= max(p.y0, p.y1)) ? 256 : 0;
    case kDrawSegment: {
      const long long vx = (long long)p.x1 - p.x0, vy = (long long)p.y1 - p.y0, wx = (long long)x - p.x0, wy = (long long)y - p.y0;
      const long long L = vx * vx + vy * vy, s = wx * vx + wy * vy;
      double d2;
      if (s <= 0) {
        d2 = (double)(wx * wx + wy * wy);
      } else if (s >= L) {
        const long long ex = (long long)x - p.x1, ey = (long long)y - p.y1;
        d2 = (double)(ex * ex + ey * ey);
      } else {
        const double c = (double)(wx * vy - wy * vx);
        d2 = c * c / (double)L;
      }
      const double v = floor(((0.5 * (double)p.p0 + 0.5) - sqrt(d2)) * 256.0 + 0.5);
      return v <= 0.0 ? 0 : v >= 256.0 ? 256 : (int)v;
    }
    case kDrawRing: {
      const long long dx = (long long)x - p.x0, dy = (long long)y - p.y0, D = 4 * (dx * dx + dy * dy);
      const long long in = max(2LL * p.x1 - p.p0, 0LL), out = 2LL * p.x1 + p.p0;
      return (D >= in * in && D <= out * out) ? 256 : 0;
    }
    case kDrawGlyph: {
      const int cx = x - p.x0, cy = y - p.y0;
      if (cx < 0 || cx >= p.x1 || cy < 0 || cy >= p.y1) return 0;
      const long long off = (long long)p.p0 + (long long)cy * p.p1 + cx;
      if (off < 0 || (unsigned long long)off >= atlas_bytes) return 0;
      const int c = atlas[off];
      return c + (c >> 7);
    }
    default:
      return 0;
  }
}

__global__ __launch_bounds__(kDrawChunk) void draw_kernel(uint8_t* __restrict__ frame, int h, int w, const DrawPrim* __restrict__ prims,
                                                          const DrawBox* __restrict__ boxes, int n, const uint8_t* __restrict__ atlas,
                                                          size_t atlas_bytes) {
  __shared__ DrawPrim s_prim[kDrawChunk];
  __shared__ DrawBox s_box[kDrawChunk];
  __shared__ int s_count[kDrawChunk / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = blockIdx.x * kDrawTileW, ty0 = blockIdx.y * kDrawTileH;
  const int tx1 = min(tx0 + kDrawTileW, w) - 1, ty1 = min(ty0 + kDrawTileH, h) - 1;
  const int y = ty0 + (tid >> 4), xq = tx0 + 4 * (tid & 15);
  const int npx = (y < h && xq < w) ? min(4, w - xq) : 0;           // pixels this lane owns (0: it only helps with the list)
  uint8_t* const row = frame + ((size_t)y * w + xq) * 3;            // dereferenced only when npx > 0
  const bool words = npx == 4 && (reinterpret_cast<uintptr_t>(row) & 3) == 0;
  int px[12];
  bool loaded = false;

  for (int base = 0; base < n; base += kDrawChunk) {
    const int i = base + tid;
    bool hit = false;
    DrawBox b{};
    if (i < n) {
      b = boxes[i];
      hit = b.x0 <= tx1 && b.x1 >= tx0 && b.y0 <= ty1 && b.y1 >= ty0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_count[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kDrawChunk / 64; ++k) {
      const int c = s_count[k];
      before += k < wave ? c : 0;
      total += c;
    }
    if (hit) {
      const int slot = before + __popcll(m & ((1ull << lane) - 1ull));   // < total <= kDrawChunk
      s_prim[slot] = prims[i];
      s_box[slot] = b;
    }
    __syncthreads();
    if (total > 0 && npx > 0) {
      if (!loaded) {
        loaded = true;
        if (words) {
          const uint32_t* r4 = reinterpret_cast<const uint32_t*>(row);
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const uint32_t v = r4[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) px[4 * q + k] = (v >> (8 * k)) & 255;
          }
        } else {
#pragma unroll
          for (int k = 0; k < 12; ++k) px[k] = k < 3 * npx ? row[k] : 0;
        }
      }
      for (int k = 0; k < total; ++k) {
        const DrawBox kb = s_box[k];
        if (y < kb.y0 || y > kb.y1 || xq > kb.x1 || xq + npx - 1 < kb.x0) continue;   // no pixel outside the box is covered
        const DrawPrim p = s_prim[k];
        const int col[3] = {p.bgr & 255, (p.bgr >> 8) & 255, (p.bgr >> 16) & 255};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = xq + j;
          if (j >= npx || x < kb.x0 || x > kb.x1) continue;
          const int a = draw_coverage(p, x, y, atlas, atlas_bytes);
          if (a == 0) continue;
#pragma unroll
          for (int c = 0; c < 3; ++c) px[3 * j + c] = (px[3 * j + c] * (256 - a) + col[c] * a + 128) >> 8;
        }
      }
    }
    // the next chunk writes s_count after this chunk's second barrier and s_prim / s_box after its own first one, which a lane
    // reaches only when it has left the loop above
  }

  if (loaded) {
    if (words) {
      uint32_t* r4 = reinterpret_cast<uint32_t*>(row);
#pragma unroll
      for (int q = 0; q < 3; ++q) r4[q] = (uint32_t)px[4 * q] | (uint32_t)px[4 * q + 1] << 8 | (uint32_t)px[4 * q + 2] << 16 | (uint32_t)px[4 * q + 3] << 24;
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (k < 3 * npx) row[k] = (uint8_t)px[k];
    }
  }
}

}  // namespace

void draw_launch(hipStream_t stream, void* frame, int h, int w, const DrawPrim* d_prims, const DrawBox* d_boxes, int n, const uint8_t* d_atlas,
                 size_t atlas_bytes) {
  hipLaunchKernelGGL(draw_kernel, dim3(cdiv(w, kDrawTileW), cdiv(h, kDrawTileH)), dim3(kDrawChunk), 0, stream, static_cast<uint8_t*>(frame), h, w,
                     d_prims, d_boxes, n, d_atlas, atlas_bytes);
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
