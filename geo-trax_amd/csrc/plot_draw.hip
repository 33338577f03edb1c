// The kernels of the plot stage's trajectory maps: what plt.imshow(orthophoto) + plt.plot / plt.scatter per vehicle do in the
// reference's plot_trajectories_in_given_coordinates (geotrax/plot.py:419-488), on a canvas that stays in HBM. The pixel rule
// (quantisation, coverage, the maximum within a polyline, the blend, the boxes, the box average) is specified in
// geotrax_amd/plot_draw.py; tests/test_plot_draw_gpu.py holds these kernels to that twin byte for byte. The rule is integer
// arithmetic throughout: the one floating-point operation below, the square-root estimate in plot_cov, is corrected by integer
// comparisons to a value that two integer inequalities define, so no contraction or rounding mode can change a result.
//
// Binning: sized exactly from a counting pass, not chunked. count (one lane per primitive: an atomic per tile its clamped box
// overlaps, and the grand total) -> scan (one workgroup: exclusive prefix sum of the tile counts, and their maximum) -> the host
// reads the total and allocates the lists at exactly that size -> fill (the same walk, a slot from a per-tile cursor: every
// primitive gets one, in arbitrary order) -> sort (one workgroup per tile ranks its entries: the indices are distinct, so
// rank = how many are smaller; O(len^2) per tile through LDS, a few hundred entries in the lists a plot produces). No capacity
// constant exists that could drop a primitive, and the paint launch sees every tile's list in ascending index order, which is
// the list order the rule is a function of. Chunking the list instead would have cost a bin + paint pair per chunk, each paint
// loading and storing its tiles again; with exact lists every pixel is read and written once.
//
// Paint: one workgroup = one 64 x 16 tile, one lane = 4 consecutive pixels of a row in registers (draw.hip's layout). The list is
// staged through LDS kPlotChunk entries at a time; a lane keeps the running maximum coverage of the current polyline for its
// pixels and blends when the polyline's index changes. A tile with an empty list touches no pixel.
#include <hip/hip_runtime.h>

#include "plot_draw.hpp"

namespace gtx {

namespace {

// Coverage 0..256 of record p at pixel (x, y): geotrax_amd/plot_draw.py `coverage`, operation by operation. (x, y) lies inside p's
// box, where every product below stays inside int64 (the twin's docstring has the bounds).
__device__ __forceinline__ int plot_cov(const PlotPrim& p, int x, int y) {
  const long long px = 16LL * x, py = 16LL * y;
  const long long vx = (long long)p.x1 - p.x0, vy = (long long)p.y1 - p.y0, wx = px - p.x0, wy = py - p.y0;
  const long long L = vx * vx + vy * vy, s = wx * vx + wy * vy;
  long long num, den = 1;
  if (s <= 0) {
    num = wx * wx + wy * wy;
  } else if (s >= L) {
    const long long ex = px - p.x1, ey = py - p.y1;
    num = ex * ex + ey * ey;
  } else {
    const long long c = wx * vy - wy * vx;
    num = c * c;
    den = L;
  }
  const long long r1 = (long long)p.R - 1;
  if (num > ((r1 * r1 * den) >> 10)) return 0;
  const long long n = num << 10;
  long long e = (long long)sqrt((double)n / (double)den);          // an estimate only: the two loops below fix the integer
  while (e > 0 && (e - 1) * (e - 1) * den >= n) --e;
  while (e * e * den < n) ++e;
  const long long v = ((long long)p.R + 1 - e) >> 1;
  return v >= 256 ? 256 : (int)v;
}

__global__ __launch_bounds__(256) void plot_reduce_kernel(const uint8_t* __restrict__ src, int h, int w, int ch, int k, uint8_t* __restrict__ dst, int ho,
                                                          int wo) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
  if (ox >= wo || oy >= ho) return;
  const int y0 = oy * k, x0 = ox * k, y1 = min(y0 + k, h), x1 = min(x0 + k, w);
  int sum[3] = {0, 0, 0};
  for (int y = y0; y < y1; ++y) {
    const uint8_t* row = src + ((size_t)y * w + x0) * ch;
    for (int x = x0; x < x1; ++x, row += ch) {
      if (ch == 1) {
        const int g = row[0];
        sum[0] += g, sum[1] += g, sum[2] += g;
      } else {                                                     // RGB(A) -> BGR
        sum[0] += row[2], sum[1] += row[1], sum[2] += row[0];
      }
    }
  }
  const int n = (y1 - y0) * (x1 - x0);                             // >= 1: (ox, oy) is inside the reduced picture
  uint8_t* o = dst + ((size_t)oy * wo + ox) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((2 * sum[c] + n) / (2 * n));
}

// the tiles a box touches after clamping to the canvas; false: none (the primitive is binned nowhere)
__device__ __forceinline__ bool plot_tile_range(const PlotBox& b, int h, int w, int& tx0, int& ty0, int& tx1, int& ty1) {
  const int x0 = max((int)b.x0, 0), y0 = max((int)b.y0, 0), x1 = min((int)b.x1, w - 1), y1 = min((int)b.y1, h - 1);
  if (x0 > x1 || y0 > y1) return false;
  tx0 = x0 / kPlotTileW, tx1 = x1 / kPlotTileW, ty0 = y0 / kPlotTileH, ty1 = y1 / kPlotTileH;
  return true;
}

__global__ __launch_bounds__(256) void plot_count_kernel(const PlotBox* __restrict__ boxes, int n, int h, int w, int tiles_x, uint32_t* __restrict__ counts,
                                                         unsigned long long* __restrict__ total) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int tx0, ty0, tx1, ty1;
  if (!plot_tile_range(boxes[i], h, w, tx0, ty0, tx1, ty1)) return;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) atomicAdd(&counts[(size_t)ty * tiles_x + tx], 1u);
  atomicAdd(total, (unsigned long long)(tx1 - tx0 + 1) * (unsigned long long)(ty1 - ty0 + 1));
}

// One workgroup: offsets[t] = sum of counts[0, t), offsets[n_tiles] = the total (mod 2^32: the host has the 64-bit total from the
// counting pass and launches nothing further when it does not fit), *max_count = the longest list.
__global__ __launch_bounds__(256) void plot_scan_kernel(const uint32_t* __restrict__ counts, int n_tiles, uint32_t* __restrict__ offsets,
                                                        uint32_t* __restrict__ max_count) {
  __shared__ uint32_t s_sum[256];
  const int tid = threadIdx.x;
  uint32_t carry = 0, longest = 0;
  for (int base = 0; base < n_tiles; base += 256 * kPlotScanPerLane) {
    const int first = base + tid * kPlotScanPerLane;
    uint32_t v[kPlotScanPerLane], mine = 0;
#pragma unroll
    for (int k = 0; k < kPlotScanPerLane; ++k) {
      v[k] = first + k < n_tiles ? counts[first + k] : 0u;
      mine += v[k];
      longest = max(longest, v[k]);
    }
    s_sum[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                            // inclusive scan of the lanes' sums
      const uint32_t add = tid >= d ? s_sum[tid - d] : 0u;
      __syncthreads();
      s_sum[tid] += add;
      __syncthreads();
    }
    uint32_t run = carry + s_sum[tid] - mine;
#pragma unroll
    for (int k = 0; k < kPlotScanPerLane; ++k) {
      if (first + k < n_tiles) offsets[first + k] = run;
      run += v[k];
    }
    carry += s_sum[255];
    __syncthreads();                                               // s_sum is written again by the next round
  }
  if (tid == 0) offsets[n_tiles] = carry;
  s_sum[tid] = longest;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if (tid < d) s_sum[tid] = max(s_sum[tid], s_sum[tid + d]);
    __syncthreads();
  }
  if (tid == 0) *max_count = s_sum[0];
}

__global__ __launch_bounds__(256) void plot_fill_kernel(const PlotBox* __restrict__ boxes, int n, int h, int w, int tiles_x,
                                                        const uint32_t* __restrict__ offsets, uint32_t* __restrict__ cursor, uint32_t* __restrict__ list,
                                                        uint32_t entries) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int tx0, ty0, tx1, ty1;
  if (!plot_tile_range(boxes[i], h, w, tx0, ty0, tx1, ty1)) return;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) {
      const size_t t = (size_t)ty * tiles_x + tx;
      const uint32_t pos = offsets[t] + atomicAdd(&cursor[t], 1u);
      if (pos < offsets[t + 1] && pos < entries) list[pos] = (uint32_t)i;   // always true: the counting pass walked the same tiles
    }
}

// One workgroup per tile: sorted[beg + rank] = v for every entry v of list[beg, end), rank = the number of entries below v.
__global__ __launch_bounds__(256) void plot_sort_kernel(const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ list,
                                                        uint32_t* __restrict__ sorted, uint32_t entries) {
  __shared__ uint32_t s_v[256];
  const int tid = threadIdx.x;
  const uint32_t beg = offsets[blockIdx.x], end = min(offsets[blockIdx.x + 1], entries);
  if (beg >= end) return;
  for (uint32_t ib = beg; ib < end; ib += 256) {
    const bool have = ib + tid < end;
    const uint32_t v = have ? list[ib + tid] : 0u;
    uint32_t rank = 0;
    for (uint32_t jb = beg; jb < end; jb += 256) {
      __syncthreads();                                             // the previous chunk has been read
      s_v[tid] = jb + tid < end ? list[jb + tid] : 0xFFFFFFFFu;    // larger than every index
      __syncthreads();
      const int m = (int)min(256u, end - jb);
      for (int j = 0; j < m; ++j) rank += s_v[j] < v ? 1u : 0u;
    }
    if (have && beg + rank < end) sorted[beg + rank] = v;
  }
}

__global__ __launch_bounds__(kPlotChunk) void plot_paint_kernel(uint8_t* __restrict__ canvas, int h, int w, size_t pitch, const PlotPrim* __restrict__ prims,
                                                                const PlotBox* __restrict__ boxes, int n, const uint32_t* __restrict__ offsets,
                                                                const uint32_t* __restrict__ sorted, uint32_t entries) {
  __shared__ PlotPrim s_prim[kPlotChunk];
  __shared__ PlotBox s_box[kPlotChunk];
  const int tid = threadIdx.x;
  const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  const uint32_t beg = offsets[tile], end = min(offsets[tile + 1], entries);
  if (beg >= end) return;                                           // the whole workgroup: nothing reaches this tile
  const int y = blockIdx.y * kPlotTileH + (tid >> 4), xq = blockIdx.x * kPlotTileW + 4 * (tid & 15);
  const int npx = (y < h && xq < w) ? min(4, w - xq) : 0;           // pixels this lane owns (0: it only helps with the list)
  uint8_t* const row = canvas + (size_t)y * pitch + (size_t)xq * 3; // dereferenced only when npx > 0
  const bool words = npx == 4 && (reinterpret_cast<uintptr_t>(row) & 3) == 0;
  int px[12], mc[4] = {0, 0, 0, 0};
  if (npx > 0) {
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
  int cur_run = -1, cur_bgr = 0, cur_alpha = 0;
  auto flush = [&]() {
    const int col[3] = {cur_bgr & 255, (cur_bgr >> 8) & 255, (cur_bgr >> 16) & 255};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (mc[j] > 0) {
        const int f = cur_alpha * mc[j];
#pragma unroll
        for (int c = 0; c < 3; ++c) px[3 * j + c] += ((col[c] - px[3 * j + c]) * f + 32768) >> 16;
        mc[j] = 0;
      }
    }
  };

  for (uint32_t base = beg; base < end; base += kPlotChunk) {
    const int m = (int)min((uint32_t)kPlotChunk, end - base);
    __syncthreads();                                                // the previous chunk has been painted
    if (tid < m) {
      const uint32_t i = sorted[base + tid];
      const bool ok = i < (uint32_t)n;
      s_prim[tid] = ok ? prims[i] : PlotPrim{0, 0, 0, 0, 1, 0, 0, -2};
      s_box[tid] = ok ? boxes[i] : PlotBox{1, 1, 0, 0};             // an empty box: covers nothing
    }
    __syncthreads();
    if (npx > 0) {
      for (int k = 0; k < m; ++k) {
        const int run = s_prim[k].run;
        if (run != cur_run) {
          flush();
          cur_run = run, cur_bgr = s_prim[k].bgr, cur_alpha = s_prim[k].alpha;
        }
        const PlotBox kb = s_box[k];
        if (y < kb.y0 || y > kb.y1 || xq > kb.x1 || xq + npx - 1 < kb.x0) continue;   // no pixel outside the box is covered
        const PlotPrim p = s_prim[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = xq + j;
          if (j >= npx || x < kb.x0 || x > kb.x1) continue;
          mc[j] = max(mc[j], plot_cov(p, x, y));
        }
      }
    }
  }
  if (npx == 0) return;
  flush();
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

}  // namespace

void plot_reduce_launch(hipStream_t stream, const uint8_t* src, int h, int w, int channels, int k, uint8_t* dst_bgr) {
  const int ho = cdiv(h, k), wo = cdiv(w, k);
  hipLaunchKernelGGL(plot_reduce_kernel, dim3(cdiv(wo, 256), ho), dim3(256), 0, stream, src, h, w, channels, k, dst_bgr, ho, wo);
  GTX_HIP(hipGetLastError());
}

void plot_count_launch(hipStream_t stream, const PlotBox* boxes, int n, int h, int w, uint32_t* counts, unsigned long long* total) {
  hipLaunchKernelGGL(plot_count_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, boxes, n, h, w, cdiv(w, kPlotTileW), counts, total);
  GTX_HIP(hipGetLastError());
}

void plot_scan_launch(hipStream_t stream, const uint32_t* counts, int n_tiles, uint32_t* offsets, uint32_t* max_count) {
  hipLaunchKernelGGL(plot_scan_kernel, dim3(1), dim3(256), 0, stream, counts, n_tiles, offsets, max_count);
  GTX_HIP(hipGetLastError());
}

void plot_fill_launch(hipStream_t stream, const PlotBox* boxes, int n, int h, int w, const uint32_t* offsets, uint32_t* cursor, uint32_t* list,
                      uint32_t entries) {
  hipLaunchKernelGGL(plot_fill_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, boxes, n, h, w, cdiv(w, kPlotTileW), offsets, cursor, list, entries);
  GTX_HIP(hipGetLastError());
}

void plot_sort_launch(hipStream_t stream, const uint32_t* offsets, int n_tiles, const uint32_t* list, uint32_t* sorted, uint32_t entries) {
  hipLaunchKernelGGL(plot_sort_kernel, dim3(n_tiles), dim3(256), 0, stream, offsets, list, sorted, entries);
  GTX_HIP(hipGetLastError());
}

void plot_paint_launch(hipStream_t stream, uint8_t* canvas, int h, int w, size_t pitch, const PlotPrim* prims, const PlotBox* boxes, int n,
                       const uint32_t* offsets, const uint32_t* sorted, uint32_t entries) {
  hipLaunchKernelGGL(plot_paint_kernel, dim3(cdiv(w, kPlotTileW), cdiv(h, kPlotTileH)), dim3(kPlotChunk), 0, stream, canvas, h, w, pitch, prims, boxes, n,
                     offsets, sorted, entries);
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
