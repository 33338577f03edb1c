// YOLOv9's downsampling pools (pool_down.hpp): avg_pool2d(2, 1) for AConv / ADown's convolution half and the same average followed by
// max_pool2d(3, 2, 1) for ADown's other half, in one launch. gfx950 only.
//
// Bound by memory traffic: nothing but additions and maxima per byte (measured: profiles/yolov9_time.txt).
// A lane owns one 8-channel group (16 bytes of fp16, 32 of fp32 or of the pair format: whole dwordx4 accesses) at one column and walks down a strip of rows, so a wave reads runs of consecutive groups and
// pixels along W. Rows are reused in registers: the average keeps the horizontal sums of the row above (every input row is added
// once per strip instead of twice), the maximum keeps the horizontal sums of the row above and the pooled row it shares with the
// next output row (four input rows per output row become two). What a lane's neighbour reads again -- one column of two for the
// average, two of four for the maximum -- and the one or two halo rows of a strip come out of L2. The two halves of an ADown run in
// different workgroups of the one launch: the chunk is on channels, so the first blocks take the average's channel range and the
// rest the maximum's.
#include "pool_down.hpp"

#include <cmath>

namespace gtx {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int kAvgRows = 8;   // output rows of the average per strip (+ 1 halo row read)
constexpr int kMaxRows = 4;   // output rows of the maximum per strip: 8 input rows (+ 2 halo rows read)

// ---- 8-channel groups in the three activation formats; e = element index of the group's first channel (a multiple of 8)
template <int FMT> __device__ __forceinline__ void load8(const void* base, size_t e, float v[8]) {
  const char* b = static_cast<const char*>(base);
  if constexpr (FMT == DT_F16) {
    const half8 h = *reinterpret_cast<const half8*>(b + e * 2);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
  } else if constexpr (FMT == DT_F32) {
    const float4 a = *reinterpret_cast<const float4*>(b + e * 4), c = *reinterpret_cast<const float4*>(b + e * 4 + 16);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
  } else {                                                       // pair format: 8 hi halves then 8 lo halves (split_format.hpp)
    const half8 hi = *reinterpret_cast<const half8*>(b + e * 4), lo = *reinterpret_cast<const half8*>(b + e * 4 + 16);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)hi[i] + (float)lo[i];
  }
}
// |v| never exceeds the largest input here, which came out of the same format: no clamp, no saturation flag
template <int FMT> __device__ __forceinline__ void store8(void* base, size_t e, const float v[8]) {
  char* b = static_cast<char*>(base);
  if constexpr (FMT == DT_F16) {
    half8 h;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = (_Float16)v[i];
    *reinterpret_cast<half8*>(b + e * 2) = h;
  } else if constexpr (FMT == DT_F32) {
    *reinterpret_cast<float4*>(b + e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(b + e * 4 + 16) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    half8 hi, lo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      hi[i] = (_Float16)v[i];
      lo[i] = (_Float16)(v[i] - (float)hi[i]);                             // v - hi is exact in fp32
    }
    *reinterpret_cast<half8*>(b + e * 4) = hi;
    *reinterpret_cast<half8*>(b + e * 4 + 16) = lo;
  }
}

struct PoolDown {
  RtMap in, avg, mx;
  int n;
  unsigned avg_blocks;      // the launch's first avg_blocks workgroups take the average, the others the maximum
  size_t avg_items, max_items;
};

// in(r, x) + in(r, x + 1) of one 8-channel group: the horizontal half of the 2 x 2 average
template <int FMT> __device__ __forceinline__ void hsum(const RtMap& in, size_t row, int x, int ch, float hs[8]) {
  float a[8], b[8];
  load8<FMT>(in.ptr, (row * in.w + x) * in.cstride + ch, a);
  load8<FMT>(in.ptr, (row * in.w + x + 1) * in.cstride + ch, b);
#pragma unroll
  for (int i = 0; i < 8; ++i) hs[i] = a[i] + b[i];
}

// the three horizontal sums a 3-wide window of the pooled map at pooled columns 2 ox - 1 .. 2 ox + 1 needs of input row `row`
// (input columns 2 ox - 1 .. 2 ox + 2); lo / hi: whether the first / last pooled column exists
template <int FMT> __device__ __forceinline__ void hsum3(const RtMap& in, size_t row, int ox, int ch, bool lo, bool hi, float hs[3][8]) {
  float v[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool ok = (j > 0 || lo) && (j < 3 || hi);
    if (ok) {
      load8<FMT>(in.ptr, (row * in.w + (2 * ox - 1 + j)) * in.cstride + ch, v[j]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[j][i] = 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) hs[j][i] = v[j][i] + v[j + 1][i];
}

template <int FMT>
__global__ __launch_bounds__(256) void pool_down_kernel(PoolDown P) {
  const RtMap &in = P.in;
  const int H = in.h, W = in.w;
  if (blockIdx.x < P.avg_blocks) {
    // ---- out(y, x) = 0.25 ((in(y, x) + in(y, x + 1)) + (in(y + 1, x) + in(y + 1, x + 1))); the last row and column: zeros
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= P.avg_items) return;
    const int G = P.avg.c / 8, strips = (H + kAvgRows - 1) / kAvgRows;
    const int g = (int)(idx % G), x = (int)(idx / G % W), strip = (int)(idx / ((size_t)G * W) % strips);
    const size_t img = idx / ((size_t)G * W * strips);
    const int y0 = strip * kAvgRows, y1 = min(y0 + kAvgRows, H);
    const int ch_in = in.coff + g * 8, ch_out = P.avg.coff + g * 8;
    const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float top[8], bot[8], o[8];
    if (x < W - 1) hsum<FMT>(in, img * H + y0, x, ch_in, top);
    for (int y = y0; y < y1; ++y) {
      const size_t e = ((img * H + y) * W + x) * P.avg.cstride + ch_out;
      if (x == W - 1 || y == H - 1) {
        store8<FMT>(P.avg.ptr, e, zero);
        continue;
      }
      hsum<FMT>(in, img * H + y + 1, x, ch_in, bot);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o[i] = 0.25f * (top[i] + bot[i]);
        top[i] = bot[i];
      }
      store8<FMT>(P.avg.ptr, e, o);
    }
    return;
  }
  // ---- out(oy, ox) = max over the pooled rows 2 oy - 1 .. 2 oy + 1 and columns 2 ox - 1 .. 2 ox + 1 that exist (0 .. H - 2, 0 .. W - 2)
  const size_t idx = (size_t)(blockIdx.x - P.avg_blocks) * 256 + threadIdx.x;
  if (idx >= P.max_items) return;
  const int Ho = H / 2, Wo = W / 2;
  const int G = P.mx.c / 8, strips = (Ho + kMaxRows - 1) / kMaxRows;
  const int g = (int)(idx % G), ox = (int)(idx / G % Wo), strip = (int)(idx / ((size_t)G * Wo) % strips);
  const size_t img = idx / ((size_t)G * Wo * strips);
  const int oy0 = strip * kMaxRows, oy1 = min(oy0 + kMaxRows, Ho);
  const int ch_in = in.coff + P.avg.c + g * 8, ch_out = P.mx.coff + g * 8;
  const bool lo = ox > 0, hi = ox < Wo - 1;
  float prev[3][8], cur[3][8], acc[8], carry[8];
  int p = oy0 > 0 ? 2 * oy0 - 1 : 0;                 // the next pooled row; prev holds the horizontal sums of input row p
  hsum3<FMT>(in, img * H + p, ox, ch_in, lo, hi, prev);
  // the maximum of pooled row p over the window's columns into m (combined with what m holds when join), then on to row p + 1
  auto pooled_row = [&](float m[8], bool join) {
    hsum3<FMT>(in, img * H + p + 1, ox, ch_in, lo, hi, cur);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = 0.25f * (prev[1][i] + cur[1][i]);    // pooled column 2 ox: always there
      if (lo) v = fmaxf(v, 0.25f * (prev[0][i] + cur[0][i]));
      if (hi) v = fmaxf(v, 0.25f * (prev[2][i] + cur[2][i]));
      m[i] = join ? fmaxf(m[i], v) : v;
#pragma unroll
      for (int j = 0; j < 3; ++j) prev[j][i] = cur[j][i];
    }
    ++p;
  };
  for (int oy = oy0; oy < oy1; ++oy) {
    bool have = false;
    if (oy > oy0) {                                  // pooled row 2 oy - 1 was the row below of the output row above
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = carry[i];
      have = true;
    } else if (oy > 0) {
      pooled_row(acc, false);
      have = true;
    }
    pooled_row(acc, have);                           // pooled row 2 oy <= H - 2
    if (2 * oy + 1 <= H - 2) {
      pooled_row(carry, false);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaxf(acc[i], carry[i]);
    }
    store8<FMT>(P.mx.ptr, ((img * Ho + oy) * Wo + ox) * P.mx.cstride + ch_out, acc);
  }
}

bool slice_ok(const RtMap& m) { return m.c > 0 && m.c % 8 == 0 && m.cstride % 8 == 0 && m.coff % 8 == 0 && m.coff >= 0 && m.coff + m.c <= m.cstride; }

}  // namespace

const char* pool_down_refusal(int fmt, const RtMap& in, const RtMap& avg, const RtMap& mx, int n) {
  if (fmt != DT_F16 && fmt != DT_F32 && fmt != DT_F32S) return "unsupported map format";
  if (n < 1) return "no image";
  if (in.h < 2 || in.w < 2) return "the map must be at least 2 x 2";
  if (in.h % 2 || in.w % 2) return "the map's height and width must be even";
  if (!slice_ok(in) || !slice_ok(avg) || (mx.c != 0 && !slice_ok(mx)))
    return "channel counts, strides and offsets must be multiples of 8 and every slice must fit its stride";
  if (mx.c < 0 || in.c != avg.c + mx.c) return "the input's channels must be the average's followed by the maximum's";
  if (avg.h != in.h || avg.w != in.w) return "the average is stored at the input's size (last row and column zero)";
  if (mx.c != 0 && (mx.h != in.h / 2 || mx.w != in.w / 2)) return "the maximum is stored at half the input's size";
  if (!in.ptr || !avg.ptr || (mx.c != 0 && !mx.ptr)) return "a map has no buffer";
  const size_t items = (size_t)n * cdiv(in.h, kAvgRows) * in.w * (avg.c / 8) + (size_t)n * cdiv(in.h / 2, kMaxRows) * (in.w / 2) * (mx.c / 8);
  if (items / 256 + 2 > 0x7fffffffu) return "too many workgroups for one launch";
  return nullptr;
}

void launch_pool_down(int fmt, const RtMap& in, const RtMap& avg, const RtMap& mx, int n, hipStream_t s) {
  const char* why = pool_down_refusal(fmt, in, avg, mx, n);
  GTX_CHECK(!why, "pool_down: %s", why);
  PoolDown P{in, avg, mx, n, 0, 0, 0};
  P.avg_items = (size_t)n * cdiv(in.h, kAvgRows) * in.w * (avg.c / 8);
  P.max_items = (size_t)n * cdiv(in.h / 2, kMaxRows) * (in.w / 2) * (mx.c / 8);
  P.avg_blocks = (unsigned)((P.avg_items + 255) / 256);
  const unsigned blocks = P.avg_blocks + (unsigned)((P.max_items + 255) / 256);
  if (fmt == DT_F16) hipLaunchKernelGGL(pool_down_kernel<DT_F16>, dim3(blocks), dim3(256), 0, s, P);
  else if (fmt == DT_F32) hipLaunchKernelGGL(pool_down_kernel<DT_F32>, dim3(blocks), dim3(256), 0, s, P);
  else hipLaunchKernelGGL(pool_down_kernel<DT_F32S>, dim3(blocks), dim3(256), 0, s, P);
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
