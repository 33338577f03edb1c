// yolov5.yaml's 6x6 stride-2 stem (see stem6.hpp). gfx950 only.
//
// The layer writes the network's largest tensor (c0 x 4 bytes per output pixel on the default path, 118 MB per 1920 x 1920 frame at
// c0 = 32) from its smallest (4 bytes per input pixel), so the image side is what the tiling can spoil: an output reads a 6 x 6 window,
// horizontally adjacent outputs share 4 of its 6 columns, vertically adjacent ones 4 of its 6 rows. A workgroup therefore stages the
// patch of its tile of outputs in LDS once -- (2 rows + 4) x (2 * 32 + 4) pixels, every byte converted through a 256-entry table
// on the way (fp16 of v / 255, or its hi + lo pair) -- and all its outputs read their windows from there: 1.6 loaded pixels per
// output pixel pair instead of 36.
// The matrix-core kernels are an implicit GEMM D[cout 32][pixel 32] += W[cout][k] X[k][pixel] on mfma_f32_32x32x16_f16 with k = the 108
// taps in w108's row order (ky, kx, colour), padded with four zero taps to 112 = 7 steps. The patch is stored [row][column][colour] in
// halves, so the 18 taps of one window row are 9 consecutive dwords and a lane's fragment (8 consecutive k) is 4 dword reads; a wave's
// 32 pixels sit 3 dwords apart, which spreads them over all 32 banks. One wave takes one output row of the tile, keeps its seven pixel
// fragments in registers and walks the groups of 32 output channels with them. Epilogues are the 3x3 stem's (det_kernels.hip).
#include "stem6.hpp"

#include <cmath>

#include "conv_igemm.hpp"

namespace gtx {

namespace {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx16_t __attribute__((ext_vector_type(16)));

constexpr int kCols = kStem6Cols;            // output columns per tile
constexpr int kPatchCols = 2 * kCols + 4;    // image columns 2 ox0 - 2 .. 2 (ox0 + 31) + 3
constexpr int kSteps = 7;                    // k-steps of 16: 108 taps + 4 zero taps
constexpr int kTapDwords = 54;               // 108 halves

__device__ __forceinline__ float silu_f(float v) { return v * __builtin_amdgcn_rcpf(1.f + __expf(-v)); }

// The RGB0 word of patch pixel (py, px) of the tile at (oy0, ox0); 0 -- the value 0.0, the convolution's padding -- beyond the border
__device__ __forceinline__ unsigned patch_word(const uchar4* base, int h, int w, int oy0, int ox0, int py, int px) {
  const int iy = 2 * oy0 - 2 + py, ix = 2 * ox0 - 2 + px;
  if (iy < 0 || iy >= h || ix < 0 || ix >= w) return 0u;
  return reinterpret_cast<const unsigned*>(base)[(unsigned)(iy * w + ix)];     // offsets fit 32 bits (one image)
}

// kSplit: pixels and weights as hi + lo halves, three MFMAs per product, pair-format output (split_format.hpp); else fp16 throughout
template <bool kSplit>
__device__ __forceinline__ void stem6_mma(const uchar4* __restrict__ img, int h, int w, const _Float16* __restrict__ wpk,
                                          const float* __restrict__ bias, float acc_scale, void* __restrict__ out, int ho, int wo, int c0,
                                          int groups) {
  constexpr int kRows = kStem6Rows, kPatchRows = 2 * kRows + 4;
  constexpr int kPitch = kPatchCols * 3 / 2;                        // dwords per patch row (204 halves)
  __shared__ unsigned s_hi[kPatchRows * kPitch];
  __shared__ unsigned s_lo[kSplit ? kPatchRows * kPitch : 1];
  __shared__ unsigned s_lut[256];                                   // byte -> hi | lo << 16 of byte / 255 (fp16 path: lo unused)
  {
    const float f = (float)threadIdx.x / 255.f;
    const _Float16 hi = (_Float16)f, lo = (_Float16)(f - (float)hi);
    s_lut[threadIdx.x] = (unsigned)__builtin_bit_cast(unsigned short, hi) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
  }
  __syncthreads();
  const int ox0 = blockIdx.x * kCols, oy0 = blockIdx.y * kRows, n = blockIdx.z;
  const uchar4* base = img + (size_t)n * h * w;
  // two neighbouring pixels per thread and turn: 6 halves = 3 dwords of the patch row
  for (int i = threadIdx.x; i < kPatchRows * (kPatchCols / 2); i += blockDim.x) {
    const int py = i / (kPatchCols / 2), pp = i - py * (kPatchCols / 2);
    const unsigned a = patch_word(base, h, w, oy0, ox0, py, 2 * pp), b = patch_word(base, h, w, oy0, ox0, py, 2 * pp + 1);
    const unsigned e[6] = {s_lut[a & 255u], s_lut[(a >> 8) & 255u], s_lut[(a >> 16) & 255u],
                           s_lut[b & 255u], s_lut[(b >> 8) & 255u], s_lut[(b >> 16) & 255u]};
    const int d = py * kPitch + 3 * pp;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      s_hi[d + q] = (e[2 * q] & 0xffffu) | (e[2 * q + 1] << 16);
      if (kSplit) s_lo[d + q] = (e[2 * q] >> 16) | (e[2 * q + 1] & 0xffff0000u);
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int oy = oy0 + wave, ox = ox0 + r;
  if (oy >= ho) return;                                             // no barrier below
  // the lane's seven fragments: k = 16 s + 8 hh + 0 .. 7 = dwords 8 s + 4 hh + 0 .. 3 of the window, dword d = 9 ky + j at patch
  // (2 wave + ky, 2 r) + j; dwords 54 and 55 are the zero taps
  const int dw0 = 2 * wave * kPitch + 3 * r;
  half8 xh[kSteps], xl[kSplit ? kSteps : 1];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) {
    unsigned vh[4], vl[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int d0 = 8 * s + e, d1 = d0 + 4;                        // hh = 0 / 1
      const int off0 = d0 / 9 * kPitch + d0 % 9, off1 = d1 < kTapDwords ? d1 / 9 * kPitch + d1 % 9 : 0;
      const int off = dw0 + (hh ? off1 : off0);
      const bool tap = d1 < kTapDwords || !hh;
      vh[e] = tap ? s_hi[off] : 0u;
      vl[e] = kSplit && tap ? s_lo[off] : 0u;
    }
    xh[s] = __builtin_bit_cast(half8, make_uint4(vh[0], vh[1], vh[2], vh[3]));
    if (kSplit) xl[s] = __builtin_bit_cast(half8, make_uint4(vl[0], vl[1], vl[2], vl[3]));
  }
  for (int g = 0; g < groups; ++g) {
    floatx16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      if (kSplit) {
        const half8 wh = *reinterpret_cast<const half8*>(wpk + ((((size_t)g * kSteps + s) * 2 + 0) * 64 + lane) * 8);
        const half8 wl = *reinterpret_cast<const half8*>(wpk + ((((size_t)g * kSteps + s) * 2 + 1) * 64 + lane) * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl[s], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh[s], acc, 0, 0, 0);
      } else {
        const half8 wf = *reinterpret_cast<const half8*>(wpk + (((size_t)g * kSteps + s) * 64 + lane) * 8);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf, xh[s], acc, 0, 0, 0);
      }
    }
    // acc[4 g4 + i] = channel 32 g + 8 g4 + 4 hh + i of pixel r
    if (kSplit) {
      // pair format: lanes l and l + 32 hold the two halves of an 8-channel group; two v_permlane32_swap make the group's 16-byte
      // hi chunk (lane l) and lo chunk (lane l + 32), as in the 3x3 stem. Every lane runs the swaps; the stores are guarded.
      float* o = (float*)out + (((size_t)n * ho + oy) * wo + (ox < wo ? ox : 0)) * c0 + g * 32;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int cl = g * 32 + 8 * g4 + 4 * hh;
        half4 hv, lv;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // the clamp only keeps an absurd checkpoint from producing inf - inf (bias is padded to whole 32-channel groups)
          const float v = __builtin_amdgcn_fmed3f(silu_f(fmaf(acc[4 * g4 + i], acc_scale, bias[cl + i])), -65504.f, 65504.f);
          const _Float16 hi = (_Float16)v;
          hv[i] = hi;
          lv[i] = (_Float16)(v - (float)hi);
        }
        const uint2 hu = *reinterpret_cast<const uint2*>(&hv), lu = *reinterpret_cast<const uint2*>(&lv);
        const auto sx = __builtin_amdgcn_permlane32_swap(hu.x, lu.x, false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(hu.y, lu.y, false, false);
        if (ox < wo && g * 32 + 8 * g4 < c0)                          // c0 is a multiple of 8: whole groups
          *reinterpret_cast<uint4*>(o + 8 * g4 + 4 * hh) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
      }
    } else if (ox < wo) {
      _Float16* o = (_Float16*)out + (((size_t)n * ho + oy) * wo + ox) * c0 + g * 32;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int cl = 8 * g4 + 4 * hh;
        if (g * 32 + cl < c0) {
          half4 v;
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = (_Float16)silu_f(acc[4 * g4 + i] + bias[g * 32 + cl + i]);
          *reinterpret_cast<half4*>(o + cl) = v;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void stem6_mfma_kernel(const uchar4* __restrict__ img, int h, int w, const _Float16* __restrict__ wpk,
                                                         const float* __restrict__ bias, _Float16* __restrict__ out, int ho, int wo, int c0,
                                                         int groups) {
  stem6_mma<false>(img, h, w, wpk, bias, 1.f, out, ho, wo, c0, groups);
}

__global__ __launch_bounds__(256) void stem6_split_kernel(const uchar4* __restrict__ img, int h, int w, const _Float16* __restrict__ wpk,
                                                          const float* __restrict__ bias, float acc_scale, float* __restrict__ out, int ho,
                                                          int wo, int c0, int groups) {
  stem6_mma<true>(img, h, w, wpk, bias, acc_scale, out, ho, wo, c0, groups);
}

// Exact fp32: one thread = one output pixel of an 8 x 32 tile, all C0 channels, on the same staged patch (as fp32 values); the weights
// are read through wave-uniform addresses, i.e. the scalar cache, as in stem_kernel.
template <int C0>
__global__ __launch_bounds__(256) void stem6_kernel(const uchar4* __restrict__ img, int h, int w, const float* __restrict__ w108,
                                                    const float* __restrict__ bias, float* __restrict__ out, int ho, int wo) {
  constexpr int kRows = kStem6RowsF32, kPatchRows = 2 * kRows + 4;
  __shared__ float s_px[kPatchRows * kPatchCols * 3];
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = (float)threadIdx.x / 255.f;
  __syncthreads();
  const int ox0 = blockIdx.x * kCols, oy0 = blockIdx.y * kRows, n = blockIdx.z;
  const uchar4* base = img + (size_t)n * h * w;
  for (int i = threadIdx.x; i < kPatchRows * kPatchCols; i += blockDim.x) {
    const int py = i / kPatchCols, px = i - py * kPatchCols;
    const unsigned a = patch_word(base, h, w, oy0, ox0, py, px);
    s_px[3 * i] = s_lut[a & 255u]; s_px[3 * i + 1] = s_lut[(a >> 8) & 255u]; s_px[3 * i + 2] = s_lut[(a >> 16) & 255u];
  }
  __syncthreads();
  const int ty = threadIdx.x >> 5, tx = threadIdx.x & 31;
  const int oy = oy0 + ty, ox = ox0 + tx;
  if (oy >= ho || ox >= wo) return;
  float acc[C0];
#pragma unroll
  for (int c = 0; c < C0; ++c) acc[c] = bias[c];
#pragma unroll 1
  for (int ky = 0; ky < 6; ++ky) {
    const float* row = s_px + ((2 * ty + ky) * kPatchCols + 2 * tx) * 3;      // the window row's 18 values
    const float* wt = w108 + ky * 18 * C0;
#pragma unroll
    for (int j = 0; j < 18; ++j) {
      const float v = row[j];
#pragma unroll
      for (int c = 0; c < C0; ++c) acc[c] = fmaf(v, wt[j * C0 + c], acc[c]);
    }
  }
  float* o = out + (((size_t)n * ho + oy) * wo + ox) * C0;
#pragma unroll
  for (int c = 0; c < C0; c += 4) *reinterpret_cast<float4*>(o + c) = make_float4(silu_f(acc[c]), silu_f(acc[c + 1]), silu_f(acc[c + 2]), silu_f(acc[c + 3]));
}

}  // namespace

void launch_stem6(int dtype, const void* img, int n, int h, int w, const float* w108, const float* bias, const void* wpk, int c0, void* out,
                  int ho, int wo, hipStream_t s, float acc_scale) {
  GTX_CHECK(h >= 2 && w >= 2 && ho == stem6_out(h) && wo == stem6_out(w) && n >= 1, "stem6: a %d x %d image does not give a %d x %d map", w, h, wo, ho);
  GTX_CHECK(c0 >= 16 && c0 <= 96 && c0 % 16 == 0, "stem6: unsupported channel count %d", c0);
  if (dtype == DT_F32S || dtype == DT_F16) {
    GTX_CHECK(wpk != nullptr, "stem6: packed weights missing");
    const dim3 grid(cdiv(wo, kCols), cdiv(ho, kStem6Rows), n);
    if (dtype == DT_F32S)
      hipLaunchKernelGGL(stem6_split_kernel, grid, dim3(256), 0, s, (const uchar4*)img, h, w, (const _Float16*)wpk, bias, acc_scale, (float*)out, ho, wo,
                         c0, cdiv(c0, 32));
    else
      hipLaunchKernelGGL(stem6_mfma_kernel, grid, dim3(256), 0, s, (const uchar4*)img, h, w, (const _Float16*)wpk, bias, (_Float16*)out, ho, wo, c0,
                         cdiv(c0, 32));
    GTX_HIP(hipGetLastError());
    return;
  }
  GTX_CHECK(dtype == DT_F32, "stem6: dtype %d", dtype);
  const dim3 grid(cdiv(wo, kCols), cdiv(ho, kStem6RowsF32), n);
#define GTX_STEM6(C)                                                                                                                     \
  if (c0 == C) {                                                                                                                         \
    hipLaunchKernelGGL((stem6_kernel<C>), grid, dim3(256), 0, s, (const uchar4*)img, h, w, w108, bias, (float*)out, ho, wo);             \
    GTX_HIP(hipGetLastError());                                                                                                          \
    return;                                                                                                                              \
  }
  GTX_STEM6(16) GTX_STEM6(32) GTX_STEM6(48) GTX_STEM6(64) GTX_STEM6(80) GTX_STEM6(96)
#undef GTX_STEM6
}

namespace {
// value of packed element (group g, step s, lane, e): row 16 s + 8 hh + e of w108 at channel 32 g + r, zero for the padding
inline float stem6_w(const float* w108, int c0, int g, int s, int lane, int e) {
  const int k = 16 * s + 8 * (lane >> 5) + e, co = g * 32 + (lane & 31);
  return k < 108 && co < c0 ? w108[(size_t)k * c0 + co] : 0.f;
}
inline uint16_t half_bits(_Float16 v) {
  uint16_t b;
  memcpy(&b, &v, 2);
  return b;
}
}  // namespace

std::vector<uint16_t> pack_stem6_weights_f16(const float* w108, int c0) {
  const int groups = cdiv(c0, 32);
  std::vector<uint16_t> out((size_t)groups * kSteps * 64 * 8, 0);
  for (int g = 0; g < groups; ++g)
    for (int s = 0; s < kSteps; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) out[(((size_t)g * kSteps + s) * 64 + lane) * 8 + e] = half_bits((_Float16)stem6_w(w108, c0, g, s, lane, e));
  return out;
}

std::vector<uint16_t> pack_stem6_weights_split(const float* w108, int c0, float* acc_scale) {
  const int groups = cdiv(c0, 32);
  float wmax = 0.f;
  for (int i = 0; i < 108 * c0; ++i) wmax = std::max(wmax, std::fabs(w108[i]));
  int shift = 0;
  if (wmax > 0.f && std::isfinite(wmax)) {
    int e;
    std::frexp(wmax, &e);
    shift = std::max(-100, std::min(100, 14 - e));
  }
  const float up = std::ldexp(1.f, shift);
  *acc_scale = std::ldexp(1.f, -shift);
  std::vector<uint16_t> out((size_t)groups * kSteps * 2 * 64 * 8, 0);
  for (int g = 0; g < groups; ++g)
    for (int s = 0; s < kSteps; ++s)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 8; ++e) {
          const float v = stem6_w(w108, c0, g, s, lane, e) * up;
          const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
          out[((((size_t)g * kSteps + s) * 2 + 0) * 64 + lane) * 8 + e] = half_bits(hi);
          out[((((size_t)g * kSteps + s) * 2 + 1) * 64 + lane) * 8 + e] = half_bits(lo);
        }
  return out;
}

}  // namespace gtx
