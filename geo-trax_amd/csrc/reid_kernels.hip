// Crop + resample and pooled-embedding kernels of the ReID network (reid_kernels.hpp). gfx950 only.
//
// Crop + resample: PIL's two-pass fixed-point bilinear resample for 8-bit images (Resample.c: ImagingResampleHorizontal_8bpc, then
// ImagingResampleVertical_8bpc; 22 fraction bits, rounding bias 1 << 21, clip8 after each pass, a u8 intermediate). The
// coefficients and bounds arrive precomputed (host, double, reid.cpp), so the kernel is integer arithmetic only: its bytes are
// PIL's bytes whatever the compiler contracts.
//
// Work layout: one workgroup per (crop, band of kBand output rows), all S columns. The horizontal pass of the source rows the band
// reads goes through LDS in chunks of kChunk rows; every thread keeps the vertical sums of its kPix output pixels in registers
// and adds each chunk's rows that fall in their windows (integer sums: the chunking does not change a bit). A crop's short side
// runs from ~10 px to the frame's height (downscale factor short / S: up to 2160 / 224 = 9.6, support +-9.6 source rows), so an
// 8-row band reads from 2 source rows up to 8 * 9.6 + 2 * 9.6 = ~96 (~45 for a 1000-px short side); chunking keeps the LDS at a
// fixed 32 KB (S <= 256; 30 KB in chunks of 24 rows for S up to 320) whatever the band reads. Neighbouring bands recompute the few
// source rows their windows share.
#include "reid_kernels.hpp"

namespace gtx {

namespace {
constexpr int kBand = 8;                // output rows per workgroup
constexpr int kThreads = 256;
constexpr int kPrec = 22;               // PIL PRECISION_BITS (32 - 8 - 2)

__device__ __forceinline__ uint32_t clip8(int v) {
  if (v >= (1 << kPrec << 8)) return 255u;
  if (v <= 0) return 0u;
  return (uint32_t)(v >> kPrec);
}
}  // namespace

// kMaxS: the largest S of this instance; kChunk: intermediate rows per LDS chunk
template <int kMaxS, int kChunk>
__global__ __launch_bounds__(kThreads) void reid_crop_kernel(const uint8_t* __restrict__ frames, int H, int W,
                                                             const ReidCrop* __restrict__ crops, const int* __restrict__ pool, int S,
                                                             uchar4* __restrict__ out) {
  constexpr int kPix = kBand * kMaxS / kThreads;   // output pixels per thread (8 / 10)
  __shared__ uint32_t tile[kChunk * kMaxS];
  const ReidCrop c = crops[blockIdx.y];
  const int r0 = blockIdx.x * kBand;
  const int rows = min(kBand, S - r0);
  const int tid = threadIdx.x;
  const int* __restrict__ bh = pool + c.bh;
  const int* __restrict__ bv = pool + c.bv;
  const int ylo = bv[2 * r0], yhi = bv[2 * (r0 + rows - 1)] + bv[2 * (r0 + rows - 1) + 1];   // windows move monotonically down
  const uint8_t* __restrict__ src = frames + ((size_t)c.frame * H + c.y0) * (size_t)W * 3 + (size_t)c.x0 * 3;
  int acc[kPix][3];
#pragma unroll
  for (int i = 0; i < kPix; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 1 << (kPrec - 1);
  for (int y = ylo; y < yhi; y += kChunk) {
    const int nr = min(kChunk, yhi - y);
    // horizontal pass of source rows [y, y + nr) at the S output columns
    for (int q = tid; q < nr * S; q += kThreads) {
      const int row = q / S, col = q - row * S;
      const int xmin = bh[2 * col], xn = bh[2 * col + 1];
      const int* __restrict__ k = pool + c.hoff + col * c.kh;
      const uint8_t* __restrict__ p = src + (size_t)(y + row) * W * 3 + (size_t)xmin * 3;
      int s0 = 1 << (kPrec - 1), s1 = s0, s2 = s0;
      for (int x = 0; x < xn; ++x) {
        const int kx = k[x];
        s0 += (int)p[3 * x] * kx;
        s1 += (int)p[3 * x + 1] * kx;
        s2 += (int)p[3 * x + 2] * kx;
      }
      tile[q] = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16);
    }
    __syncthreads();
    // vertical pass: the chunk's rows that fall in each output row's window
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
      const int p = tid + i * kThreads;
      if (p < rows * S) {
        const int r = p / S, col = p - r * S;
        const int ymin = bv[2 * (r0 + r)], yn = bv[2 * (r0 + r) + 1];
        const int* __restrict__ k = pool + c.voff + (r0 + r) * c.kv;
        const int lo = max(ymin, y), hi = min(ymin + yn, y + nr);
        for (int yy = lo; yy < hi; ++yy) {
          const uint32_t v = tile[(yy - y) * S + col];
          const int ky = k[yy - ymin];
          acc[i][0] += (int)(v & 255u) * ky;
          acc[i][1] += (int)((v >> 8) & 255u) * ky;
          acc[i][2] += (int)((v >> 16) & 255u) * ky;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kPix; ++i) {
    const int p = tid + i * kThreads;
    if (p < rows * S) {
      const int r = p / S, col = p - r * S;
      out[((size_t)blockIdx.y * S + r0 + r) * S + col] =
          make_uchar4((unsigned char)clip8(acc[i][0]), (unsigned char)clip8(acc[i][1]), (unsigned char)clip8(acc[i][2]), 0);
    }
  }
}

void launch_reid_crop(const uint8_t* frames, int h, int w, const ReidCrop* crops, const int* pool, int n, int S, void* out, hipStream_t s) {
  GTX_CHECK(S >= 32 && S <= 320, "reid crop: size %d outside [32, %d]", S, 320);
  if (n == 0) return;
  const dim3 grid(cdiv(S, kBand), n), block(kThreads);
  if (S <= 256) hipLaunchKernelGGL((reid_crop_kernel<256, 32>), grid, block, 0, s, frames, h, w, crops, pool, S, (uchar4*)out);
  else hipLaunchKernelGGL((reid_crop_kernel<320, 24>), grid, block, 0, s, frames, h, w, crops, pool, S, (uchar4*)out);
  GTX_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void reid_pool_kernel(const uint8_t* __restrict__ in, int fmt, int n, int hw, int cstride, int coff, int c,
                                                        float* __restrict__ out) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (ch >= c) return;
  const size_t base = (size_t)b * hw * cstride;
  float sum = 0.f;
  for (int p = 0; p < hw; ++p) {
    const size_t e = base + (size_t)p * cstride + coff + ch;
    float v;
    if (fmt == 1) {                                           // pair format: group of 8 at byte 4 * (e & ~7), hi then lo halves
      const uint8_t* g = in + (e & ~(size_t)7) * 4;
      v = (float)*reinterpret_cast<const _Float16*>(g + 2 * (e & 7)) + (float)*reinterpret_cast<const _Float16*>(g + 16 + 2 * (e & 7));
    } else {
      v = reinterpret_cast<const float*>(in)[e];
    }
    sum += v;
  }
  out[(size_t)b * c + ch] = sum / (float)hw;
}

void launch_reid_pool(const void* in, int fmt, int n, int hw, int cstride, int coff, int c, float* out, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(reid_pool_kernel, dim3(cdiv(c, 256), n), dim3(256), 0, s, (const uint8_t*)in, fmt, n, hw, cstride, coff, c, out);
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
