// Baseline JPEG, the pixel half: what cv2.VideoCapture.read() (geotrax/extract.py:146) does after entropy decoding, for
// Motion-JPEG clips and folders of .jpg frames. The host (csrc/jpeg_parse.cpp) delivers a packed record of quantised
// coefficients; two launches per frame turn it into the packed BGR frame gtx_yuv420_to_bgr_dev would have produced:
//
//   jpeg_idct_kernel     record -> dequantise -> 8x8 inverse DCT -> +128, clamp -> u8 planes (Y, Cb, Cr at block-grid size)
//   jpeg_colour_kernel   planes -> chroma upsampling -> YCbCr -> BGR u8 [h][w][3]
//
// The arithmetic is libjpeg's default decode, integer throughout (what Pillow and cv2.imread yield): the slow-integer IDCT of
// jidctint.c (13-bit constants, a column pass that keeps 2 extra bits, a row pass), the "fancy" triangle upsampler of
// jdsample.c for h2v1 / h2v2 (plain replication when the chroma plane is at most 2 samples wide, as there) and the 16-bit
// fixed-point tables of jdcolor.c. geotrax_amd/jpeg.py restates it in numpy, line for line.
//
// Both kernels are HBM-bound (a 4K 4:2:0 frame: ~5 MB of record in, 12 MB of planes out; 12 MB in, 25 MB out). One lane owns
// one 8x8 block: its coefficient run is contiguous in the stream, its eight 8-byte row stores sit beside its neighbour lanes'.
// The workspace lives in LDS, 65 words per lane so that lane l's word j falls in bank (l + j) % 64.
#include <hip/hip_runtime.h>

#include "detector.hpp"
#include "jpeg.hpp"

namespace gtx {
namespace {
using jpeg::RecordHeader;

__constant__ uint8_t kNaturalDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jidctint.c: CONST_BITS 13, PASS1_BITS 2
constexpr int kC0298 = 2446, kC0390 = 3196, kC0541 = 4433, kC0765 = 6270, kC0899 = 7373, kC1175 = 9633, kC1501 = 12299,
              kC1847 = 15137, kC1961 = 16069, kC2053 = 16819, kC2562 = 20995, kC3072 = 25172;

// One 1-D pass over in[0..7] (stride s): out[k] = (even/odd sums + round) >> shift, as jidctint.c writes them. The sums are formed
// in unsigned 32-bit arithmetic, which wraps: clean data stays far inside the range (libjpeg-turbo's SIMD form uses 32-bit lanes
// too), damaged data that the parser lets through wraps here exactly as numpy's int32 does in the host twin.
__device__ __forceinline__ void idct8(const int* in, int s, uint32_t round, int shift, int out[8]) {
  using u = uint32_t;
  u z2 = (u)in[2 * s], z3 = (u)in[6 * s];
  u z1 = (z2 + z3) * (u)kC0541;
  const u tmp2 = z1 - z3 * (u)kC1847, tmp3 = z1 + z2 * (u)kC0765;
  z2 = (u)in[0], z3 = (u)in[4 * s];
  const u tmp0 = (z2 + z3) << 13, tmp1 = (z2 - z3) << 13;       // << CONST_BITS
  const u tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  u t0 = (u)in[7 * s], t1 = (u)in[5 * s], t2 = (u)in[3 * s], t3 = (u)in[1 * s];
  z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2;
  u z4 = t1 + t3;
  const u z5 = (z3 + z4) * (u)kC1175;
  t0 *= (u)kC0298, t1 *= (u)kC2053, t2 *= (u)kC3072, t3 *= (u)kC1501;
  z1 = 0u - z1 * (u)kC0899, z2 = 0u - z2 * (u)kC2562, z3 = 0u - z3 * (u)kC1961, z4 = 0u - z4 * (u)kC0390;
  z3 += z5, z4 += z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  out[0] = (int)(tmp10 + t3 + round) >> shift;                  // arithmetic shift of the wrapped sum
  out[7] = (int)(tmp10 - t3 + round) >> shift;
  out[1] = (int)(tmp11 + t2 + round) >> shift;
  out[6] = (int)(tmp11 - t2 + round) >> shift;
  out[2] = (int)(tmp12 + t1 + round) >> shift;
  out[5] = (int)(tmp12 - t1 + round) >> shift;
  out[3] = (int)(tmp13 + t0 + round) >> shift;
  out[4] = (int)(tmp13 - t0 + round) >> shift;
}

__device__ __forceinline__ uint32_t sat8(int v) { return (uint32_t)min(max(v, 0), 255); }

constexpr int kIdctLanes = 64, kWsStride = 65;

__global__ __launch_bounds__(kIdctLanes) void jpeg_idct_kernel(const uint8_t* __restrict__ rec, RecordHeader hd, uint8_t* __restrict__ planes) {
  __shared__ int ws_all[kIdctLanes * kWsStride];
  const uint32_t b = blockIdx.x * kIdctLanes + threadIdx.x;
  if (b >= hd.n_blocks) return;                                  // no barrier below: a lane works on its own 65 words
  int* ws = ws_all + threadIdx.x * kWsStride;
  // which block: MCU, position inside it -> component and block coordinates
  const uint32_t luma = hd.hs * hd.vs, bpm = hd.ncomp == 1 ? 1u : luma + 2u;
  const uint32_t mcu = b / bpm, k = b - mcu * bpm, mx = mcu % hd.mcus_x, my = mcu / hd.mcus_x;
  uint32_t c, bx, by;
  if (hd.ncomp == 1 || k < luma) {
    c = 0, bx = mx * hd.hs + k % hd.hs, by = my * hd.vs + k / hd.hs;
  } else {
    c = 1 + (k - luma), bx = mx, by = my;
  }
  if (c >= hd.ncomp || bx >= hd.bw[c] || by >= hd.bh[c]) return;  // cannot happen for a checked record
  size_t plane_off = 0;
  for (uint32_t i = 0; i < c; ++i) plane_off += 64 * (size_t)hd.bw[i] * hd.bh[i];
  const uint16_t* quant = reinterpret_cast<const uint16_t*>(rec + jpeg::kQuantOffset) + 64 * c;
  const uint32_t* offsets = reinterpret_cast<const uint32_t*>(rec + jpeg::kOffsetsOffset);
  const int16_t* coefs = reinterpret_cast<const int16_t*>(rec + jpeg::kOffsetsOffset + 4 * ((size_t)hd.n_blocks + 1));
  // the run of this block, checked against the record's own sizes before anything is indexed by it
  const uint32_t first = offsets[b], last = offsets[b + 1];
  uint32_t len = last > first ? last - first : 0u;
  len = min(len, 64u);
  if (first > hd.n_coef || len > hd.n_coef - first) len = 0;

#pragma unroll
  for (int j = 0; j < 64; ++j) ws[j] = 0;
  for (uint32_t z = 0; z < len; ++z) {
    const int nat = kNaturalDev[z];
    ws[nat] = (int)coefs[first + z] * (int)quant[nat];            // DEQUANTIZE: at most 2^15 * 2^8, no overflow
  }
  // pass 1: columns, results scaled up by 2^PASS1_BITS, in place (a column is read whole before it is written)
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    int o[8];
    idct8(ws + col, 8, 1u << 10, 11, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[8 * r + col] = o[r];
  }
  // pass 2: rows; descale by 2^(CONST_BITS + PASS1_BITS + 3), level shift, clamp, one 8-byte store per row
  const size_t stride = 8 * (size_t)hd.bw[c];
  uint8_t* dst = planes + plane_off + (size_t)by * 8 * stride + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    int o[8];
    idct8(ws + 8 * r, 1, 1u << 17, 18, o);
    uint2 v;
    v.x = sat8(o[0] + 128) | sat8(o[1] + 128) << 8 | sat8(o[2] + 128) << 16 | sat8(o[3] + 128) << 24;
    v.y = sat8(o[4] + 128) | sat8(o[5] + 128) << 8 | sat8(o[6] + 128) << 16 | sat8(o[7] + 128) << 24;
    *reinterpret_cast<uint2*>(dst + (size_t)r * stride) = v;      // 8-byte aligned: plane sizes and offsets are multiples of 64 / 8
  }
}

// jdcolor.c build_ycc_rgb_table: FIX(1.40200), FIX(1.77200), FIX(0.71414), FIX(0.34414) at 16 bits
constexpr int kCrR = 91881, kCbB = 116130, kCrG = 46802, kCbG = 22554, kHalf = 1 << 15;

// Upsampled chroma at output columns x0 .. x0+3 of output row y (x0 a multiple of 4). cw, ch: the real chroma plane
// (ceil(w / 2), ceil(h / 2) where subsampled), whose edges are the upsampler's edges; stride: the padded plane's row pitch.
__device__ __forceinline__ void chroma4(const uint8_t* __restrict__ pl, int stride, int cw, int ch, int hs, int vs, int x0, int y, int w, int out[4]) {
  if (hs == 1) {                                                 // 4:4:4
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = pl[(size_t)y * stride + min(x0 + k, w - 1)];
    return;
  }
  const int i0 = x0 >> 1;                                        // chroma columns i0, i0 + 1 (and their neighbours i0 - 1, i0 + 2)
  if (cw <= 2) {                                                 // jdsample.c: fancy upsampling needs more than 2 columns; replicate
    const uint8_t* row = pl + (size_t)(vs == 2 ? (y >> 1) : y) * stride;
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = row[min(i0 + (k >> 1), cw - 1)];
    return;
  }
  if (vs == 1) {                                                 // h2v1_fancy_upsample
    const uint8_t* row = pl + (size_t)y * stride;
    int s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = row[min(max(i0 - 1 + k, 0), cw - 1)];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = i0 + k, v3 = 3 * s[k + 1];
      out[2 * k] = (i == 0 || i >= cw) ? s[k + 1] : (v3 + s[k] + 1) >> 2;
      out[2 * k + 1] = (i >= cw - 1) ? s[k + 1] : (v3 + s[k + 2] + 2) >> 2;
    }
    return;
  }
  // h2v2_fancy_upsample: the nearer row weighs 3, the farther 1; past the plane's first / last real row the row itself
  const int r = y >> 1, rn = (y & 1) ? min(r + 1, ch - 1) : max(r - 1, 0);
  const uint8_t *near = pl + (size_t)r * stride, *far = pl + (size_t)rn * stride;
  int s[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = min(max(i0 - 1 + k, 0), cw - 1);
    s[k] = 3 * near[i] + far[i];
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int i = i0 + k, t = s[k + 1];
    out[2 * k] = (i == 0 || i >= cw) ? (t * 4 + 8) >> 4 : (t * 3 + s[k] + 8) >> 4;
    out[2 * k + 1] = (i >= cw - 1) ? (t * 4 + 7) >> 4 : (t * 3 + s[k + 2] + 7) >> 4;
  }
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, RecordHeader hd, uint8_t* __restrict__ bgr) {
  const int w = (int)hd.width, h = (int)hd.height;
  const int x0 = (int)(blockIdx.x * blockDim.x + threadIdx.x) * 4, y = (int)blockIdx.y;
  if (x0 >= w || y >= h) return;
  const int ys = 8 * (int)hd.bw[0];
  const uint8_t* yrow = planes + (size_t)y * ys;
  const bool full = x0 + 4 <= w && (w & 3) == 0 && (reinterpret_cast<uintptr_t>(bgr) & 3) == 0;   // 4-byte stores need all three
  int yy[4];
  if (x0 + 4 <= ys) {                                            // the padded luma row is a multiple of 8 wide: aligned 4-byte load
    const uint32_t q = *reinterpret_cast<const uint32_t*>(yrow + x0);
    yy[0] = q & 255, yy[1] = (q >> 8) & 255, yy[2] = (q >> 16) & 255, yy[3] = q >> 24;
  } else {
    for (int k = 0; k < 4; ++k) yy[k] = yrow[min(x0 + k, ys - 1)];
  }
  uint32_t out[3] = {0, 0, 0};
  if (hd.ncomp == 1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t v = (uint32_t)yy[k];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int o = 3 * k + ch;
        out[o >> 2] |= v << (8 * (o & 3));
      }
    }
  } else {
    const int hs = (int)hd.hs, vs = (int)hd.vs, cs = 8 * (int)hd.bw[1];
    const int cw = hs == 2 ? (w + 1) >> 1 : w, chh = vs == 2 ? (h + 1) >> 1 : h;
    const size_t ysz = 64 * (size_t)hd.bw[0] * hd.bh[0], csz = 64 * (size_t)hd.bw[1] * hd.bh[1];
    int cb[4], cr[4];
    chroma4(planes + ysz, cs, cw, chh, hs, vs, x0, y, w, cb);
    chroma4(planes + ysz + csz, cs, cw, chh, hs, vs, x0, y, w, cr);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int u = cb[k] - 128, v = cr[k] - 128;
      const uint32_t r = sat8(yy[k] + ((kCrR * v + kHalf) >> 16));
      const uint32_t g = sat8(yy[k] + ((-kCbG * u + kHalf - kCrG * v) >> 16));
      const uint32_t bb = sat8(yy[k] + ((kCbB * u + kHalf) >> 16));
      const int o = 3 * k;
      out[o >> 2] |= bb << (8 * (o & 3));
      out[(o + 1) >> 2] |= g << (8 * ((o + 1) & 3));
      out[(o + 2) >> 2] |= r << (8 * ((o + 2) & 3));
    }
  }
  uint8_t* d = bgr + ((size_t)y * w + x0) * 3;
  if (full) {
    uint32_t* d4 = reinterpret_cast<uint32_t*>(d);                // (y * w + x0) * 3 is a multiple of 4 when w and x0 are
    d4[0] = out[0], d4[1] = out[1], d4[2] = out[2];
  } else {
    for (int k = 0; k < 12 && x0 + k / 3 < w; ++k) d[k] = (uint8_t)(out[k >> 2] >> (8 * (k & 3)));
  }
}
}  // namespace

void jpeg_decode_launch(gtx_ctx* ctx, const void* d_record, const jpeg::RecordHeader& hd, void* d_planes, void* bgr, hipEvent_t between) {
  GTX_HIP(hipSetDevice(ctx->device));
  GTX_CHECK(hd.n_blocks > 0 && hd.width > 0 && hd.height > 0, "jpeg_decode: empty record");
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3(cdiv((int)hd.n_blocks, kIdctLanes)), dim3(kIdctLanes), 0, ctx->stream,
                     static_cast<const uint8_t*>(d_record), hd, static_cast<uint8_t*>(d_planes));
  GTX_HIP(hipGetLastError());
  if (between) GTX_HIP(hipEventRecord(between, ctx->stream));
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3(cdiv(cdiv((int)hd.width, 4), 256), hd.height), dim3(256), 0, ctx->stream,
                     static_cast<const uint8_t*>(d_planes), hd, static_cast<uint8_t*>(bgr));
  GTX_HIP(hipGetLastError());
}
}  // namespace gtx
