// Baseline JPEG, the pixel half of writing: what cv2.VideoWriter.write() (geotrax/visualize.py:298) does before entropy coding,
// for Motion-JPEG output. A packed BGR frame in HBM becomes the packed record of jpeg_parse.hpp (quantised coefficients in
// zigzag runs); the host (csrc/jpeg_emit.cpp) Huffman-codes it. csrc/jpeg.hip run backwards, six launches per frame:
//
//   jpeg_planes_kernel    BGR -> YCbCr, edges replicated, chroma 2x2-averaged -> u8 planes (Y, Cb, Cr at block-grid size)
//   jpeg_fdct_kernel      planes -> -128 -> 8x8 forward DCT -> quantise -> zigzag -> dense runs [n_blocks][64] + block lengths
//   jpegscan::scan_*      exclusive prefix sum of the lengths -> the record's offset[] (tile sums, scan of the sums, apply;
//                         csrc/jpeg_scan.hpp, shared with the entropy coder)
//   jpeg_compact_kernel   dense runs -> coef[] at the offsets
//
// On the GPU entropy route (use_gpu_entropy) the last four are replaced by csrc/jpeg_huff.hip's launches: dense runs -> picture.
//
// The arithmetic is libjpeg's default encode, integer throughout (what Pillow and cv2.imwrite produce): the 16-bit fixed-point
// tables of jccolor.c, h2v2_downsample of jcsample.c with its alternating bias, the slow-integer DCT of jfdctint.c (13-bit
// constants, a row pass that keeps 2 extra bits, a column pass), the divide of jcdctmgr.c, and jccoefct.c's dummy blocks where
// an MCU reaches past a component's own block grid. geotrax_amd/jpeg.py restates it in numpy, line for line.
#include <hip/hip_runtime.h>

#include "detector.hpp"
#include "jpeg_enc.hpp"
#include "jpeg_scan.hpp"

namespace gtx {
namespace {
using jpeg::RecordHeader;

__constant__ uint8_t kNaturalEnc[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jccolor.c rgb_ycc_start: FIX(0.29900), FIX(0.58700), FIX(0.11400), FIX(0.16874), FIX(0.33126), FIX(0.50000), FIX(0.41869),
// FIX(0.08131) at 16 bits; Cb and Cr add CBCR_OFFSET + ONE_HALF - 1
constexpr int kYR = 19595, kYG = 38470, kYB = 7471, kCbR = 11059, kCbG = 21709, kHalfC = 32768, kCrG = 27439, kCrB = 5329;
constexpr int kOneHalf = 1 << 15, kCOff = (128 << 16) + kOneHalf - 1;

struct Ycc {
  int y, cb, cr;
};
// the pixel at (x, y) clamped into the frame: the edge replication of expand_right_edge / expand_bottom_edge
__device__ __forceinline__ Ycc ycc_at(const uint8_t* __restrict__ bgr, int w, int h, int x, int y) {
  const uint8_t* p = bgr + ((size_t)min(y, h - 1) * w + min(x, w - 1)) * 3;
  const int b = p[0], g = p[1], r = p[2];
  return {(kYR * r + kYG * g + kYB * b + kOneHalf) >> 16, (-kCbR * r - kCbG * g + kHalfC * b + kCOff) >> 16,
          (kHalfC * r - kCrG * g - kCrB * b + kCOff) >> 16};
}

// One lane: one chroma sample and the hs x vs luma samples under it (4:2:0: 2x2; 4:4:4: the pixel itself).
__global__ __launch_bounds__(256) void jpeg_planes_kernel(const uint8_t* __restrict__ bgr, RecordHeader hd, uint8_t* __restrict__ planes) {
  const int w = (int)hd.width, h = (int)hd.height, hs = (int)hd.hs, vs = (int)hd.vs;
  const int cw = 8 * (int)hd.bw[1], chh = 8 * (int)hd.bh[1], yw = 8 * (int)hd.bw[0], yh = 8 * (int)hd.bh[0];
  const int cx = (int)(blockIdx.x * blockDim.x + threadIdx.x), cy = (int)blockIdx.y;
  if (cx >= cw || cy >= chh || cx * hs + hs > yw || cy * vs + vs > yh) return;
  const size_t ysz = (size_t)yw * yh, csz = (size_t)cw * chh;
  uint8_t *py = planes, *pcb = planes + ysz, *pcr = planes + ysz + csz;
  if (hs == 1) {                                                 // 4:4:4: a full-size copy
    const Ycc v = ycc_at(bgr, w, h, cx, cy);
    py[(size_t)cy * yw + cx] = (uint8_t)v.y;
    pcb[(size_t)cy * cw + cx] = (uint8_t)v.cb;
    pcr[(size_t)cy * cw + cx] = (uint8_t)v.cr;
    return;
  }
  // luma: the 2x2 samples at their own (clamped) positions
  int scb = 0, scr = 0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const Ycc a = ycc_at(bgr, w, h, 2 * cx, 2 * cy + dy), b = ycc_at(bgr, w, h, 2 * cx + 1, 2 * cy + dy);
    *reinterpret_cast<uchar2*>(py + (size_t)(2 * cy + dy) * yw + 2 * cx) = make_uchar2((uint8_t)a.y, (uint8_t)b.y);   // yw, 2 * cx even
    scb += a.cb + b.cb, scr += a.cr + b.cr;
  }
  // chroma: h2v2_downsample over the input rows padded to an even count; chroma rows past ceil(h / 2) repeat the last
  // downsampled row (jcprepct.c pads its output), which is another value than the box over repeated input rows when h is even
  const int rows = (h + 1) >> 1;
  if (cy >= rows) {
    const int ry = rows - 1;
    scb = 0, scr = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      const Ycc a = ycc_at(bgr, w, h, 2 * cx, 2 * ry + dy), b = ycc_at(bgr, w, h, 2 * cx + 1, 2 * ry + dy);
      scb += a.cb + b.cb, scr += a.cr + b.cr;
    }
  }
  const int bias = 1 + (cx & 1);                                  // 1, 2, 1, 2, ... along a row
  pcb[(size_t)cy * cw + cx] = (uint8_t)((scb + bias) >> 2);
  pcr[(size_t)cy * cw + cx] = (uint8_t)((scr + bias) >> 2);
}

// jfdctint.c: CONST_BITS 13, PASS1_BITS 2
constexpr int kF0298 = 2446, kF0390 = 3196, kF0541 = 4433, kF0765 = 6270, kF0899 = 7373, kF1175 = 9633, kF1501 = 12299,
              kF1847 = 15137, kF1961 = 16069, kF2053 = 16819, kF2562 = 20995, kF3072 = 25172;

// One 1-D pass over d[0..7] (stride s), in place. FIRST: the row pass (outputs scaled up by 2^PASS1_BITS), else the column pass.
// Samples are 8-bit, so every sum stays far inside 32 bits.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int* d, int s) {
  const int d0 = d[0], d1 = d[s], d2 = d[2 * s], d3 = d[3 * s], d4 = d[4 * s], d5 = d[5 * s], d6 = d[6 * s], d7 = d[7 * s];
  int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
  const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  constexpr int sh = FIRST ? 11 : 15, rnd = 1 << (sh - 1);        // CONST_BITS -/+ PASS1_BITS
  if (FIRST) {
    d[0] = (tmp10 + tmp11) * 4, d[4 * s] = (tmp10 - tmp11) * 4;
  } else {
    d[0] = (tmp10 + tmp11 + 2) >> 2, d[4 * s] = (tmp10 - tmp11 + 2) >> 2;
  }
  int z1 = (tmp12 + tmp13) * kF0541;
  d[2 * s] = (z1 + tmp13 * kF0765 + rnd) >> sh;
  d[6 * s] = (z1 - tmp12 * kF1847 + rnd) >> sh;
  z1 = tmp4 + tmp7;
  int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int z5 = (z3 + z4) * kF1175;
  tmp4 *= kF0298, tmp5 *= kF2053, tmp6 *= kF3072, tmp7 *= kF1501;
  z1 *= -kF0899, z2 *= -kF2562, z3 *= -kF1961, z4 *= -kF0390;
  z3 += z5, z4 += z5;
  d[7 * s] = (tmp4 + z1 + z3 + rnd) >> sh;
  d[5 * s] = (tmp5 + z2 + z4 + rnd) >> sh;
  d[3 * s] = (tmp6 + z2 + z3 + rnd) >> sh;
  d[s] = (tmp7 + z1 + z4 + rnd) >> sh;
}

constexpr int kFdctLanes = 64, kWsStride = 65;

// One lane owns one 8x8 block (scan order, as jpeg_idct_kernel numbers them); its workspace is 65 LDS words, so lane l's word j
// falls in bank (l + j) % 64. dense: [n_blocks][64] int16, the block's zigzag run from position 0 (what lies past the block's
// length is not written and never read); lens: the length (last non-zero position + 1, 0 for an all-zero block).
__global__ __launch_bounds__(kFdctLanes) void jpeg_fdct_kernel(const uint8_t* __restrict__ planes, RecordHeader hd, const uint16_t* __restrict__ quant,
                                                              int16_t* __restrict__ dense, uint32_t* __restrict__ lens) {
  __shared__ int ws_all[kFdctLanes * kWsStride];
  const uint32_t b = blockIdx.x * kFdctLanes + threadIdx.x;
  if (b >= hd.n_blocks) return;                                  // no barrier below: a lane works on its own 65 words
  int* ws = ws_all + threadIdx.x * kWsStride;
  const uint32_t luma = hd.hs * hd.vs, bpm = hd.ncomp == 1 ? 1u : luma + 2u;
  const uint32_t mcu = b / bpm, k = b - mcu * bpm, mx = mcu % hd.mcus_x, my = mcu / hd.mcus_x;
  uint32_t c, bx, by;
  if (hd.ncomp == 1 || k < luma) {
    c = 0, bx = mx * hd.hs + k % hd.hs, by = my * hd.vs + k / hd.hs;
  } else {
    c = 1 + (k - luma), bx = mx, by = my;
  }
  if (c >= hd.ncomp || bx >= hd.bw[c] || by >= hd.bh[c]) {        // cannot happen for a header of make_header
    lens[b] = 0;
    return;
  }
  // jccoefct.c: a luma block past the component's own grid (ceil(w / 8) x ceil(h / 8)) only fills up the MCU: no AC, the DC of
  // the block before it in the MCU -- right edge: the last real block of its row; bottom row: the last block of the MCU's row above
  bool dummy = false;
  if (c == 0) {
    const uint32_t rbw = (hd.width + 7) / 8, rbh = (hd.height + 7) / 8;
    if (by >= rbh) {
      dummy = true, by = rbh - 1, bx = min(mx * hd.hs + hd.hs - 1, rbw - 1);
    } else if (bx >= rbw) {
      dummy = true, bx = rbw - 1;
    }
  }
  size_t plane_off = 0;
  for (uint32_t i = 0; i < c; ++i) plane_off += 64 * (size_t)hd.bw[i] * hd.bh[i];
  const size_t stride = 8 * (size_t)hd.bw[c];
  const uint8_t* src = planes + plane_off + (size_t)by * 8 * stride + (size_t)bx * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint2 v = *reinterpret_cast<const uint2*>(src + (size_t)r * stride);   // 8-byte aligned: plane sizes and offsets are multiples of 64 / 8
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ws[8 * r + j] = (int)((v.x >> (8 * j)) & 255u) - 128;
      ws[8 * r + 4 + j] = (int)((v.y >> (8 * j)) & 255u) - 128;
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct8<true>(ws + 8 * r, 1);
#pragma unroll
  for (int col = 0; col < 8; ++col) fdct8<false>(ws + col, 8);
  // jcdctmgr.c: the divisor is 8 * q (the DCT's output is scaled by 8); half of it is added to the magnitude, the division truncates
  const uint16_t* q = quant + 64 * c;
  uint32_t len = 0;
  uint32_t packed[4];
  uint4* out = reinterpret_cast<uint4*>(dense + (size_t)b * 64);
#pragma unroll
  for (int z = 0; z < 64; ++z) {
    const int nat = kNaturalEnc[z];
    int v = 0;
    if (z == 0 || !dummy) {
      const int t = ws[nat], div = (int)max((uint32_t)q[nat], 1u) << 3;
      const int mag = ((t < 0 ? -t : t) + (div >> 1)) / div;
      v = t < 0 ? -mag : mag;
    }
    if (v != 0) len = (uint32_t)z + 1;
    const uint32_t u = (uint32_t)(uint16_t)(int16_t)v;
    if (z & 1) packed[(z >> 1) & 3] |= u << 16; else packed[(z >> 1) & 3] = u;
    if ((z & 7) == 7) out[z >> 3] = make_uint4(packed[0], packed[1], packed[2], packed[3]);
  }
  lens[b] = len;
}

// One lane per (block, position): coefficient z of block b goes to coef[offset[b] + z] when z is inside the block's run.
// cap: coefficients the stream has room for (64 per block: never exceeded by offsets the scan made from lengths <= 64).
__global__ __launch_bounds__(256) void jpeg_compact_kernel(const int16_t* __restrict__ dense, const uint32_t* __restrict__ offsets, uint32_t n_blocks,
                                                           size_t cap, int16_t* __restrict__ coef) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t b = i >> 6;
  const uint32_t z = (uint32_t)(i & 63);
  if (b >= n_blocks) return;
  const uint32_t first = offsets[b], last = offsets[b + 1];
  if (last < first || z >= last - first || (size_t)first + z >= cap) return;
  coef[(size_t)first + z] = dense[i];
}
}  // namespace

void JpegEncoder::check_args(int h, int w, int quality, int subsampling) {
  if (h <= 0 || w <= 0 || h > jpeg::kMaxDim || w > jpeg::kMaxDim) fail(GTX_ERR_INVALID, "jpeg_enc: a %d x %d frame is outside 1..%d", w, h, jpeg::kMaxDim);
  if (quality < 1 || quality > 100) fail(GTX_ERR_INVALID, "jpeg_enc: quality %d is outside 1..100", quality);
  if (subsampling != 0 && subsampling != 2) fail(GTX_ERR_INVALID, "jpeg_enc: subsampling %d (0 = 4:4:4, 2 = 4:2:0)", subsampling);
}

JpegEncoder::JpegEncoder(gtx_ctx* ctx, int h, int w, int quality, int subsampling) : ctx_(ctx) {
  check_args(h, w, quality, subsampling);
  if (!ctx) fail(GTX_ERR_INVALID, "ctx is NULL");
  const int s = subsampling == 2 ? 2 : 1;
  if (!jpeg::make_header(h, w, 3, s, s, &hd_) || !jpeg::quality_tables(quality, quant_[0], quant_[1])) fail(GTX_ERR_INTERNAL, "jpeg_enc: header");
  memcpy(quant_[2], quant_[1], sizeof quant_[1]);
  GTX_HIP(hipSetDevice(ctx->device));
  const size_t nb = hd_.n_blocks, n_tiles = (nb + kJpegScanTile - 1) / kJpegScanTile;
  d_planes_.alloc(jpeg::planes_bytes(hd_));
  d_quant_.alloc(sizeof quant_);
  d_dense_.alloc(nb * 64 * sizeof(int16_t));
  d_lens_.alloc(nb * sizeof(uint32_t));
  d_tiles_.alloc(n_tiles * sizeof(uint32_t));
  d_rec_.alloc(4 * (nb + 1) + 2 * 64 * nb);
  GTX_HIP(hipMemcpy(d_quant_.p, quant_, sizeof quant_, hipMemcpyHostToDevice));
  GTX_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_total_), sizeof(uint32_t), hipHostMallocDefault));
  GTX_HIP(hipEventCreateWithFlags(&e0_, wait_event_flags(true)));
  GTX_HIP(hipEventCreateWithFlags(&e1_, wait_event_flags(true)));
  GTX_HIP(hipEventCreateWithFlags(&eh_, wait_event_flags(true)));
}

JpegEncoder::~JpegEncoder() {
  if (in_flight_) (void)hipEventSynchronize(e1_);
  if (e0_) (void)hipEventDestroy(e0_);
  if (e1_) (void)hipEventDestroy(e1_);
  if (eh_) (void)hipEventDestroy(eh_);
  if (h_total_) (void)hipHostFree(h_total_);
}

void JpegEncoder::submit(const void* bgr) {
  if (!bgr) fail(GTX_ERR_INVALID, "bgr is NULL");
  if (in_flight_) fail(GTX_ERR_INVALID, "jpeg_enc_submit: the frame submitted before has not been collected");
  GTX_HIP(hipSetDevice(ctx_->device));
  hipStream_t s = ctx_->stream;
  const uint32_t nb = hd_.n_blocks;
  uint32_t* offsets = d_rec_.as<uint32_t>();
  int16_t* coef = reinterpret_cast<int16_t*>(d_rec_.as<uint8_t>() + 4 * ((size_t)nb + 1));
  GTX_HIP(hipEventRecord(e0_, s));
  hipLaunchKernelGGL(jpeg_planes_kernel, dim3(cdiv(8 * (int)hd_.bw[1], 256), 8 * hd_.bh[1]), dim3(256), 0, s, static_cast<const uint8_t*>(bgr), hd_,
                     d_planes_.as<uint8_t>());
  hipLaunchKernelGGL(jpeg_fdct_kernel, dim3(cdiv((int)nb, kFdctLanes)), dim3(kFdctLanes), 0, s, d_planes_.as<const uint8_t>(), hd_,
                     d_quant_.as<const uint16_t>(), d_dense_.as<int16_t>(), d_lens_.as<uint32_t>());
  if (huff_) {                                                    // the GPU entropy route: no record, the picture instead
    GTX_HIP(hipGetLastError());
    GTX_HIP(hipEventRecord(eh_, s));
    huff_->enqueue(d_dense_.as<const int16_t>(), d_lens_.as<const uint32_t>());
    GTX_HIP(hipEventRecord(e1_, s));
    in_flight_ = submitted_ = true;
    return;
  }
  jpegscan::scan_launch<uint32_t>(s, d_lens_.as<const uint32_t>(), nb, nullptr, 64u, d_tiles_.as<uint32_t>(), offsets, offsets + nb);
  hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)(((size_t)nb * 64 + 255) / 256)), dim3(256), 0, s, d_dense_.as<const int16_t>(), offsets, nb,
                     (size_t)64 * nb, coef);
  GTX_HIP(hipGetLastError());
  GTX_HIP(hipEventRecord(e1_, s));
  GTX_HIP(hipMemcpyAsync(h_total_, offsets + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  in_flight_ = submitted_ = true;
}

void JpegEncoder::use_gpu_entropy() {
  if (huff_) return;
  if (submitted_) fail(GTX_ERR_INVALID, "jpeg_enc_set_entropy: the encoder has already been given a frame");
  GTX_HIP(hipSetDevice(ctx_->device));
  huff_.reset(new JpegHuff(ctx_, hd_, &quant_[0][0]));
  d_rec_.release();                                               // no record is made on this route
  d_tiles_.release();
}

bool JpegEncoder::collect_jpeg(void* out, size_t capacity, size_t* bytes) {
  if (!huff_) fail(GTX_ERR_INVALID, "jpeg_enc_collect_jpeg: the encoder is on the host entropy route (gtx_jpeg_enc_collect returns its record)");
  if (!in_flight_) fail(GTX_ERR_INVALID, "jpeg_enc_collect_jpeg: no frame has been submitted");
  if (!bytes) fail(GTX_ERR_INVALID, "bytes is NULL");
  if (!out && capacity) fail(GTX_ERR_INVALID, "jpeg_enc_collect_jpeg: out is NULL with a capacity of %zu", capacity);
  GTX_HIP(hipSetDevice(ctx_->device));
  bool fits = false;
  try {
    fits = huff_->finish(out, capacity, bytes, nullptr);
  } catch (...) {
    in_flight_ = false;                                           // a frame that cannot be coded is given up
    throw;
  }
  if (!fits) return false;
  GTX_HIP(hipEventElapsedTime(&last_ms_, e0_, e1_));
  GTX_HIP(hipEventElapsedTime(&entropy_ms_, eh_, e1_));
  in_flight_ = false;
  return true;
}

bool JpegEncoder::collect(void* record, size_t capacity, size_t* bytes) {
  if (huff_) fail(GTX_ERR_INVALID, "jpeg_enc_collect: the encoder is on the GPU entropy route (gtx_jpeg_enc_collect_jpeg returns its picture)");
  if (!in_flight_) fail(GTX_ERR_INVALID, "jpeg_enc_collect: no frame has been submitted");
  if (!bytes) fail(GTX_ERR_INVALID, "bytes is NULL");
  if (!record && capacity) fail(GTX_ERR_INVALID, "jpeg_enc_collect: record is NULL with a capacity of %zu", capacity);
  if (record && (reinterpret_cast<uintptr_t>(record) & 3)) fail(GTX_ERR_INVALID, "jpeg_enc_collect: the record buffer is not 4-byte aligned");
  GTX_HIP(hipSetDevice(ctx_->device));
  GTX_HIP(hipStreamSynchronize(ctx_->stream));                    // the chain and the copy of the closing offset
  const size_t nb = hd_.n_blocks, n_coef = *h_total_;
  if (n_coef > 64 * nb) fail(GTX_ERR_INTERNAL, "jpeg_enc_collect: the device reports %zu coefficients for %zu blocks", n_coef, nb);
  const size_t total = jpeg::record_bytes(nb, n_coef);
  *bytes = total;
  if (capacity < total) return false;
  jpeg::RecordHeader hd = hd_;
  hd.n_coef = (uint32_t)n_coef, hd.bytes = (uint32_t)total;
  uint8_t* rec = static_cast<uint8_t*>(record);
  memcpy(rec, &hd, sizeof hd);
  memcpy(rec + jpeg::kQuantOffset, quant_, sizeof quant_);
  GTX_HIP(hipMemcpyAsync(rec + jpeg::kOffsetsOffset, d_rec_.p, total - jpeg::kOffsetsOffset, hipMemcpyDeviceToHost, ctx_->stream));   // the real length only
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  GTX_HIP(hipEventElapsedTime(&last_ms_, e0_, e1_));
  in_flight_ = false;
  return true;
}

}  // namespace gtx
