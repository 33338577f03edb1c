// Baseline JPEG, the entropy half of writing, on the GPU: what cv2.VideoWriter.write() (geotrax/visualize.py:298) does after
// quantisation. The dense zigzag runs and block lengths jpeg_fdct_kernel leaves in HBM become the finished picture in HBM, byte
// for byte what the host emitter (csrc/jpeg_emit.cpp emit(), the specification) writes for the same blocks. Encoding with the
// fixed Annex K.3 tables is parallel work: a block's code depends on its own coefficients and one other block's DC value, its
// position in the stream is a prefix sum, and byte stuffing is a count and a scatter. Eleven launches per frame:
//
//   jpeg_huff_bits_kernel      one lane per block: the bits emit() would write for it (DC difference against the block before it
//                              of the same component in scan order, AC run/size codes, ZRLs, EOB)
//   jpegscan::scan_* <u64>     exclusive prefix sum of the bit counts -> every block's bit offset; the total
//   jpeg_huff_zero_kernel      zeroes the bit buffer as far as the total reaches
//   jpeg_huff_pack_kernel      one lane per block: its code at its bit offset, MSB first; words shared with a neighbour are
//                              combined with atomicOr, words a block owns are stored; the last block pads with 1-bits
//   jpeg_huff_ffcount_kernel   one lane per kJpegStuffChunk bytes of the packed scan: its FF bytes
//   jpegscan::scan_* <u64>     exclusive prefix sum of the counts
//   jpeg_huff_stuff_kernel     one lane per chunk: its bytes to their final place behind the header, a 00 after every FF; the
//                              last chunk's lane closes the picture with EOI and writes its length
//
// The header (SOI .. SOS) is built once by jpeg::header(), the function emit() itself calls, and stays in front of the scan.
// Every count that depends on the data stays in HBM (the grids are sized for the worst case, workgroups past the real size
// leave at once), so nothing between the first launch and the last needs the host.
#include <hip/hip_runtime.h>

#include "detector.hpp"
#include "jpeg_enc.hpp"
#include "jpeg_scan.hpp"

namespace gtx {
namespace {

constexpr int kDcEntries = 2 * 12, kCodeEntries = kDcEntries + 2 * 256;   // HuffCodes as one uint32 array
// d_state_: uint64[4]
constexpr int kStBits = 0, kStFf = 1, kStBytes = 2, kStErr = 3;
constexpr size_t kPackedSlack = 128;            // the bit buffer past the bound: whole 16-byte stores and whole chunks may reach there

struct HuffGeom {
  uint32_t nb, bpm, luma;                        // blocks, blocks per MCU, luma blocks per MCU (bpm == 1: one component)
};

__device__ __forceinline__ int bit_length(uint32_t v) { return v ? 32 - __clz(v) : 0; }

// the block whose DC value block b's is predicted from (emit()'s pred[c] walk), or -1: the first block of its component
__device__ __forceinline__ int64_t dc_predecessor(uint32_t b, const HuffGeom& g, int* chroma) {
  if (g.bpm == 1) {
    *chroma = 0;
    return (int64_t)b - 1;
  }
  const uint32_t mcu = b / g.bpm, k = b - mcu * g.bpm;
  *chroma = k >= g.luma;
  if (k < g.luma && k > 0) return (int64_t)b - 1;
  if (mcu == 0) return -1;
  return k == 0 ? (int64_t)b - g.bpm + g.luma - 1 : (int64_t)b - g.bpm;   // the MCU before: its last luma block, or the same chroma block
}

struct CountSink {
  uint32_t bits = 0;
  __device__ __forceinline__ void put(uint32_t, int k) { bits += (uint32_t)k; }
};

// Bits go out MSB first. The buffer is read as bytes in stream order afterwards, so a 32-bit group is stored byte-swapped.
struct PackSink {
  uint32_t* w;
  uint64_t acc = 0;                              // the low `fill` bits are pending, oldest highest
  int fill;
  bool shared;                                   // the word at w also holds the end of the block before
  __device__ __forceinline__ PackSink(uint32_t* words, uint64_t bit) : w(words + (bit >> 5)), fill((int)(bit & 31)), shared((bit & 31) != 0) {}
  __device__ __forceinline__ void put(uint32_t v, int k) {       // k <= 16, v < 2^k; fill < 32 before, so at most 47 bits pend
    acc = (acc << k) | v;
    fill += k;
    if (fill >= 32) {
      const uint32_t word = __builtin_bswap32((uint32_t)(acc >> (fill - 32)));
      if (shared) atomicOr(w, word); else *w = word;
      shared = false;
      ++w, fill -= 32;
    }
  }
  __device__ __forceinline__ void finish() {                     // the rest shares its word with the block behind
    if (fill) atomicOr(w, __builtin_bswap32((uint32_t)(acc << (32 - fill))));
  }
};

// emit()'s inner loop for one block. v: the block's 64 positions, read below len only; tab: HuffCodes in LDS. A value the
// tables cannot code sets *bad and is coded as the largest category, so that the bit count stays inside kJpegMaxBlockBits.
template <class Sink>
__device__ __forceinline__ void code_block(const int16_t* __restrict__ v, int len, int pred, int chroma, const uint32_t* tab, Sink& sink, bool* bad) {
  const uint32_t* dc = tab + 12 * chroma;
  const uint32_t* ac = tab + kDcEntries + 256 * chroma;
  const int dcv = len ? v[0] : 0, diff = dcv - pred;
  int s = bit_length((uint32_t)(diff < 0 ? -diff : diff));
  if (s > 11) *bad = true, s = 11;
  sink.put(dc[s] & 0xFFFFu, (int)(dc[s] >> 16));
  if (s) sink.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
  int run = 0, a = 0;
  for (int z0 = 0; z0 < len; z0 += 8) {                          // eight positions per 16-byte load
    const uint4 q = *reinterpret_cast<const uint4*>(v + z0);
    const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int z = z0 + j;
      if (z == 0 || z >= len) continue;
      a = (int)(int16_t)(w4[j >> 1] >> (16 * (j & 1)));
      if (a == 0) {
        ++run;
        continue;
      }
      for (; run > 15; run -= 16) sink.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
      s = bit_length((uint32_t)(a < 0 ? -a : a));
      if (s > 10) *bad = true, s = 10;
      const uint32_t e = ac[run << 4 | s];
      sink.put(e & 0xFFFFu, (int)(e >> 16));
      sink.put((uint32_t)(a < 0 ? a - 1 : a) & ((1u << s) - 1u), s);
      run = 0;
    }
  }
  // emit(): zeros up to position 63 follow unless the run is 64 long and ends in a non-zero (`a` is position len - 1 then);
  // a run that ends in zeros inside the record counts among them, its pending zeros are dropped
  if (!(len == 64 && a != 0)) sink.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}

__device__ __forceinline__ void load_codes(const uint32_t* __restrict__ codes, uint32_t* tab) {
  for (int i = (int)threadIdx.x; i < kCodeEntries; i += kJpegPackChunk) tab[i] = codes[i];
  __syncthreads();
}

__device__ __forceinline__ int dc_of(const int16_t* __restrict__ dense, const uint32_t* __restrict__ lens, int64_t p) {
  return p >= 0 && lens[p] ? (int)dense[(size_t)p * 64] : 0;
}

__global__ __launch_bounds__(kJpegPackChunk) void jpeg_huff_bits_kernel(const int16_t* __restrict__ dense, const uint32_t* __restrict__ lens, HuffGeom g,
                                                                        const uint32_t* __restrict__ codes, uint32_t* __restrict__ bits,
                                                                        uint32_t* __restrict__ err) {
  __shared__ uint32_t tab[kCodeEntries];
  load_codes(codes, tab);
  const uint32_t b = blockIdx.x * kJpegPackChunk + threadIdx.x;
  if (b >= g.nb) return;
  int chroma;
  const int64_t p = dc_predecessor(b, g, &chroma);
  CountSink sink;
  bool bad = false;
  code_block(dense + (size_t)b * 64, (int)min(lens[b], 64u), dc_of(dense, lens, p), chroma, tab, sink, &bad);
  bits[b] = sink.bits;
  if (bad) atomicOr(err, 1u);
}

// 16 bytes per lane, up to the word behind the scan's last (the pack's closing atomicOr never reaches further)
__global__ __launch_bounds__(256) void jpeg_huff_zero_kernel(const uint64_t* __restrict__ state, size_t cap_bytes, uint4* __restrict__ packed) {
  const size_t at = ((size_t)blockIdx.x * 256 + threadIdx.x) * 16;
  const size_t need = (size_t)((state[kStBits] + 7) / 8) + 8;
  if (at < need && at + 16 <= cap_bytes) packed[at / 16] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kJpegPackChunk) void jpeg_huff_pack_kernel(const int16_t* __restrict__ dense, const uint32_t* __restrict__ lens, HuffGeom g,
                                                                        const uint32_t* __restrict__ codes, const uint32_t* __restrict__ bits,
                                                                        const uint64_t* __restrict__ bit_off, uint32_t* __restrict__ packed) {
  __shared__ uint32_t tab[kCodeEntries];
  load_codes(codes, tab);
  const uint32_t b = blockIdx.x * kJpegPackChunk + threadIdx.x;
  if (b >= g.nb) return;
  int chroma;
  const int64_t p = dc_predecessor(b, g, &chroma);
  const uint64_t at = bit_off[b];
  PackSink sink(packed, at);
  bool bad = false;
  code_block(dense + (size_t)b * 64, (int)min(lens[b], 64u), dc_of(dense, lens, p), chroma, tab, sink, &bad);
  if (b == g.nb - 1) {                                            // Writer::flush: the last byte is padded with 1-bits
    const int pad = (int)((0 - (at + bits[b])) & 7);
    if (pad) sink.put((1u << pad) - 1u, pad);
  }
  sink.finish();
}

// the 64 bytes of chunk i as 16 stream-order words; bytes at or past `end` read as 0
__device__ __forceinline__ uint32_t ff_count(const uint32_t* w, uint64_t first, uint64_t end) {
  uint32_t n = 0;
#pragma unroll
  for (int j = 0; j < kJpegStuffChunk; ++j)
    if (first + j < end && ((w[j >> 2] >> (8 * (j & 3))) & 255u) == 255u) ++n;
  return n;
}

__device__ __forceinline__ void load_chunk(const uint8_t* __restrict__ packed, uint64_t i, uint32_t* w) {
  const uint4* src = reinterpret_cast<const uint4*>(packed + i * kJpegStuffChunk);
#pragma unroll
  for (int j = 0; j < kJpegStuffChunk / 16; ++j) {
    const uint4 q = src[j];
    w[4 * j] = q.x, w[4 * j + 1] = q.y, w[4 * j + 2] = q.z, w[4 * j + 3] = q.w;
  }
}

__global__ __launch_bounds__(256) void jpeg_huff_ffcount_kernel(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ state,
                                                                uint32_t* __restrict__ ff_cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, bytes = (state[kStBits] + 7) / 8;
  if (i >= jpegscan::stuff_chunks(state[kStBits])) return;
  uint32_t w[kJpegStuffChunk / 4];
  load_chunk(packed, i, w);
  ff_cnt[i] = ff_count(w, i * kJpegStuffChunk, bytes);
}

// pic: the header is in place; the scan follows it. cap: bytes of pic (jpeg_picture_bound: never reached by a scan inside its bound).
__global__ __launch_bounds__(256) void jpeg_huff_stuff_kernel(const uint8_t* __restrict__ packed, const uint64_t* __restrict__ ff_off, size_t header_len,
                                                              size_t cap, uint8_t* __restrict__ pic, uint64_t* __restrict__ state) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x, bytes = (state[kStBits] + 7) / 8, chunks = jpegscan::stuff_chunks(state[kStBits]);
  if (i >= chunks) return;
  uint32_t w[kJpegStuffChunk / 4];
  load_chunk(packed, i, w);
  size_t at = header_len + (size_t)(i * kJpegStuffChunk + ff_off[i]);
#pragma unroll
  for (int j = 0; j < kJpegStuffChunk; ++j) {
    const uint32_t v = (w[j >> 2] >> (8 * (j & 3))) & 255u;
    if (i * kJpegStuffChunk + j < bytes) {                         // (no break: the loop unrolls and w stays in registers)
      if (at < cap) pic[at] = (uint8_t)v;
      ++at;
      if (v == 255u) {
        if (at < cap) pic[at] = 0;
        ++at;
      }
    }
  }
  if (i == chunks - 1) {
    if (at + 2 <= cap) pic[at] = 0xFF, pic[at + 1] = 0xD9;
    state[kStBytes] = at + 2;
  }
}

}  // namespace

JpegHuff::JpegHuff(gtx_ctx* ctx, const jpeg::RecordHeader& hd, const uint16_t* quant) : ctx_(ctx) {
  if (!ctx) fail(GTX_ERR_INVALID, "ctx is NULL");
  nb_ = hd.n_blocks;
  luma_ = hd.hs * hd.vs, bpm_ = hd.ncomp == 1 ? 1u : luma_ + 2u;
  if (nb_ == 0 || nb_ % bpm_) fail(GTX_ERR_INVALID, "jpeg_huff: %u blocks are not whole MCUs of %u", nb_, bpm_);
  uint8_t header[jpeg::kMaxHeaderBytes];
  header_len_ = jpeg::header(hd, quant, header, sizeof header);
  if (header_len_ > sizeof header) fail(GTX_ERR_INTERNAL, "jpeg_huff: a header of %zu bytes", header_len_);
  jpeg::HuffCodes codes;
  jpeg::std_huff_codes(&codes);
  static_assert(sizeof(jpeg::HuffCodes) == kCodeEntries * sizeof(uint32_t), "HuffCodes is one uint32 array");
  GTX_HIP(hipSetDevice(ctx->device));
  const size_t scan = jpeg_scan_bound(nb_), chunks = (scan + kJpegStuffChunk - 1) / kJpegStuffChunk;
  d_codes_.alloc(sizeof codes);
  d_bits_.alloc((size_t)nb_ * sizeof(uint32_t));
  d_bitoff_.alloc((size_t)nb_ * sizeof(uint64_t));
  d_tiles_.alloc(((size_t)nb_ + kJpegScanTile - 1) / kJpegScanTile * sizeof(uint64_t));
  d_packed_.alloc((scan + kPackedSlack + 15) / 16 * 16);
  d_ffcnt_.alloc(chunks * sizeof(uint32_t));
  d_ffoff_.alloc(chunks * sizeof(uint64_t));
  d_fftiles_.alloc((chunks + kJpegScanTile - 1) / kJpegScanTile * sizeof(uint64_t));
  d_pic_.alloc(jpeg_picture_bound(nb_));
  d_state_.alloc(4 * sizeof(uint64_t));
  GTX_HIP(hipMemcpy(d_codes_.p, &codes, sizeof codes, hipMemcpyHostToDevice));
  GTX_HIP(hipMemcpy(d_pic_.p, header, header_len_, hipMemcpyHostToDevice));
  GTX_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_state_), 4 * sizeof(uint64_t), hipHostMallocDefault));
}

JpegHuff::~JpegHuff() {
  if (h_state_) (void)hipHostFree(h_state_);
}

void JpegHuff::enqueue(const int16_t* d_dense, const uint32_t* d_lens) {
  hipStream_t s = ctx_->stream;
  const HuffGeom g{nb_, bpm_, luma_};
  const size_t scan = jpeg_scan_bound(nb_), chunks = (scan + kJpegStuffChunk - 1) / kJpegStuffChunk;
  uint64_t* state = d_state_.as<uint64_t>();
  const unsigned wgs = (unsigned)(((size_t)nb_ + kJpegPackChunk - 1) / kJpegPackChunk), chunk_wgs = (unsigned)((chunks + 255) / 256);
  GTX_HIP(hipMemsetAsync(state, 0, 4 * sizeof(uint64_t), s));
  hipLaunchKernelGGL(jpeg_huff_bits_kernel, dim3(wgs), dim3(kJpegPackChunk), 0, s, d_dense, d_lens, g, d_codes_.as<const uint32_t>(), d_bits_.as<uint32_t>(),
                     reinterpret_cast<uint32_t*>(state + kStErr));
  jpegscan::scan_launch<uint64_t>(s, d_bits_.as<const uint32_t>(), nb_, nullptr, 0xFFFFFFFFu, d_tiles_.as<uint64_t>(), d_bitoff_.as<uint64_t>(),
                                  state + kStBits);
  // zeroing, ordered ahead of the pack on the same stream
  hipLaunchKernelGGL(jpeg_huff_zero_kernel, dim3((unsigned)((d_packed_.bytes / 16 + 255) / 256)), dim3(256), 0, s, state, d_packed_.bytes,
                     d_packed_.as<uint4>());
  hipLaunchKernelGGL(jpeg_huff_pack_kernel, dim3(wgs), dim3(kJpegPackChunk), 0, s, d_dense, d_lens, g, d_codes_.as<const uint32_t>(),
                     d_bits_.as<const uint32_t>(), d_bitoff_.as<const uint64_t>(), d_packed_.as<uint32_t>());
  hipLaunchKernelGGL(jpeg_huff_ffcount_kernel, dim3(chunk_wgs), dim3(256), 0, s, d_packed_.as<const uint8_t>(), state, d_ffcnt_.as<uint32_t>());
  jpegscan::scan_launch<uint64_t>(s, d_ffcnt_.as<const uint32_t>(), chunks, state + kStBits, 0xFFFFFFFFu, d_fftiles_.as<uint64_t>(),
                                  d_ffoff_.as<uint64_t>(), state + kStFf);
  hipLaunchKernelGGL(jpeg_huff_stuff_kernel, dim3(chunk_wgs), dim3(256), 0, s, d_packed_.as<const uint8_t>(), d_ffoff_.as<const uint64_t>(), header_len_,
                     d_pic_.bytes, d_pic_.as<uint8_t>(), state);
  GTX_HIP(hipGetLastError());
  GTX_HIP(hipMemcpyAsync(h_state_, state, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
}

bool JpegHuff::finish(void* out, size_t capacity, size_t* bytes, uint32_t* bits) {
  GTX_HIP(hipStreamSynchronize(ctx_->stream));                    // the launches and the copy of the sizes
  if (h_state_[kStErr]) fail(GTX_ERR_INVALID, "JPEG record: a DC difference beyond 11 bits or an AC coefficient beyond 10 bits (no Annex K.3 code)");
  const size_t total = (size_t)h_state_[kStBytes];
  if (total < header_len_ + 3 || total > d_pic_.bytes) fail(GTX_ERR_INTERNAL, "jpeg_huff: the device reports a picture of %zu bytes for %u blocks", total, nb_);
  *bytes = total;
  if (capacity < total) return false;
  GTX_HIP(hipMemcpyAsync(out, d_pic_.p, total, hipMemcpyDeviceToHost, ctx_->stream));   // the real length only
  if (bits) GTX_HIP(hipMemcpyAsync(bits, d_bits_.p, (size_t)nb_ * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx_->stream));
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  return true;
}

}  // namespace gtx
