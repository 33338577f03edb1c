// Device half of the JPEG frame sink (csrc/jpeg_enc.hip): packed BGR in HBM -> the packed record of jpeg_parse.hpp, which the
// host emitter (csrc/jpeg_emit.cpp) Huffman-codes into a baseline JPEG; or, opt-in, the GPU entropy coder (csrc/jpeg_huff.hip),
// which turns the dense runs in HBM into the finished picture, byte for byte the emitter's.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>

#include "common.hpp"
#include "jpeg_emit.hpp"

struct gtx_ctx;

namespace gtx {

// Blocks one workgroup of the prefix sum covers (256 lanes x 4 lengths): the tile of the multi-workgroup scan.
constexpr int kJpegScanTile = 1024;
// Blocks one workgroup of the bit-count and pack passes covers: one lane per 8x8 block.
constexpr int kJpegPackChunk = 64;
// Bytes of the packed scan one lane of the stuff passes owns: it counts the chunk's FF bytes, and after the prefix sum of the
// counts writes the chunk, a 00 after every FF, at its final position.
constexpr int kJpegStuffChunk = 64;

// Most bits emit() can write for one block: the longest DC code with its amplitude (chroma category 11: 11 + 11), and for every
// one of the 63 AC positions the longest AC code with the longest amplitude (16 + 10). A position that holds a zero costs less
// (a ZRL, at most 11 bits, covers 16 of them), and the EOB (at most 4 bits) is only written when position 63 is zero, which
// saves 26. So 22 + 63 * 26 = 1660 bits.
constexpr size_t kJpegMaxBlockBits = 22 + 63 * 26;
// Bytes of the unstuffed scan of n_blocks blocks at most, the last byte padded.
inline size_t jpeg_scan_bound(size_t n_blocks) { return (n_blocks * kJpegMaxBlockBits + 7) / 8; }
// Bytes of the finished picture at most: the header, the scan with every byte an FF (a 00 after each: twice the bytes), EOI.
inline size_t jpeg_picture_bound(size_t n_blocks) { return jpeg::kMaxHeaderBytes + 2 * jpeg_scan_bound(n_blocks) + 2; }

// The entropy coder on the GPU: dense zigzag runs [n_blocks][64] + block lengths in HBM (what jpeg_fdct_kernel leaves behind)
// -> the finished picture in HBM (header + stuffed scan + EOI, contiguous). Bit offsets are 64-bit throughout (a 16384 x 16384
// frame in 4:4:4 can need 2.1e10 bits), so no frame size the encoder accepts is refused here. Eleven launches, all enqueued on
// the context's stream by enqueue(); only finish() waits.
class JpegHuff {
 public:
  JpegHuff(gtx_ctx* ctx, const jpeg::RecordHeader& hd, const uint16_t* quant /* [3][64] */);
  ~JpegHuff();
  void enqueue(const int16_t* d_dense, const uint32_t* d_lens);   // no wait; the result's sizes follow on the same stream
  // Waits for the stream. Throws GTX_ERR_INVALID when a coefficient had no Annex K.3 code. *bytes: the picture's length;
  // false: capacity < *bytes, nothing was copied. bits (may be NULL): the per-block bit counts, n_blocks of them.
  bool finish(void* out, size_t capacity, size_t* bytes, uint32_t* bits);
  size_t header_bytes() const { return header_len_; }

 private:
  gtx_ctx* ctx_;
  uint32_t nb_ = 0, bpm_ = 1, luma_ = 1;
  size_t header_len_ = 0;
  DevBuf d_codes_, d_bits_, d_bitoff_, d_tiles_, d_packed_, d_ffcnt_, d_ffoff_, d_fftiles_, d_pic_, d_state_;
  uint64_t* h_state_ = nullptr;                                   // pinned copy of d_state_: picture bytes, error flag
};

// One encoder for frames of one size, quality and sampling: its scratch in HBM and the stream-ordered chain
// planes -> forward DCT + quantisation -> prefix sum of the block lengths -> compaction (or, on the GPU entropy route, -> the
// entropy coder). One frame may be in flight per object.
class JpegEncoder {
 public:
  // subsampling: 0 = 4:4:4, 2 = 4:2:0 (libjpeg-turbo's numbering). Refuses bad sizes before anything is allocated.
  JpegEncoder(gtx_ctx* ctx, int h, int w, int quality, int subsampling);
  ~JpegEncoder();
  static void check_args(int h, int w, int quality, int subsampling);   // throws GTX_ERR_INVALID; host only
  void submit(const void* bgr);                                   // enqueues the chain on the context's stream; no wait
  // Waits for the chain, then copies the record at its real length into record[0, capacity). false: capacity < *bytes, nothing
  // was copied and the frame stays collectable.
  bool collect(void* record, size_t capacity, size_t* bytes);
  float last_ms() const { return last_ms_; }                      // the chain of the frame collected last, between two events
  // Switches to the GPU entropy route (before the first submit only): submit() then enqueues the entropy coder after the
  // forward DCT instead of the offset scan and the compaction, and collect_jpeg() replaces collect().
  void use_gpu_entropy();
  bool gpu_entropy() const { return (bool)huff_; }
  bool collect_jpeg(void* out, size_t capacity, size_t* bytes);   // collect()'s contract, for the finished picture
  float entropy_ms() const { return entropy_ms_; }                // the entropy launches alone of the frame collected last
  size_t picture_bound() const { return jpeg_picture_bound(hd_.n_blocks); }
  size_t record_bound() const { return jpeg::record_bytes(hd_.n_blocks, 64 * (size_t)hd_.n_blocks); }

 private:
  gtx_ctx* ctx_;
  jpeg::RecordHeader hd_{};
  uint16_t quant_[3][64];
  DevBuf d_planes_, d_quant_, d_dense_, d_lens_, d_tiles_, d_rec_;   // d_rec_: offset[n_blocks + 1], then coef[]
  uint32_t* h_total_ = nullptr;                                   // pinned: the closing offset
  hipEvent_t e0_ = nullptr, e1_ = nullptr, eh_ = nullptr;          // eh_: between the forward DCT and the entropy launches
  bool in_flight_ = false, submitted_ = false;
  float last_ms_ = 0.f, entropy_ms_ = 0.f;
  std::unique_ptr<JpegHuff> huff_;
};

}  // namespace gtx

struct gtx_jpeg_enc {
  std::unique_ptr<gtx::JpegEncoder> impl;
};
