// Device half of the JPEG frame sink (csrc/jpeg_enc.hip): packed BGR in HBM -> the packed record of jpeg_parse.hpp, which the
// host emitter (csrc/jpeg_emit.cpp) Huffman-codes into a baseline JPEG.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>

#include "common.hpp"
#include "jpeg_emit.hpp"

struct gtx_ctx;

namespace gtx {

// Blocks one workgroup of the prefix sum covers (256 lanes x 4 lengths): the tile of the multi-workgroup scan.
constexpr int kJpegScanTile = 1024;

// One encoder for frames of one size, quality and sampling: its scratch in HBM and the stream-ordered chain
// planes -> forward DCT + quantisation -> prefix sum of the block lengths -> compaction. One frame may be in flight per object.
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
  size_t record_bound() const { return jpeg::record_bytes(hd_.n_blocks, 64 * (size_t)hd_.n_blocks); }

 private:
  gtx_ctx* ctx_;
  jpeg::RecordHeader hd_{};
  uint16_t quant_[3][64];
  DevBuf d_planes_, d_quant_, d_dense_, d_lens_, d_tiles_, d_rec_;   // d_rec_: offset[n_blocks + 1], then coef[]
  uint32_t* h_total_ = nullptr;                                   // pinned: the closing offset
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
  bool in_flight_ = false;
  float last_ms_ = 0.f;
};

}  // namespace gtx

struct gtx_jpeg_enc {
  std::unique_ptr<gtx::JpegEncoder> impl;
};
