// Device half of the JPEG frame source's GPU entropy route (csrc/jpeg_entropy.hip): the plan of jpeg_parse.hpp in HBM (header,
// tables, the unstuffed entropy-coded segment) -> the packed record of jpeg_parse.hpp in HBM, byte for byte what the host parser
// writes for the same picture. jpeg_idct_kernel and jpeg_colour_kernel (csrc/jpeg.hip) run unchanged behind it.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "jpeg_parse.hpp"

struct gtx_ctx;

namespace gtx {

// Bits of the clean stream one lane owns (a subsequence). The supported set; 0 in an interface means the production choice.
constexpr int kJpegEntropySubBits = 1024;
inline bool jpeg_entropy_sub_bits_ok(int s) { return s == 256 || s == 512 || s == 1024 || s == 2048; }
// Lanes of one workgroup: its span of the stream (lanes * sub_bits / 8 bytes, at most 32 KB) is staged in LDS.
inline int jpeg_entropy_lanes(int sub_bits) { return sub_bits == 2048 ? 128 : 256; }
// Synchronisation rounds across workgroups that are enqueued (round 0 included): production choice, and the most a caller may ask for.
constexpr int kJpegEntropyRounds = 8, kJpegEntropyMaxRounds = 64;
// Status bits of a frame (0: the record is the parser's).
constexpr uint32_t kJpegEntropyInvalid = 1, kJpegEntropyNotConverged = 2;

// One decoder for plans of up to max_blocks blocks and max_stream_bytes of clean stream, cut at min_sub_bits or more: its scratch in
// HBM and the stream-ordered chain. Nothing in enqueue() waits for the device.
class JpegEntropy {
 public:
  JpegEntropy(gtx_ctx* ctx, size_t max_blocks, size_t max_stream_bytes, int min_sub_bits);
  // d_plan: the plan in HBM, ph its header (checked with jpeg::check_plan). d_rec: room for record_bytes(n_blocks, 64 * n_blocks).
  // The result words follow on the same stream: d_result()[0] status, [1] rounds used.
  void enqueue(const uint8_t* d_plan, const jpeg::PlanHeader& ph, int sub_bits, int rounds, uint8_t* d_rec);
  const uint32_t* d_result() const { return d_state_.as<const uint32_t>(); }
  // The header the two pixel kernels take by value for a plan's record: n_coef is the buffer's bound, not the real count.
  static jpeg::RecordHeader record_header(const jpeg::PlanHeader& ph);
  // jpeg_entropy_pack_kernel alone, the closing launch of both GPU entropy routes: dense runs + the record's offsets -> coef[],
  // header and quantisers (d_plan: a plan of either format). d_state: 2 words or more, [1] receives the rounds used.
  static void pack_launch(hipStream_t s, const uint8_t* d_plan, const jpeg::RecordHeader& hd, const int16_t* d_dense, uint8_t* d_rec, int rounds, uint32_t* d_state);

 private:
  gtx_ctx* ctx_;
  size_t max_blocks_, max_lanes_, max_stream_bytes_;
  int min_sub_bits_;
  DevBuf d_entry_, d_exit_, d_count_, d_blockoff_, d_edge_, d_lane_tiles_, d_state_;
  DevBuf d_dense_, d_aclen_, d_lens_, d_dcvals_, d_dcpref_, d_block_tiles_;
};

}  // namespace gtx
