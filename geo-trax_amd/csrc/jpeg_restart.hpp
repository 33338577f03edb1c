// Device half of the JPEG frame source's restart-interval route (csrc/jpeg_restart.hip): interval plans of jpeg_parse.hpp in HBM
// (header, tables, interval starts, the clean stream) -> the packed records of jpeg_parse.hpp in HBM, byte for byte what the host
// parser writes for the same pictures. One lane decodes one restart interval; the intervals of all frames handed to one
// enqueue() share launches. jpeg_idct_kernel and jpeg_colour_kernel (csrc/jpeg.hip) run unchanged behind it.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "jpeg_parse.hpp"

struct gtx_ctx;

namespace gtx {

// Lanes of one workgroup (one wave: a frame of few intervals still spreads over several compute units) and the most frames one
// launch takes (their descriptors travel as the kernel's argument); enqueue() cuts longer batches into several launches.
constexpr int kJpegRestartLanes = 64, kJpegRestartMaxFrames = 16;
// Status of a frame (0: the record is the parser's).
constexpr uint32_t kJpegRestartInvalid = 1;

// One decoder for batches of up to max_frames interval plans of up to max_blocks blocks each: its scratch in HBM and the
// stream-ordered chain. Nothing in enqueue() waits for the device.
class JpegRestart {
 public:
  JpegRestart(gtx_ctx* ctx, int max_frames, size_t max_blocks);
  // d_plans[k]: plan k in HBM, phs[k] its header (checked with jpeg::check_plan_intervals). d_recs[k]: room for
  // record_bytes(n_blocks, 64 * n_blocks). The result words follow on the same stream: d_result(k)[0] is frame k's status.
  void enqueue(int n, const uint8_t* const* d_plans, const jpeg::PlanHeader* phs, uint8_t* const* d_recs);
  const uint32_t* d_result(int k) const { return d_state_.as<const uint32_t>() + 2 * (size_t)k; }

 private:
  gtx_ctx* ctx_;
  int max_frames_;
  size_t max_blocks_;
  DevBuf d_dense_, d_lens_, d_tiles_, d_state_;                   // [max_frames] each
};

}  // namespace gtx
