// What the operator hooks (gtx_op_*: gtx_ops.cpp, and the hooks that sit beside their file-local kernels in gmc.hip,
// stabilizer.hip and homography.hip) share: refusing an argument, staging host arrays into fresh device buffers and back, the step between plain fp32
// host arrays and the pair format (split_format.hpp), and the event-timed launch loop. Host only, synchronous copies: none of
// this is on the product's path.
#pragma once
#include <algorithm>
#include <vector>

#include "../../include/gtx.h"
#include "common.hpp"
#include "split_format.hpp"

namespace gtx {

[[noreturn]] inline void op_bad(const char* op, const char* what) { fail(GTX_ERR_INVALID, "%s: %s", op, what); }

// d becomes a fresh buffer of max(room, bytes) bytes whose first `bytes` are src's (bytes == 0: src may be null)
inline void upload(DevBuf& d, const void* src, size_t bytes, size_t room = 0) {
  d.alloc(std::max(room, bytes));
  if (bytes) GTX_HIP(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
}

// d becomes a fresh buffer of `bytes` bytes, every byte of the allocation 0 / 0xFF
inline void zeros(DevBuf& d, size_t bytes) {
  d.alloc(bytes);
  GTX_HIP(hipMemset(d.p, 0, d.bytes));
}
inline void fill_ff(DevBuf& d, size_t bytes) {
  d.alloc(bytes);
  GTX_HIP(hipMemset(d.p, 0xFF, d.bytes));
}

inline void download(void* host, const DevBuf& d, size_t bytes) { GTX_HIP(hipMemcpy(host, d.p, bytes, hipMemcpyDeviceToHost)); }

// upload / download of an array that is plain fp32 on the host and, for GTX_F32S, in the pair format on the device
inline void upload_fmt(DevBuf& d, int fmt, const void* host, size_t bytes) {
  if (fmt != GTX_F32S) return upload(d, host, bytes);
  std::vector<uint8_t> tmp(bytes);
  f32_to_pairs(static_cast<const float*>(host), tmp.data(), bytes / 4);
  upload(d, tmp.data(), bytes);
}
inline void download_fmt(void* host, int fmt, const DevBuf& d, size_t bytes) {
  if (fmt != GTX_F32S) return download(host, d, bytes);
  std::vector<uint8_t> tmp(bytes);
  download(tmp.data(), d, bytes);
  pairs_to_f32(tmp.data(), static_cast<float*>(host), bytes / 4);
}

// Milliseconds per launch of once() on s: 3 warm-up launches, then `iters` of them between two events. The events are destroyed
// on every path out.
template <typename F>
float time_launches(hipStream_t s, int iters, F once) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float ms = 0.f;
  try {
    GTX_HIP(hipEventCreate(&e0));
    GTX_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) once();
    GTX_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) once();
    GTX_HIP(hipEventRecord(e1, s));
    GTX_HIP(hipStreamSynchronize(s));
    GTX_HIP(hipEventElapsedTime(&ms, e0, e1));
  } catch (...) {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    throw;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  return ms / iters;
}

}  // namespace gtx
