// Device half of the JPEG frame source (csrc/jpeg.hip): packed record -> u8 sample planes -> packed BGR.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "jpeg_parse.hpp"

struct gtx_ctx;

namespace gtx {
// Enqueues the two launches of one frame on ctx's stream. d_record: the record in HBM (hd is its header, already checked by
// jpeg::check_record on the host: the kernels index by its sizes); d_planes: scratch of at least jpeg::planes_bytes(hd);
// bgr: hd.height * hd.width * 3 bytes. Asynchronous. between: an event recorded between the two launches (timing), or NULL.
void jpeg_decode_launch(gtx_ctx* ctx, const void* d_record, const jpeg::RecordHeader& hd, void* d_planes, void* bgr, hipEvent_t between = nullptr);
}  // namespace gtx
