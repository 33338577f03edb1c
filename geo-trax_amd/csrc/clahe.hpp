// cv2.createCLAHE(2.0, (8, 8)).apply on the GPU (clahe.hip): what stabilo's `clahe: true` runs on the working gray image.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct gtx_ctx;

namespace gtx {
// on a u8 image in HBM (src == dst allowed); luts: kClaheLutBytes of scratch.
constexpr int kClaheLutBytes = 8 * 8 * 256;
void clahe_dev(const uint8_t* src, int h, int w, uint8_t* luts, uint8_t* dst, hipStream_t s);
// host image in / out (exposed for tests / tools: gtx_op_clahe).
void clahe_image(gtx_ctx* ctx, const uint8_t* gray, int h, int w, uint8_t* out);
}  // namespace gtx
