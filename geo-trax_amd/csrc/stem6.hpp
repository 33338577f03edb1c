// yolov5.yaml's stem: Conv(3, c0, k = 6, s = 2, p = 2) + bias + SiLU on the RGB0 image, the 108-tap counterpart of det_kernels.hpp's
// launch_stem. gfx950 only. Host launch wrapper and weight packers; kernels live in stem6.hip.
#pragma once
#include <vector>

#include "common.hpp"
#include "yolo_tables.hpp"

namespace gtx {

// img [n][h][w][4] RGB0 bytes (h, w >= 2), pixel value float32(v) / float32(255); out [n][ho][wo][c0] with ho = stem6_out(h), wo =
// stem6_out(w): output (oy, ox) reads image rows 2 oy - 2 .. 2 oy + 3 and columns 2 ox - 2 .. 2 ox + 3, zeros beyond the border.
// w108: [108][c0] fp32, row (ky * 6 + kx) * 3 + colour; bias: [c0] followed by zeros up to a multiple of 32 (the matrix-core kernels
// read a 32-channel group's bias unconditionally). c0 a multiple of 16, at most 96.
// dtype DT_F16: fp16 MFMA on wpk = pack_stem6_weights_f16, fp16 output; DT_F32S: split-f16x3 MFMA on wpk = pack_stem6_weights_split (hi + lo,
// scaled by a power of two whose inverse is acc_scale), pair-format output; DT_F32: exact fp32 on w108 (wpk unused), fp32 output.
void launch_stem6(int dtype, const void* img, int n, int h, int w, const float* w108, const float* bias, const void* wpk, int c0, void* out,
                  int ho, int wo, hipStream_t s, float acc_scale = 1.f);
// K = 108 padded with zero taps to 112 = 7 steps of 16: [group of 32 couts][k-step 7][lane 64][8 halves], lane (r = cout in group, hh)
// of step s holds rows 16 s + 8 hh .. + 7 of w108
std::vector<uint16_t> pack_stem6_weights_f16(const float* w108, int c0);
// [group][k-step 7][hi | lo][lane 64][8 halves], the weights scaled by the power of two that puts max |w| in [2^13, 2^14)
std::vector<uint16_t> pack_stem6_weights_split(const float* w108, int c0, float* acc_scale);

}  // namespace gtx
