// YOLOv9's downsampling pools (ultralytics nn.modules AConv / ADown), one launch per block. gfx950 only.
//   AConv(x) = Conv3x3s2(avg_pool2d(x, 2, 1))
//   ADown(x) = cat(Conv3x3s2(a[:, :c/2]), Conv1x1(max_pool2d(a[:, c/2:], 3, 2, 1))),  a = avg_pool2d(x, 2, 1)
// The launch writes what the convolutions read. `avg` is the (H-1) x (W-1) average stored H x W with its last row and column
// zero: the stride-2 pad-1 3x3 convolution that follows reads index H-1 only where Conv2d(3, 2, 1) on the odd-sized map reads its
// zero pad, so the even-sized stride-2 kernels consume it as it is and form the same sums. `mx` is the average followed by the
// 3x3 stride-2 max (padding excluded, as -inf), written at H/2 x W/2 without the intermediate map reaching HBM. Sums in fp32, one
// rounding where a map is stored. No value can leave fp16's range on the way (an average and a maximum stay inside their inputs'),
// so the split-f16x3 path's saturation flag is not touched.
#pragma once
#include "rtdetr_kernels.hpp"

namespace gtx {

// in [n][H][W] with avg.c + mx.c channels; avg [n][H][W] takes the first avg.c of them, mx [n][H/2][W/2] the rest (mx.c = 0 and a null
// pointer: AConv). H, W even and >= 2; channel counts, strides and offsets multiples of 8. Maps in the activation format fmt.
void launch_pool_down(int fmt, const RtMap& in, const RtMap& avg, const RtMap& mx, int n, hipStream_t s);
// what launch_pool_down would refuse, as a message (null: fine); no GPU call
const char* pool_down_refusal(int fmt, const RtMap& in, const RtMap& avg, const RtMap& mx, int n);

}  // namespace gtx
