// The box decode of a Detect layer with reg_max = 1 (yolo26.yaml): the branch's last 1x1 convolution has four outputs, the signed
// distances l, t, r, b from the anchor's cell centre in strides, and no DFL follows. Device code shared by the dense forms
// (det_kernels.hip: head_boxes_r1_kernel, head_raw_r1_kernel) and the sparse one (head_sparse.hip), so that the three form a
// candidate's box with the same operations in the same order: bit for bit the same box from the same 64 features.
#pragma once
#include <hip/hip_runtime.h>

namespace gtx {

// Output j (0..3: l, t, r, b) of the last box convolution: one fmaf chain in feature order, started from the bias. wb: [cb][4] fp32,
// bb: [4]; feat(k): box feature k of the anchor as fp32.
template <typename F>
__device__ __forceinline__ float reg1_side(F feat, int cb, const float* __restrict__ wb, const float* __restrict__ bb, int j) {
  float a = bb[j];
  for (int k = 0; k < cb; ++k) a = fmaf(feat(k), wb[k * 4 + j], a);
  return a;
}

// dist2bbox(xywh = False) * stride at anchor la of a level w cells wide: xyxy in network pixels. No clamp: a negative distance puts
// the side beyond the cell centre.
__device__ __forceinline__ float4 reg1_xyxy(float l, float t, float r, float b, int la, int w, float stride) {
  const float ax = (float)(la % w) + 0.5f, ay = (float)(la / w) + 0.5f;
  return make_float4((ax - l) * stride, (ay - t) * stride, (ax + r) * stride, (ay + b) * stride);
}

}  // namespace gtx
