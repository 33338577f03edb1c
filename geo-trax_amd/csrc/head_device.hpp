// Device arithmetic of the Detect head's pass tail: the ONE home of every number that more than one kernel forms. gfx950.
//
// The contract: the kernels below form the same number with the same operations in the same order, so they agree bit for bit, and
// tests hold them to it. Change an operation here or nowhere.
//   class score    head_candidates_kernel (the gate) == v10_select_kernel (every class of the anchors kept): cls_scores4
//                  -- tests/test_head_ops_gpu.py (v10_select), tests/test_yolov10_gpu.py
//   16-bin box     head_boxes_kernel == head_sparse_box_kernel<false> == head_raw_kernel<T, false>: box_chain from the bias in feature
//                  order (head_boxes_kernel writes that chain out itself: through the accessors its code came out 2 % slower),
//                  dfl_xywh, xywh_to_xyxy -- tests/test_detector_gpu.py (test_sparse_box_branch_is_the_dense_one_bit_for_bit),
//                  tests/test_head_ops_gpu.py (boxes), tests/test_head_sparse_ops_gpu.py (the sparse launch on its own: float64,
//                  and the dense route's hooks bit for bit), raw_output == the rows
//   reg_max = 1    head_boxes_r1_kernel == head_sparse_box_kernel<true> == head_raw_kernel<T, true>: reg1_side, reg1_xyxy
//                  -- tests/test_yolo26_gpu.py (test_sparse_box_form_equals_the_dense_one, ..._on_every_map_corner),
//                  tests/test_head_sparse_ops_gpu.py (the same two checks for the sparse launch on its own)
//   class logits   head_raw_kernel, both forms: raw_class_row (a serial chain: the scores of raw_output are not the gate's bits)
//   frame boxes    nms_resolve_kernel == nms_small_kernel == v10_rows_kernel: undo_letterbox with letterbox_undo()'s figures
//                  -- tests/test_head_ops_gpu.py (NMS, v10_rows)
// The shuffles in cls_scores4 (16 lanes), dfl_xywh (64) and the callers of reg1_side (4) need every lane of the group active: call
// them under wave-uniform control flow (a short last group repeats its last candidate). Nothing here holds a workgroup barrier.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "det_kernels.hpp"

namespace gtx {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// ---- loads, levels ----
template <typename T> __device__ __forceinline__ float ldf(const T* p) { return (float)*p; }

template <typename T> __device__ __forceinline__ void load8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void load8<_Float16>(const _Float16* p, float (&v)[8]) {
  const half8 h = *reinterpret_cast<const half8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
}
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&v)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ int find_level(const HeadParams& hp, int a) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < kMaxLevels; ++i)
    if (i < hp.n_levels && a >= hp.lv[i].anchor_begin) l = i;
  return l;
}

// ---- class branch: final 1x1 conv (nc x cc) + sigmoid ----
// Scores of classes c0 .. c0 + 3 of one anchor by the 16 lanes (sub = 0 .. 15) that share it: each lane owns 8-channel chunks of the
// anchor's cls features fc (one fully coalesced 16-B load per lane per 128 channels), one fmaf chain per class, the partial dot
// products combined with four xor-shuffles, then bias and sigmoid. Every lane gets the scores; -1 past the last class.
template <typename T>
__device__ __forceinline__ void cls_scores4(const HeadLevel& L, const T* fc, int sub, int c0, int nc, float (&sc)[4]) {
  const int chunks = L.cc >> 3;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ch = sub; ch < chunks; ch += 16) {
    float f[8];
    load8<T>(fc + ch * 8, f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (c0 + j < nc) {
        float w[8];
        load8<float>(L.wc + (size_t)(c0 + j) * L.cc + ch * 8, w);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[j] = fmaf(f[e], w[e], acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) acc[j] += __shfl_xor(acc[j], o, 64);
    sc[j] = c0 + j < nc ? 1.f / (1.f + expf(-(acc[j] + L.bc[c0 + j]))) : -1.f;
  }
}

// The raw read-back's class columns of one anchor by its wave: lane c, c + 64, ... forms class c as one serial fmaf chain from the
// bias over the cls features fc, and stores the logit or its sigmoid at row[4 + c].
template <typename T>
__device__ __forceinline__ void raw_class_row(const HeadLevel& L, const T* fc, int nc, int lane, int logits, float* row) {
  for (int c = lane; c < nc; c += 64) {
    float acc = L.bc[c];
    for (int k = 0; k < L.cc; ++k) acc = fmaf(ldf(fc + k), L.wc[c * L.cc + k], acc);
    row[4 + c] = logits ? acc : 1.f / (1.f + expf(-acc));
  }
}

// ---- box branch, 16 DFL bins per side ----
// One output of the last box 1x1 over the features [k0, k1): an fmaf chain in feature order, continued from a (the bias at k0 = 0).
// feat(k): box feature k of the anchor as fp32 (a lane shuffle, an LDS row); weight(k): its weight for this lane's output (global,
// LDS). kUnroll: the loop's unroll count (0: the compiler's choice).
template <int kUnroll = 0, typename F, typename W>
__device__ __forceinline__ float box_chain(float a, int k0, int k1, F feat, W weight) {
  if constexpr (kUnroll > 0) {
#pragma unroll kUnroll
    for (int k = k0; k < k1; ++k) a = fmaf(feat(k), weight(k), a);
  } else {
    for (int k = k0; k < k1; ++k) a = fmaf(feat(k), weight(k), a);
  }
  return a;
}

// DFL tail: lane = side * 16 + bin of a whole wave holds one box logit of the anchor la of a level w cells wide; softmax expectation
// per side, dist2bbox(xywh = True) * stride. Returns xywh in network pixels on every lane.
__device__ __forceinline__ float4 dfl_xywh(float logit, int la, int w, float stride, int lane) {
  float m = logit;                                  // softmax over the 16 lanes of a side
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  const float e = expf(logit - m);
  float se = e, sw = e * (float)(lane & 15);
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) {
    se += __shfl_xor(se, o, 64);
    sw += __shfl_xor(sw, o, 64);
  }
  const float d = sw / se;
  const float d0 = __shfl(d, 0, 64), d1 = __shfl(d, 16, 64), d2 = __shfl(d, 32, 64), d3 = __shfl(d, 48, 64);
  const float ax = (float)(la % w) + 0.5f, ay = (float)(la / w) + 0.5f;
  const float x1 = ax - d0, y1 = ay - d1, x2 = ax + d2, y2 = ay + d3;
  return make_float4((x1 + x2) * 0.5f * stride, (y1 + y2) * 0.5f * stride, (x2 - x1) * stride, (y2 - y1) * stride);
}

__device__ __forceinline__ float4 xywh_to_xyxy(const float4 b) {
  const float hw = b.z / 2.f, hh = b.w / 2.f;
  return make_float4(b.x - hw, b.y - hh, b.x + hw, b.y + hh);
}

// ---- box branch, reg_max = 1 (yolo26.yaml): the last 1x1 has four outputs, the signed distances l, t, r, b from the anchor's cell
// centre in strides, and no DFL follows ----
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

// ---- network pixels -> frame pixels: ultralytics scale_boxes + clip_boxes ----
struct LetterboxUndo {
  float gain, padx, pady;   // scale_boxes: gain = min ratio, pad = round((net - src * gain) / 2 - 0.1)
  float fw, fh;             // the frame
};
inline LetterboxUndo letterbox_undo(const Letterbox& lb) {
  return {(float)lb.gain, (float)std::nearbyint((lb.net_w - lb.src_w * lb.gain) / 2 - 0.1),
          (float)std::nearbyint((lb.net_h - lb.src_h * lb.gain) / 2 - 0.1), (float)lb.src_w, (float)lb.src_h};
}
// in place, on the kernels' own float arguments: the form that leaves the three kernels' code as it was
__device__ __forceinline__ void undo_letterbox(float4& b, float gain, float padx, float pady, float fw, float fh) {
  b.x = (b.x - padx) / gain; b.y = (b.y - pady) / gain;
  b.z = (b.z - padx) / gain; b.w = (b.w - pady) / gain;
  b.x = fminf(fmaxf(b.x, 0.f), fw); b.z = fminf(fmaxf(b.z, 0.f), fw);
  b.y = fminf(fmaxf(b.y, 0.f), fh); b.w = fminf(fmaxf(b.w, 0.f), fh);
}

}  // namespace gtx
