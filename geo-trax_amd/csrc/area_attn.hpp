// YOLO12's map-side launches that no earlier family has (yolo_trunk.cpp's A2C2f): the area attention of ultralytics' AAttn and the
// learned per-channel residual of A2C2f(residual=True). gfx950 only. Host launch wrappers; kernels live in area_attn.hip.
#pragma once
#include "rtdetr_kernels.hpp"

namespace gtx {

// AAttn's attention on maps in the path's activation format. The h w positions of a map, row-major, are the tokens; `area` cuts them
// into that many contiguous runs of h w / area tokens (horizontal bands; h w % area == 0, else refused), and a token attends to the
// tokens of its own band only: out = softmax(q^T k * 32^-0.5) v per band and head, head width 32 for q, k and v. Scores and softmax
// in fp32, the band x band score matrix never reaches HBM.
// qkv holds 96 heads channels. planar = false: per head [q 32 | k 32 | v 32], heads consecutive (what AAttn's qkv convolution writes);
// planar = true: [q of every head | k of every head | v of every head] (the trunk permutes the convolution's rows into this order, so
// that v is a channel slice the depthwise `pe` launch reads as a map). out [N][h][w][32 heads], head-major either way.
void launch_area_attention(int fmt, const RtMap& qkv, const RtMap& out, int n, int heads, int area, bool planar, int* sat, hipStream_t s);

// out = x + gamma[c] * y per channel (A2C2f's `x + gamma * y`); the three maps have one shape, c % 8 == 0, gamma [c] fp32
void launch_scale_add(int fmt, const RtMap& y, const RtMap& x, const RtMap& out, int n, const float* gamma, int* sat, hipStream_t s);

}  // namespace gtx
