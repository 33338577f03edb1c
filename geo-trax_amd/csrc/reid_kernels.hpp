// Kernels of the separate ReID network (reid.cpp): the batched crop + resample that writes the classification backbone's input,
// and the global average pool that turns its last map into one vector per crop. gfx950 only.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace gtx {

// One crop of a pass. The crop is frame[y0:y0+ch, x0:x0+cw] of frame `frame` of the batch; it is resampled to the short-side-S
// size (PIL bilinear, reid.cpp reid_resample_coeffs) and only the S x S center window is computed. Bounds and fixed-point
// coefficients live in an int pool: bounds [S][2] (first source index relative to the crop, tap count) and coefficients [S][k].
struct ReidCrop {
  int frame;
  int x0, y0, cw, ch;
  int bh, hoff, kh;     // horizontal: bounds offset, coefficient offset, coefficients per output column
  int bv, voff, kv;     // vertical: the same per output row
};

// frames: [nb][h][w][3] BGR u8 (device); out: [n][S][S][4] u8, channel slots (B, G, R, 0): the byte image launch_stem reads,
// with the network's input channel c in slot c (the classifier sees the frame's BGR order, reid.cpp kNetChannelsBgr).
void launch_reid_crop(const uint8_t* frames, int h, int w, const ReidCrop* crops, const int* pool, int n, int S, void* out, hipStream_t s);

// mean over the hw pixels of every (crop, channel) of an NHWC map: fmt 0 = fp32, 1 = the pair format (split_format.hpp);
// out [n][c] fp32. The pixels are summed in raster order, one thread per (crop, channel).
void launch_reid_pool(const void* in, int fmt, int n, int hw, int cstride, int coff, int c, float* out, hipStream_t s);

}  // namespace gtx
