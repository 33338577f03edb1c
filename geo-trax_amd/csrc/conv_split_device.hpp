// Device code and launcher shared by the split-f16x3 kernels (conv_igemm_split.hip, conv_k32_split.hip, conv_k32s2_split.hip,
// head_sparse.hip): the ONE home of their arithmetic contract. gfx950 only.
// The parity tests (the sparse box branch against the dense one, the fused front against the two launches, every form against
// the 32x32x16 kernel) hold because every kernel runs the operations below, in this order: change them here or nowhere.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <mutex>

#include "conv_igemm.hpp"

namespace gtx {

typedef float float2v __attribute__((ext_vector_type(2)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

// ---- arithmetic ----
// The epilogues work on PAIRS of values: gfx950 has packed fp32 multiply / add / fma (v_pk_mul_f32, v_pk_add_f32,
// v_pk_fma_f32: two values per lane and issue slot) and a packed fp32 -> fp16 conversion, so SiLU + the hi / lo split cost
// 8.5 vector instructions per value instead of 12.5 -- the epilogue is the VALU-bound part of a workgroup's life. Same
// operations in the same order as the scalar forms (x * rcp(1 + __expf(-x)); hi = fp16(x), lo = fp16(x - hi)): the results are
// theirs bit for bit.
__device__ __forceinline__ float2v relu2(const float2v v) { return float2v{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f)}; }   // RT-DETR's HGNetv2 blocks
__device__ __forceinline__ float2v silu2(const float2v v) {
  const float2v t = v * -1.44269504088896341f;                      // exp(-v) = exp2(-v log2 e): what __expf compiles to
  const float2v d = float2v{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)} + 1.f;
  return v * float2v{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
}
// ConvProblem::act: 0 none, 1 SiLU, 2 ReLU
__device__ __forceinline__ float2v act2(const float2v v, const int act) { return act == 1 ? silu2(v) : act == 2 ? relu2(v) : v; }
// 2 fp32 values -> their two hi halves and two lo halves (one register each); sat becomes true when a value had to be clamped
__device__ __forceinline__ void split2(const float2v v, unsigned& hi, unsigned& lo, bool& sat) {
  const float2v x = {__builtin_amdgcn_fmed3f(v.x, -65504.f, 65504.f), __builtin_amdgcn_fmed3f(v.y, -65504.f, 65504.f)};
  sat |= x.x != v.x || x.y != v.y;                                  // also true for a NaN (it is clamped to -65504 by v_med3)
  const half2v h = __builtin_convertvector(x, half2v);
  const half2v l = __builtin_convertvector(x - __builtin_convertvector(h, float2v), half2v);   // x - hi is exact in fp32
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}
// 4 fp32 values -> their 4 hi halves and 4 lo halves (8 bytes each)
__device__ __forceinline__ void split4(const float2v (&v)[2], uint2& hi, uint2& lo, bool& sat) {
  split2(v[0], hi.x, lo.x, sat);
  split2(v[1], hi.y, lo.y, sat);
}
// The accumulators start at bias / acc_scale (acc_scale is a power of two: exact), so the epilogue is one multiply and has no
// loads of its own: the bias fetch overlaps the first global -> LDS round trip instead of opening the epilogue.
__device__ __forceinline__ floatx4 acc_start(const float4 b, const float inv_sc) {
  return floatx4{b.x * inv_sc, b.y * inv_sc, b.z * inv_sc, b.w * inv_sc};
}

// ---- LDS layout ----
// 16-byte chunk swizzle of a 128-byte row (8 chunks: 4 hi, 4 lo) of a staged patch or of the packed weight image
__host__ __device__ constexpr int swz128(int row) { return (row >> 1) & 7; }
// epilogue transpose: a wave stages 32 pixels x BN channels of 4 bytes, then stores whole runs; four waves per workgroup
__host__ __device__ constexpr int epi_pitch(int bn) { return bn * 4 + 16; }     // bytes per staged pixel row
__host__ __device__ constexpr int epi_bytes(int bn) { return 4 * 32 * epi_pitch(bn); }

// ---- block decode ----
// The launch header of a ConvGroup kernel whose workgroup computes TH x TW output pixels of one cout tile. Returns false
// when this hardware block has no work; else P = its problem, ct = its cout tile, n = its image, (oy0, ox0) = its first pixel.
template <int TH, int TW>
__device__ __forceinline__ bool conv_block_decode(const ConvGroup& g, ConvProblem& P, int& ct, int& n, int& oy0, int& ox0) {
  // as one burst of scalar loads: group size and every member's first block
  const int cnt = g.count;
  int bb[kMaxGroup];
#pragma unroll
  for (int i = 0; i < kMaxGroup; ++i) bb[i] = g.p[i].block_begin;
  // XCD-aware logical block id: blocks b and b+8 share an XCD (speed only, never correctness); every XCD works through one
  // contiguous range of logical blocks -- the cout tiles of one pixel tile (same input patch) and neighbouring pixel tiles
  // (shared halo) meet in one L2 -- and the ranges hold equal work (ConvGroup::xcd_begin). Surplus blocks of the shorter
  // ranges leave here.
  const int xcd = blockIdx.x & 7;
  const int L = g.xcd_begin[xcd] + (int)(blockIdx.x >> 3);
  if (L >= g.xcd_begin[xcd + 1]) return false;
  int pi = 0;
#pragma unroll
  for (int i = 1; i < kMaxGroup; ++i)
    if (i < cnt && L >= bb[i]) pi = i;
  P = g.p[pi];                              // by value: one burst of wide scalar loads instead of a load (and a wait) per field
  const int lb = L - P.block_begin;
  ct = lb % P.n_ct;
  const int pt = lb / P.n_ct;
  const int tx = pt % P.tiles_x;
  const int t2 = pt / P.tiles_x;
  const int ty = t2 % P.tiles_y + P.ty_first;
  n = t2 / P.tiles_y;
  oy0 = ty * TH;
  ox0 = tx * TW;
  return true;
}

// ---- epilogue pieces ----
// After the MFMAs a lane holds 4 consecutive channels of one pixel, and the lane W away (W = 32: v_mfma_f32_32x32x16_f16,
// lanes l and l + 32; W = 16: v_mfma_f32_16x16x32_f16, lanes kg = 2 q and 2 q + 1) holds the other half of their 8-channel
// group. Two lane swaps turn that into the group's 16-byte hi chunk (lower lane) and 16-byte lo chunk (upper lane) of the
// pair format, at the byte offset the lane's fp32 float4 would have had.
template <int W>
__device__ __forceinline__ void lane_swap(const unsigned a, const unsigned b, unsigned& lower, unsigned& upper) {
  static_assert(W == 16 || W == 32, "v_permlane16_swap or v_permlane32_swap");
  if constexpr (W == 16) {
    const auto s = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    lower = s[0]; upper = s[1];
  } else {
    const auto s = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    lower = s[0]; upper = s[1];
  }
}
// the pixel's residual channels c0.. (pair format), or null when the launch has no residual or the pixel is outside the map
__device__ __forceinline__ const float* residual_row(const ConvProblem& P, const int n, const int oy, const int ox, const int c0) {
  if (!P.res || oy >= P.Ho || ox >= P.Wo) return nullptr;
  return static_cast<const float*>(P.res) + (((size_t)n * P.Ho + oy) * P.Wo + ox) * P.res_cstride + P.res_coff + c0;
}
// v += the residual of the lane's 4 channels; src = the lane's 16 bytes of the residual's pair row (the group's hi chunk in
// the lower lane, its lo chunk in the upper one), null = zeros. Every lane must come here (the swaps): branch on uniform values only.
template <int W>
__device__ __forceinline__ void add_residual(float2v (&v)[2], const float* src) {
  uint4 rc = make_uint4(0, 0, 0, 0);
  if (src) rc = *reinterpret_cast<const uint4*>(src);
  unsigned hw[2], lw[2];                                            // (hi, lo) of this lane's channels 0, 1 and 2, 3
  lane_swap<W>(rc.x, rc.z, hw[0], lw[0]);
  lane_swap<W>(rc.y, rc.w, hw[1], lw[1]);
  const half4 rh = *reinterpret_cast<const half4*>(hw), rl = *reinterpret_cast<const half4*>(lw);
#pragma unroll
  for (int q = 0; q < 2; ++q)                                       // hi + lo is exact in fp32
    v[q] += float2v{(float)rh[2 * q], (float)rh[2 * q + 1]} + float2v{(float)rl[2 * q], (float)rl[2 * q + 1]};
}
// the lane's 16 bytes of the pair format for its 4 values (see lane_swap); every lane must come here
template <int W>
__device__ __forceinline__ uint4 pair_chunk(const float2v (&v)[2], bool& sat) {
  uint2 hi, lo;
  split4(v, hi, lo, sat);
  uint4 c;
  lane_swap<W>(hi.x, lo.x, c.x, c.z);
  lane_swap<W>(hi.y, lo.y, c.y, c.w);
  return c;
}
// One accumulator fragment (4 channels of a pixel) through the epilogue: acc * 2^-shift (the bias is already in) ->
// activation (+ residual, res_src as add_residual's src) -> pair format, or plain fp32 (ConvProblem::out_plain: the Detect
// head's last stage, read by the decode kernels) -> the lane's 16 bytes at dst. has_res and plain are uniform.
template <int W>
__device__ __forceinline__ void epilogue_fragment(const floatx4 a, const float sc, const int act, const bool has_res, const float* res_src,
                                                  const bool plain, char* dst, bool& sat) {
  float2v v[2] = {act2(float2v{a[0], a[1]} * sc, act), act2(float2v{a[2], a[3]} * sc, act)};
  if (has_res) add_residual<W>(v, res_src);
  if (plain) *reinterpret_cast<float4*>(dst) = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
  else *reinterpret_cast<uint4*>(dst) = pair_chunk<W>(v, sat);
}
// The wave's staged rows (32 pixels = output rows py0, py0 + 1 x 16 columns from ox0, epi_pitch(BN) bytes apart) -> `out`, as
// whole BN * 4-byte runs per pixel. cvalid < BN in a last cout tile that is half empty (Cout = 16, 48, 80 ...).
template <int BN>
__device__ __forceinline__ void store_runs(const char* stg, const ConvProblem& P, const int n, const int ct, const int py0, const int ox0,
                                           const int cvalid, const int lane) {
  constexpr int LPP = BN / 4;                 // lanes per pixel (16 B each)
  constexpr int PPI = 64 / LPP;               // pixels per store instruction
#pragma unroll
  for (int it = 0; it < 32 / PPI; ++it) {
    const int p = it * PPI + lane / LPP, q = lane % LPP;
    const int py = py0 + (p >> 4), px = ox0 + (p & 15);
    const uint4 val = *reinterpret_cast<const uint4*>(stg + p * epi_pitch(BN) + q * 16);
    if (py < P.Ho && px < P.Wo && (q >> 1) * 8 < cvalid) {     // cvalid is a multiple of 16: whole groups
      float* dst = static_cast<float*>(P.out) + (((size_t)n * P.Ho + py) * P.Wo + px) * P.out_cstride + P.out_coff + ct * BN + q * 4;
      *reinterpret_cast<uint4*>(dst) = val;
    }
  }
}
// raises the launch's saturation flag (may be null) when a lane of the wave had to clamp
__device__ __forceinline__ void flag_saturation(int* flag, const bool sat, const int lane) {
  if (flag && __builtin_amdgcn_ballot_w64(sat) != 0 && lane == 0) atomicOr(flag, 1);
}
// The complete epilogue of the 16x16x32 tile (conv_k32_split.hip, conv_k32s2_split.hip): 8 x 16 pixels x 64 couts, wave w owns
// tile rows 2 w, 2 w + 1; lane (col, kg) of acc[a][m] holds couts 16 a + 4 kg + 0..3 of pixel (row 2 w + m, col) -- byte
// 64 a + 16 kg of the pixel's 256-byte run. Staged per wave in LDS (smem: the workgroup's, free after the barrier), stored as runs.
__device__ __forceinline__ void epilogue_k32(const floatx4 (&acc)[4][2], const ConvProblem& P, char* smem, const int ct, const int n,
                                             const int oy0, const int ox0, const int wave, const int lane) {
  constexpr int BN = 64, PITCH = epi_pitch(BN);
  const int col = lane & 15, kg = lane >> 4;
  const int cvalid = P.Cout - ct * BN;
  const bool plain = P.out_plain != 0, has_res = P.res != nullptr;
  bool sat = false;
  __syncthreads();                                // every wave is done with the staging buffers
  char* stg = smem + wave * (32 * PITCH);         // wave-private: its own LDS writes are ordered before its reads
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const float* __restrict__ res = residual_row(P, n, oy0 + 2 * wave + m, ox0 + col, ct * BN);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int cl = 16 * a + 4 * kg;
      epilogue_fragment<16>(acc[a][m], P.acc_scale, P.act, has_res, (res && cl < cvalid) ? res + cl : nullptr, plain,
                            stg + (16 * m + col) * PITCH + cl * 4, sat);
    }
  }
  store_runs<BN>(stg, P, n, ct, oy0 + 2 * wave, ox0, cvalid, lane);
  flag_saturation(P.sat_flag, sat, lane);
}

// ---- host: the launch of a ConvGroup kernel with `lds_bytes` of dynamic LDS (fixed per kernel for the process) ----
template <auto Kernel>
void launch_conv_group(const ConvGroup& g, const int threads, const int lds_bytes, hipStream_t stream) {
  static std::once_flag once;                     // one per kernel instantiation
  std::call_once(once, [&] {
    GTX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
  });
  hipLaunchKernelGGL(Kernel, dim3(g.grid_blocks), dim3(threads), lds_bytes, stream, g);
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
