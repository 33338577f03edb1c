// 3x3 stride-2 split-f16x3 convolution on v_mfma_f32_16x16x32_f16 ("K32 stride-2 form", ConvForm::K32S2). gfx950 only.
//
// conv_k32_split.hip's arithmetic contract and workgroup (conv_split_device.hpp: pair-format activations, three fp16 MFMAs per
// product -- small terms first --, fp32 accumulation, the packed weight image with 32-channel chunks, epilogue_k32,
// conv_block_decode): 8 x 16 output pixels x 64 couts per 4-wave workgroup, wave w owns tile rows 2w, 2w + 1 and all four 16-cout
// blocks, B fragments read one tap ahead and A fragments one block ahead.
//
// Staging. A chunk's whole patch is 17 x 33 pixels x 128 B = 71.8 KB: beside a kernel row of weights (24.6 KB) one workgroup per
// CU. But kernel rows 0 and 2 read the ODD patch rows only (input rows 2 oy - 1 and 2 oy + 1: nine of them, row r + ky / 2 for
// tile row r) and kernel row 1 the eight EVEN ones, so a chunk runs as three stages over ONE 9-row buffer:
//   stage 0: odd rows + weight row 0 -> taps (0, kx)      stage 1: weight row 2 -> taps (2, kx), one buffer row further down
//   stage 2: even rows + weight row 1 -> taps (1, kx)
// Every input pixel and every weight is fetched once per chunk, as in the whole-patch form; only the order of the sum differs
// (kernel rows 0, 2, 1). A buffer row keeps its 33 pixels as two column planes, 17 even patch columns then 16 odd ones: tap kx
// of output column c is patch column 2 c + kx = plane kx & 1, entry c + kx / 2, so the 16 lanes of a fragment read 16
// consecutive 128-byte rows -- the stride-1 kernel's conflict-free ds_read_b128 pattern under the same swz128 swizzle (with the
// pixels in column order they would be 256 B apart: a two-way bank conflict on every read).
//
// LDS: 9 x 33 x 128 B = 38 016 B patch + 24 576 B weight row = 62 592 B per workgroup, two workgroups per CU (125 184 of
// 163 840 B). Registers: 200 VGPRs of the 256 that two waves per SIMD leave (five patch prefetch slots of 8 registers, six weight
// slots of 4, 32 accumulator and 48 fragment registers), no spills.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "conv_split_device.hpp"

namespace gtx {

namespace {

#define GTXS_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)

struct K32S2Tile {
  static constexpr int TH = 8, TW = 16, BN = 64, KC = 32, CPR = 4, NCH = 8, RB = 128;
  static constexpr int PROWS = TH + 1;                            // odd stage: 9 rows; even stage: 8 (the last one is zero-filled)
  static constexpr int PW = 2 * TW + 1, NEVEN = TW + 1;           // 33 patch columns: 17 even ones, then the 16 odd ones
  static constexpr int NPIX = PROWS * PW;
  static constexpr int PATCH_UNITS = NPIX * CPR;                  // one unit = 8 channels of one pixel (hi chunk, lo chunk)
  static constexpr int PATCH_SLOTS = (PATCH_UNITS + 255) / 256;   // 5
  static constexpr int PATCH_BYTES = NPIX * RB;
  static constexpr int WROW_CHUNKS = 3 * BN * NCH;                // 16-byte chunks of one kernel row of weights: 1536
  static constexpr int W_SLOTS = WROW_CHUNKS / 256;               // 6
  static constexpr int WROW_BYTES = WROW_CHUNKS * 16;
  static constexpr int STAGE_BYTES = PATCH_BYTES + WROW_BYTES;
  static constexpr int LDS_BYTES = STAGE_BYTES > epi_bytes(BN) ? STAGE_BYTES : epi_bytes(BN);
};
static_assert(2 * K32S2Tile::LDS_BYTES <= 160 * 1024, "two workgroups per CU");

__global__ __attribute__((amdgpu_flat_work_group_size(1, 256), amdgpu_waves_per_eu(2)))
void conv_k32s2_split_kernel(const ConvGroup g) {
  using Tile = K32S2Tile;
  constexpr int PW = Tile::PW, RB = Tile::RB, BN = Tile::BN, CPR = Tile::CPR;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* lds_patch = smem;
  char* lds_w = smem + Tile::PATCH_BYTES;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  ConvProblem P;                                   // launch header: conv_split_device.hpp
  int ct, n, oy0, ox0;
  if (!conv_block_decode<Tile::TH, Tile::TW>(g, P, ct, n, oy0, ox0)) return;
  const int iy0 = 2 * oy0 - 1, ix0 = 2 * ox0 - 1;  // the patch's first (odd-stage) row and first column

  const float* __restrict__ in = static_cast<const float*>(P.in);
  const int nchunks = P.Cin / Tile::KC;

  // Unit qid = (buffer pixel p, 8-channel group c); p = 33 row + plane entry. Buffer row `row` holds input row iy0 + 2 row in the
  // odd stage and iy0 + 1 + 2 row in the even one (rows 0..7; row 8 is stored as zeros there and never read).
  int goff_o[Tile::PATCH_SLOTS], goff_e[Tile::PATCH_SLOTS];   // element offset of the unit (activation buffers are < 2^31 elements), -1 = zero fill
  int loff[Tile::PATCH_SLOTS];                    // LDS byte offset of the unit's hi chunk (-1 = unused slot); its lo chunk: ^ 64
#pragma unroll
  for (int s = 0; s < Tile::PATCH_SLOTS; ++s) {
    const int qid = tid + 256 * s;
    const int p = qid / CPR, c = qid % CPR;
    const int row = p / PW, e = p - row * PW;
    const int px = e < Tile::NEVEN ? 2 * e : 2 * (e - Tile::NEVEN) + 1;
    const int ix = ix0 + px, iyo = iy0 + 2 * row, iye = iyo + 1;
    const bool used = qid < Tile::PATCH_UNITS;
    const bool xin = used && ix >= 0 && ix < P.W;
    goff_o[s] = xin && iyo >= 0 && iyo < P.H ? ((n * P.H + iyo) * P.W + ix) * P.in_cstride + P.in_coff + c * 8 : -1;
    goff_e[s] = xin && row < Tile::TH && iye < P.H ? ((n * P.H + iye) * P.W + ix) * P.in_cstride + P.in_coff + c * 8 : -1;   // iye >= 0 always
    loff[s] = used ? p * RB + ((c ^ swz128(p)) << 4) : -1;
  }
  // packed image: [cout tile][chunk][tap = 3 ky + kx][n][8 swizzled 16-byte chunks] (pack_conv_weights_split, kc = 32): a kernel
  // row of a chunk is 1536 contiguous uint4
  const uint4* __restrict__ wsrc = reinterpret_cast<const uint4*>(P.wpack) + (size_t)ct * nchunks * (3 * Tile::WROW_CHUNKS) + tid;

  const int col = lane & 15, kg = lane >> 4;
  const int p0 = (2 * wave) * PW + col;            // buffer pixel of (tile row 2 wave, column col) at tap column 0, buffer row offset 0

  uint4 pre_a[Tile::PATCH_SLOTS], pre_b[Tile::PATCH_SLOTS];
  uint4 pw0, pw1, pw2, pw3, pw4, pw5;               // the next kernel row of weights (W_SLOTS = 6)
  static_assert(Tile::W_SLOTS == 6, "six weight slots");
#define GTXS_PREFETCH_PATCH(GOFF, CHUNK)                                                     \
  {                                                                                          \
    const int c0__ = (CHUNK) * Tile::KC;                                                     \
    _Pragma("unroll") for (int s = 0; s < Tile::PATCH_SLOTS; ++s) {                          \
      uint4 va__ = make_uint4(0, 0, 0, 0), vb__ = make_uint4(0, 0, 0, 0);                    \
      if (GOFF[s] >= 0) {                                                                    \
        const uint4* src__ = reinterpret_cast<const uint4*>(in + GOFF[s] + c0__);            \
        va__ = src__[0];                                                                     \
        vb__ = src__[1];                                                                     \
      }                                                                                      \
      pre_a[s] = va__;                                                                       \
      pre_b[s] = vb__;                                                                       \
    }                                                                                        \
  }
#define GTXS_PREFETCH_W(ROWIDX)                      /* ROWIDX = 3 chunk + kernel row */      \
  {                                                                                          \
    const uint4* w__ = wsrc + (size_t)(ROWIDX) * Tile::WROW_CHUNKS;                          \
    pw0 = w__[0]; pw1 = w__[256]; pw2 = w__[512]; pw3 = w__[768]; pw4 = w__[1024]; pw5 = w__[1280]; \
  }
#define GTXS_COMMIT_PATCH()                                                                  \
  {                                                                                          \
    _Pragma("unroll") for (int s = 0; s < Tile::PATCH_SLOTS; ++s) {                          \
      if (loff[s] >= 0) {                                                                    \
        *reinterpret_cast<uint4*>(lds_patch + loff[s]) = pre_a[s];                           \
        *reinterpret_cast<uint4*>(lds_patch + (loff[s] ^ (CPR << 4))) = pre_b[s];            \
      }                                                                                      \
    }                                                                                        \
  }
#define GTXS_COMMIT_W()                                                                      \
  {                                                                                          \
    uint4* d__ = reinterpret_cast<uint4*>(lds_w) + tid;                                      \
    d__[0] = pw0; d__[256] = pw1; d__[512] = pw2; d__[768] = pw3; d__[1024] = pw4; d__[1280] = pw5; \
  }

  GTXS_PREFETCH_PATCH(goff_o, 0)
  GTXS_PREFETCH_W(0)

  // accumulators start at bias / acc_scale: lane (col, kg) of block a holds couts 16 a + 4 kg + 0..3
  floatx4 acc[4][2];                             // [cout block a][pixel block m]
  {
    const float inv_sc = __builtin_amdgcn_rcpf(P.acc_scale);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
      if (P.bias) b = *reinterpret_cast<const float4*>(P.bias + ct * BN + 16 * a + 4 * kg);
#pragma unroll
      for (int m = 0; m < 2; ++m) acc[a][m] = acc_start(b, inv_sc);
    }
  }

  half8 bh[2][2], bl[2][2];                      // [slot][pixel block m]
  half8 ah[2], al[2];                            // [slot]
  // pixels' fragments of tap column KX, buffer row offset DR (0; 1 = kernel row 2) -> slot; piece Q = 0..3 is one 16-byte read
  // (m = Q >> 1, hi / lo = Q & 1). Tap column 0: even plane entry col, 1: odd plane entry col, 2: even plane entry col + 1.
#define GTXS_LOAD_B(DR, KX, SLOT, Q)                                                           \
    {                                                                                          \
      const int p__ = p0 + (((Q) >> 1) + (DR)) * PW + ((KX) == 1 ? Tile::NEVEN : (KX) >> 1);   \
      const char* pr__ = lds_patch + p__ * RB;                                                 \
      if (((Q) & 1) == 0) bh[SLOT][(Q) >> 1] = *reinterpret_cast<const half8*>(pr__ + ((kg ^ swz128(p__)) << 4)); \
      else bl[SLOT][(Q) >> 1] = *reinterpret_cast<const half8*>(pr__ + (((CPR + kg) ^ swz128(p__)) << 4)); \
    }
  // weights' fragments of (tap column KX, cout block A) -> slot
#define GTXS_LOAD_A(KX, A, SLOT)                                                               \
    {                                                                                          \
      const int nrow__ = 16 * (A) + col;                                                       \
      const char* wr__ = lds_w + ((KX) * BN + nrow__) * RB;                                    \
      ah[SLOT] = *reinterpret_cast<const half8*>(wr__ + ((kg ^ swz128(nrow__)) << 4));         \
      al[SLOT] = *reinterpret_cast<const half8*>(wr__ + (((CPR + kg) ^ swz128(nrow__)) << 4)); \
    }
  // One stage = 12 units (tap column kx, cout block a) of 6 MFMAs; unit u reads the weights of unit u + 1 and one piece of the
  // next tap's pixels. The B slot alternates from tap to tap through the stages (stage ST, tap kx: slot (3 ST + kx) & 1).
  // NEXT_DR >= 0: the stage after this one reads the same buffer NEXT_DR rows down, and its first tap is read here too.
#define GTXS_UNIT(ST, DR, U, NEXT_DR)                                                          \
    {                                                                                          \
      constexpr int kx__ = (U) / 4, a__ = (U) % 4;                                             \
      constexpr int bs__ = ((ST) * 3 + kx__) & 1;                                              \
      __builtin_amdgcn_sched_barrier(0);                                                       \
      if ((U) + 1 < 12) GTXS_LOAD_A(((U) + 1) / 4, ((U) + 1) % 4, ((U) + 1) & 1)               \
      if (kx__ < 2) GTXS_LOAD_B(DR, kx__ + 1, bs__ ^ 1, a__)                                   \
      else if ((NEXT_DR) >= 0) GTXS_LOAD_B((NEXT_DR) < 0 ? 0 : (NEXT_DR), 0, bs__ ^ 1, a__)    \
      acc[a__][0] = GTXS_MFMA(al[(U) & 1], bh[bs__][0], acc[a__][0]);                          \
      acc[a__][1] = GTXS_MFMA(al[(U) & 1], bh[bs__][1], acc[a__][1]);                          \
      acc[a__][0] = GTXS_MFMA(ah[(U) & 1], bl[bs__][0], acc[a__][0]);                          \
      acc[a__][1] = GTXS_MFMA(ah[(U) & 1], bl[bs__][1], acc[a__][1]);                          \
      acc[a__][0] = GTXS_MFMA(ah[(U) & 1], bh[bs__][0], acc[a__][0]);                          \
      acc[a__][1] = GTXS_MFMA(ah[(U) & 1], bh[bs__][1], acc[a__][1]);                          \
      _Pragma("unroll") for (int i__ = 0; i__ < 3; ++i__) {                                    \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                     \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
      }                                                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                       \
    }
#define GTXS_STAGE(ST, DR, NEXT_DR)                                                            \
    GTXS_LOAD_A(0, 0, 0)                                                                       \
    GTXS_UNIT(ST, DR, 0, NEXT_DR) GTXS_UNIT(ST, DR, 1, NEXT_DR) GTXS_UNIT(ST, DR, 2, NEXT_DR) GTXS_UNIT(ST, DR, 3, NEXT_DR)   \
    GTXS_UNIT(ST, DR, 4, NEXT_DR) GTXS_UNIT(ST, DR, 5, NEXT_DR) GTXS_UNIT(ST, DR, 6, NEXT_DR) GTXS_UNIT(ST, DR, 7, NEXT_DR)   \
    GTXS_UNIT(ST, DR, 8, NEXT_DR) GTXS_UNIT(ST, DR, 9, NEXT_DR) GTXS_UNIT(ST, DR, 10, NEXT_DR) GTXS_UNIT(ST, DR, 11, NEXT_DR)

  for (int chunk = 0; chunk < nchunks; ++chunk) {
    // ---- stage 0: the odd rows + kernel row 0 ----
    __syncthreads();                               // the previous chunk's fragment reads are done
    GTXS_COMMIT_PATCH()
    GTXS_COMMIT_W()
    __syncthreads();
    GTXS_PREFETCH_W(3 * chunk + 2)
    GTXS_LOAD_B(0, 0, 0, 0) GTXS_LOAD_B(0, 0, 0, 1) GTXS_LOAD_B(0, 0, 0, 2) GTXS_LOAD_B(0, 0, 0, 3)
    GTXS_STAGE(0, 0, 1)
    // ---- stage 1: kernel row 2 on the same rows, one further down; the even rows are requested here ----
    __syncthreads();
    GTXS_COMMIT_W()
    __syncthreads();
    GTXS_PREFETCH_PATCH(goff_e, chunk)
    GTXS_PREFETCH_W(3 * chunk + 1)
    GTXS_STAGE(1, 1, -1)
    // ---- stage 2: the even rows + kernel row 1; the next chunk's odd rows and first weight row are requested here ----
    __syncthreads();
    GTXS_COMMIT_PATCH()
    GTXS_COMMIT_W()
    __syncthreads();
    if (chunk + 1 < nchunks) {
      GTXS_PREFETCH_PATCH(goff_o, chunk + 1)
      GTXS_PREFETCH_W(3 * chunk + 3)
    }
    GTXS_LOAD_B(0, 0, 0, 0) GTXS_LOAD_B(0, 0, 0, 1) GTXS_LOAD_B(0, 0, 0, 2) GTXS_LOAD_B(0, 0, 0, 3)
    GTXS_STAGE(2, 0, -1)
  }
#undef GTXS_STAGE
#undef GTXS_UNIT
#undef GTXS_LOAD_A
#undef GTXS_LOAD_B

  // ---- epilogue: acc * 2^-shift -> activation (+ residual) -> split -> NHWC pair format (conv_split_device.hpp) ----
  epilogue_k32(acc, P, smem, ct, n, oy0, ox0, wave, lane);
}

}  // namespace

void conv_k32s2_launch(const ConvGroup& g, const ConvConfig& c, hipStream_t stream) {
  GTX_CHECK(c.ks == 3 && c.stride == 2 && c.bn == K32S2Tile::BN && c.kc == K32S2Tile::KC && c.th == 8,
            "conv (K32 stride-2 form): 3x3 stride 2, 64-cout tiles, 32-channel chunks (ks=%d stride=%d bn=%d kc=%d)", c.ks, c.stride, c.bn, c.kc);
  for (int i = 0; i < g.count; ++i)
    GTX_CHECK(g.p[i].Cin % K32S2Tile::KC == 0 && g.p[i].post_w == nullptr && g.p[i].front_img == nullptr && g.p[i].c_split == 0,
              "conv (K32 stride-2 form): Cin %d must be a multiple of 32 and the launch a plain 3x3 layer", g.p[i].Cin);
  launch_conv_group<conv_k32s2_split_kernel>(g, 256, K32S2Tile::LDS_BYTES, stream);
}

}  // namespace gtx
