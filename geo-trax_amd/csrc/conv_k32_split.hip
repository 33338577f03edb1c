// 3x3 stride-1 split-f16x3 convolution on v_mfma_f32_16x16x32_f16 ("K32 form", ConvForm::K32). gfx950 only.
//
// Same arithmetic contract as conv_igemm_split.hip, kept in conv_split_device.hpp (pair-format activations, every product as three fp16 MFMAs -- small terms
// first -- with fp32 accumulation, weights scaled by an exact power of two, same packed weight image with 32-channel chunks),
// the other matrix instruction: K = 32 per issue on a 16 x 16 tile. The chip holds a higher clock under that shape
// (MI355X_MICROARCH.md, "DVFS give-back": 1.12-1.15 x the FLOP/s of 32x32x16 at equal cycles per FLOP); a timing-only swap
// inside the 32x32x16 kernel priced it at 8 % on the matrix-bound layers (profiles/HISTORY.md section 8).
//
// K = 32 does not divide a tap's 16 staged channels, so a K chunk here is 32 input channels and a kernel ROW of the weights
// (3 taps x 64 couts x 128 B = 24.6 KB) is staged at a time beside the chunk's patch (10 x 18 pixels x 128 B = 23 KB):
// 47.6 KB per workgroup, three per CU like the 32x32x16 kernel. A workgroup = 8 x 16 output pixels x 64 couts; wave w owns
// tile rows 2w, 2w + 1 = two 16-pixel B blocks, and all four 16-cout A blocks: 8 accumulators of 4 registers.
// Fragment registers are the budget (3 waves per SIMD = 168 registers): the pixels' fragments (B) are held per tap and read one
// tap ahead, the weights' (A) per 16-cout block and read one block ahead -- 3 ds_read_b128 per 6 MFMAs, the 32x32x16 kernel's ratio.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "conv_split_device.hpp"

namespace gtx {

namespace {

#define GTXK_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)

struct K32Tile {
  static constexpr int TH = 8, TW = 16, BN = 64, KC = 32, CPR = 4, NCH = 8, RB = 128;
  static constexpr int PH = TH + 2, PW = TW + 2, NPIX = PH * PW;
  static constexpr int PATCH_UNITS = NPIX * CPR;                  // one unit = 8 channels of one pixel (hi chunk, lo chunk)
  static constexpr int PATCH_SLOTS = (PATCH_UNITS + 255) / 256;   // 3
  static constexpr int PATCH_BYTES = NPIX * RB;
  static constexpr int WROW_CHUNKS = 3 * BN * NCH;                // 16-byte chunks of one kernel row of weights: 1536
  static constexpr int W_SLOTS = WROW_CHUNKS / 256;               // 6
  static constexpr int WROW_BYTES = WROW_CHUNKS * 16;
  static constexpr int STAGE_BYTES = PATCH_BYTES + WROW_BYTES;
  static constexpr int LDS_BYTES = STAGE_BYTES > epi_bytes(BN) ? STAGE_BYTES : epi_bytes(BN);
};
static_assert(3 * K32Tile::LDS_BYTES <= 160 * 1024, "three workgroups per CU");

__global__ __attribute__((amdgpu_flat_work_group_size(1, 256), amdgpu_waves_per_eu(3)))
void conv_k32_split_kernel(const ConvGroup g) {
  using Tile = K32Tile;
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
  const int iy0 = oy0 - 1, ix0 = ox0 - 1;

  const float* __restrict__ in = static_cast<const float*>(P.in);
  const int nchunks = P.Cin / Tile::KC;

  int goff[Tile::PATCH_SLOTS];                    // element offset of the unit (activation buffers are < 2^31 elements), -1 = zero fill
  int loff[Tile::PATCH_SLOTS];                    // LDS byte offset of the unit's hi chunk (-1 = unused slot); its lo chunk: ^ 64
#pragma unroll
  for (int s = 0; s < Tile::PATCH_SLOTS; ++s) {
    const int qid = tid + 256 * s;
    const int p = qid / CPR, c = qid % CPR;
    const int py = p / PW, px = p - py * PW;
    const int iy = iy0 + py, ix = ix0 + px;
    const bool used = qid < Tile::PATCH_UNITS;
    const bool inb = used && iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
    goff[s] = inb ? ((n * P.H + iy) * P.W + ix) * P.in_cstride + P.in_coff + c * 8 : -1;
    loff[s] = used ? p * RB + ((c ^ swz128(p)) << 4) : -1;
  }
  // packed image: [cout tile][chunk][tap = 3 ky + kx][n][8 swizzled 16-byte chunks] (pack_conv_weights_split, kc = 32): a kernel
  // row of a chunk is 1536 contiguous uint4
  const uint4* __restrict__ wsrc = reinterpret_cast<const uint4*>(P.wpack) + (size_t)ct * nchunks * (3 * Tile::WROW_CHUNKS) + tid;

  const int col = lane & 15, kg = lane >> 4;
  const int p0 = (2 * wave) * PW + col;            // patch pixel of (tile row 2 wave, column col) at tap (0, 0)

  uint4 pre_a[Tile::PATCH_SLOTS], pre_b[Tile::PATCH_SLOTS];
  uint4 pw0, pw1, pw2, pw3, pw4, pw5;               // the next kernel row of weights (W_SLOTS = 6)
  static_assert(Tile::W_SLOTS == 6, "six weight slots");
#define GTXK_PREFETCH_PATCH(CHUNK)                                                           \
  {                                                                                          \
    const int c0__ = (CHUNK) * Tile::KC;                                                     \
    _Pragma("unroll") for (int s = 0; s < Tile::PATCH_SLOTS; ++s) {                          \
      uint4 va__ = make_uint4(0, 0, 0, 0), vb__ = make_uint4(0, 0, 0, 0);                    \
      if (goff[s] >= 0) {                                                                    \
        const uint4* src__ = reinterpret_cast<const uint4*>(in + goff[s] + c0__);            \
        va__ = src__[0];                                                                     \
        vb__ = src__[1];                                                                     \
      }                                                                                      \
      pre_a[s] = va__;                                                                       \
      pre_b[s] = vb__;                                                                       \
    }                                                                                        \
  }
#define GTXK_PREFETCH_W(ROWIDX)                      /* ROWIDX = 3 chunk + kernel row */      \
  {                                                                                          \
    const uint4* w__ = wsrc + (size_t)(ROWIDX) * Tile::WROW_CHUNKS;                          \
    pw0 = w__[0]; pw1 = w__[256]; pw2 = w__[512]; pw3 = w__[768]; pw4 = w__[1024]; pw5 = w__[1280]; \
  }
#define GTXK_COMMIT_PATCH()                                                                  \
  {                                                                                          \
    _Pragma("unroll") for (int s = 0; s < Tile::PATCH_SLOTS; ++s) {                          \
      if (loff[s] >= 0) {                                                                    \
        *reinterpret_cast<uint4*>(lds_patch + loff[s]) = pre_a[s];                           \
        *reinterpret_cast<uint4*>(lds_patch + (loff[s] ^ (CPR << 4))) = pre_b[s];                           \
      }                                                                                      \
    }                                                                                        \
  }
#define GTXK_COMMIT_W()                                                                      \
  {                                                                                          \
    uint4* d__ = reinterpret_cast<uint4*>(lds_w) + tid;                                      \
    d__[0] = pw0; d__[256] = pw1; d__[512] = pw2; d__[768] = pw3; d__[1024] = pw4; d__[1280] = pw5; \
  }

  GTXK_PREFETCH_PATCH(0)
  GTXK_PREFETCH_W(0)

  // accumulators start at bias / acc_scale: lane (col, kg) of block a holds couts 16 a + 4 kg + 0..3. (The loop is the kernel's own:
  // as a shared function that fills the array it costs conv_k32_split_kernel nine more spilled registers.)
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
  // pixels' fragments of tap (KY, KX) -> slot; piece Q = 0..3 is one 16-byte read (m = Q >> 1, hi / lo = Q & 1)
#define GTXK_LOAD_B(KY, KX, SLOT, Q)                                                           \
    {                                                                                          \
      const int p__ = p0 + (((Q) >> 1) + (KY)) * PW + (KX);                                    \
      const char* pr__ = lds_patch + p__ * RB;                                                 \
      if (((Q) & 1) == 0) bh[SLOT][(Q) >> 1] = *reinterpret_cast<const half8*>(pr__ + ((kg ^ swz128(p__)) << 4)); \
      else bl[SLOT][(Q) >> 1] = *reinterpret_cast<const half8*>(pr__ + (((CPR + kg) ^ swz128(p__)) << 4)); \
    }
  // weights' fragments of (tap column KX, cout block A) -> slot
#define GTXK_LOAD_A(KX, A, SLOT)                                                               \
    {                                                                                          \
      const int nrow__ = 16 * (A) + col;                                                       \
      const char* wr__ = lds_w + ((KX) * BN + nrow__) * RB;                                    \
      ah[SLOT] = *reinterpret_cast<const half8*>(wr__ + ((kg ^ swz128(nrow__)) << 4));     \
      al[SLOT] = *reinterpret_cast<const half8*>(wr__ + (((CPR + kg) ^ swz128(nrow__)) << 4)); \
    }
  // One kernel row = 12 units (tap column kx, cout block a) of 6 MFMAs; unit u reads the weights of unit u + 1 and one piece of
  // the next tap's pixels (the next row's first tap too: the patch stays through the chunk). BSLOT0 = slot of the row's first tap.
#define GTXK_UNIT(KY, U, LAST_ROW)                                                             \
    {                                                                                          \
      constexpr int kx__ = (U) / 4, a__ = (U) % 4;                                             \
      constexpr int bs__ = ((KY) * 3 + kx__) & 1;                                              \
      __builtin_amdgcn_sched_barrier(0);                                                       \
      if ((U) + 1 < 12) GTXK_LOAD_A(((U) + 1) / 4, ((U) + 1) % 4, ((U) + 1) & 1)               \
      if (kx__ < 2) GTXK_LOAD_B(KY, kx__ + 1, bs__ ^ 1, a__)                                   \
      else if (!(LAST_ROW)) GTXK_LOAD_B((KY) + 1, 0, bs__ ^ 1, a__)                            \
      acc[a__][0] = GTXK_MFMA(al[(U) & 1], bh[bs__][0], acc[a__][0]);                          \
      acc[a__][1] = GTXK_MFMA(al[(U) & 1], bh[bs__][1], acc[a__][1]);                          \
      acc[a__][0] = GTXK_MFMA(ah[(U) & 1], bl[bs__][0], acc[a__][0]);                          \
      acc[a__][1] = GTXK_MFMA(ah[(U) & 1], bl[bs__][1], acc[a__][1]);                          \
      acc[a__][0] = GTXK_MFMA(ah[(U) & 1], bh[bs__][0], acc[a__][0]);                          \
      acc[a__][1] = GTXK_MFMA(ah[(U) & 1], bh[bs__][1], acc[a__][1]);                          \
      _Pragma("unroll") for (int i__ = 0; i__ < 3; ++i__) {                                    \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                     \
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                     \
      }                                                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                       \
    }
#define GTXK_ROW(KY, LAST_ROW)                                                                 \
    GTXK_LOAD_A(0, 0, 0)                                                                       \
    GTXK_UNIT(KY, 0, LAST_ROW) GTXK_UNIT(KY, 1, LAST_ROW) GTXK_UNIT(KY, 2, LAST_ROW) GTXK_UNIT(KY, 3, LAST_ROW)   \
    GTXK_UNIT(KY, 4, LAST_ROW) GTXK_UNIT(KY, 5, LAST_ROW) GTXK_UNIT(KY, 6, LAST_ROW) GTXK_UNIT(KY, 7, LAST_ROW)   \
    GTXK_UNIT(KY, 8, LAST_ROW) GTXK_UNIT(KY, 9, LAST_ROW) GTXK_UNIT(KY, 10, LAST_ROW) GTXK_UNIT(KY, 11, LAST_ROW)

  for (int chunk = 0; chunk < nchunks; ++chunk) {
    // ---- kernel row 0: new patch + the row's weights ----
    __syncthreads();                               // the previous chunk's fragment reads are done
    GTXK_COMMIT_PATCH()
    GTXK_COMMIT_W()
    __syncthreads();
    GTXK_PREFETCH_W(3 * chunk + 1)
    GTXK_LOAD_B(0, 0, 0, 0) GTXK_LOAD_B(0, 0, 0, 1) GTXK_LOAD_B(0, 0, 0, 2) GTXK_LOAD_B(0, 0, 0, 3)
    GTXK_ROW(0, false)
    // ---- kernel row 1 ----
    __syncthreads();
    GTXK_COMMIT_W()
    __syncthreads();
    GTXK_PREFETCH_W(3 * chunk + 2)
    GTXK_ROW(1, false)
    // ---- kernel row 2: the next chunk's patch and first row are requested here ----
    __syncthreads();
    GTXK_COMMIT_W()
    __syncthreads();
    if (chunk + 1 < nchunks) {
      GTXK_PREFETCH_PATCH(chunk + 1)
      GTXK_PREFETCH_W(3 * chunk + 3)
    }
    GTXK_ROW(2, true)
  }
#undef GTXK_ROW
#undef GTXK_UNIT
#undef GTXK_LOAD_A
#undef GTXK_LOAD_B

  // ---- epilogue: acc * 2^-shift -> activation (+ residual) -> split -> NHWC pair format (conv_split_device.hpp) ----
  epilogue_k32(acc, P, smem, ct, n, oy0, ox0, wave, lane);
}

}  // namespace

void conv_k32_launch(const ConvGroup& g, const ConvConfig& c, hipStream_t stream) {
  GTX_CHECK(c.ks == 3 && c.stride == 1 && c.bn == K32Tile::BN && c.kc == K32Tile::KC && c.th == 8,
            "conv (K32 form): 3x3 stride 1, 64-cout tiles, 32-channel chunks (ks=%d stride=%d bn=%d kc=%d)", c.ks, c.stride, c.bn, c.kc);
  for (int i = 0; i < g.count; ++i)
    GTX_CHECK(g.p[i].Cin % K32Tile::KC == 0 && g.p[i].post_w == nullptr && g.p[i].front_img == nullptr && g.p[i].c_split == 0,
              "conv (K32 form): Cin %d must be a multiple of 32 and the launch a plain 3x3 layer", g.p[i].Cin);
  launch_conv_group<conv_k32_split_kernel>(g, 256, K32Tile::LDS_BYTES, stream);
}

}  // namespace gtx
