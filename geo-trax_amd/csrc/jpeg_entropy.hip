// Baseline JPEG, the entropy half of reading, on the GPU: what cv2.VideoCapture.read() (geotrax/extract.py:146) does before the
// inverse DCT. The host only walks the header and removes the byte stuffing (jpeg::plan()); the Huffman decode of the scan, which
// has no restart markers to enter at, is the self-synchronising parallel decode:
//
//   The clean stream is cut into subsequences of S bits, one lane each. A lane's state is (bit position, block index within the MCU,
//   zigzag index; zigzag 0 = the block's DC symbol comes next), one 64-bit word. f_i(entry) is the state in which a decode of
//   subsequence i that starts in `entry` first stands at or past bit (i + 1) * S. f_i is total: a code in no table, a run of zeros
//   that leaves the block, a DC category above 15, too few bits left or an entry outside the subsequence give the poison value.
//
//   jpeg_entropy_sync_kernel   round 0: every lane decodes from its own boundary with state (0, 0); then, in LDS, a lane whose left
//                              neighbour's exit differs from the entry it decoded from decodes again from that exit, until no lane
//                              of the workgroup changes (at most `lanes` times). Rounds 1 .. R - 1: a workgroup takes the exit the
//                              workgroup before it stored in the round before (two buffers: what a round reads no launch of that
//                              round writes, so the rounds used do not depend on the order workgroups run in) and leaves at once
//                              when that is the entry it has. Subsequence 0's entry is known; where every entry equals the left
//                              neighbour's exit, every entry is by induction the sequential decoder's.
//   jpegscan::scan_* <u32>     blocks that begin in every subsequence -> index of the first of them
//   jpeg_entropy_write_kernel  decodes once more from the entry, checks entry == left exit (else: not converged), writes the
//                              coefficients into the zeroed dense [n_blocks][64] (DC as the difference), drops what lies past the
//                              last block as the parser does; a poisoned step inside the picture's blocks, or data that ends before
//                              they do, sets `invalid`
//   jpeg_entropy_dcvals_kernel, jpegscan::scan_* per component, jpeg_entropy_dc_kernel
//                              prefix sum of the DC differences by component in scan order (32-bit wrapping sums: the first value
//                              outside int16 is exact, and sets `invalid`); block lengths (last non-zero + 1)
//   jpegscan::scan_* <u32>     block lengths -> offset[] of the record
//   jpeg_entropy_pack_kernel   the runs compacted into coef[]; header, quantisers, status and rounds used
//
// Bits past the end of the stream read as zero and cannot be consumed (the parser's consume()). Every step consumes at least one
// bit, so a lane's loop ends after S steps at most. Every index is checked against its buffer where it is formed.
#include <hip/hip_runtime.h>

#include "detector.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_scan.hpp"
#include "jpeg_symbol.hpp"

namespace gtx {
namespace {
using jpeg::PlanHuff;

constexpr uint64_t kPoison = ~0ull;
constexpr int kSpanWords = 8192, kSpanPad = 32;                   // a workgroup's 32 KB of stream; the overshoot word and the swizzle's group
constexpr int kTabWords = 6 * (int)sizeof(PlanHuff) / 4;
// d_state_: uint32 words
constexpr int kStStatus = 0, kStRounds = 1, kStClosing = 2, kStChanged = 4, kStWords = kStChanged + kJpegEntropyMaxRounds;

struct Geom {
  uint64_t bits;                                                  // of the clean stream
  uint32_t n_words;                                               // 32-bit words of it in the plan (zero padded)
  uint32_t n_lanes, n_wgs, sub_bits;
  uint32_t bpm, luma, ncomp, n_blocks;                            // blocks per MCU, luma blocks per MCU
};

__device__ __forceinline__ uint64_t pack_state(uint64_t p, uint32_t k, uint32_t z) { return p | (uint64_t)k << 40 | (uint64_t)z << 44; }

// LDS word of stream word w of the workgroup's span: the 32 words of a group are permuted by the group's number, so that lanes
// whose subsequences start a whole number of groups apart read different banks
__device__ __forceinline__ uint32_t span_at(uint32_t w) { return (w & ~31u) | ((w ^ (w >> 5)) & 31u); }

// tables and the workgroup's span [wg * span_words, + span_words + 2) of the stream into LDS; words past the stream are 0
__device__ __forceinline__ void stage(const uint8_t* __restrict__ plan, const Geom& g, uint32_t span_words, uint32_t* tabs, uint32_t* span) {
  const uint32_t* src_t = reinterpret_cast<const uint32_t*>(plan + jpeg::kPlanHuffOffset);
  for (int i = (int)threadIdx.x; i < kTabWords; i += (int)blockDim.x) tabs[i] = src_t[i];
  const uint32_t* src_s = reinterpret_cast<const uint32_t*>(plan + jpeg::kPlanStreamOffset);
  const uint64_t first = (uint64_t)blockIdx.x * span_words;
  for (uint32_t i = threadIdx.x; i < span_words + 2 && i < (uint32_t)kSpanWords + 2; i += blockDim.x)
    span[span_at(i)] = first + i < g.n_words ? src_s[first + i] : 0u;
  __syncthreads();
}

struct NoSink {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void dc(int) {}
  __device__ __forceinline__ void ac(uint32_t, int) {}
  __device__ __forceinline__ void end() {}
  __device__ __forceinline__ void poisoned(bool) {}
};

struct WriteSink {
  int16_t* dense;
  uint32_t* aclen;
  uint32_t* status;
  uint32_t nb, b, next_b, maxz;                                   // b: the block being decoded (past nb: dropped), next_b: the next to begin
  __device__ __forceinline__ void flush() {
    if (maxz && b < nb) atomicMax(&aclen[b], maxz);
    maxz = 0;
  }
  __device__ __forceinline__ void begin() { flush(), b = next_b++; }
  __device__ __forceinline__ void dc(int v) { if (b < nb) dense[(size_t)b * 64] = (int16_t)v; }
  __device__ __forceinline__ void ac(uint32_t z, int v) {          // z in 1..63
    if (b < nb) dense[(size_t)b * 64 + z] = (int16_t)v;
    maxz = z + 1;
  }
  __device__ __forceinline__ void end() { flush(); }
  __device__ __forceinline__ void poisoned(bool at_dc) {           // the step belongs to the block that would begin, or to b
    if ((at_dc ? next_b : b) < nb) atomicOr(status, kJpegEntropyInvalid);
  }
};

// f_lane(entry). span: the workgroup's staged words, whose first bit is stream bit span_bit0. *count: blocks that began.
template <class Sink>
__device__ __forceinline__ uint64_t decode_lane(const uint32_t* span, uint64_t span_bit0, const PlanHuff* tabs, const Geom& g, uint64_t lane, uint64_t entry,
                                                uint32_t* count, Sink& sink) {
  *count = 0;
  if (entry >> 50) return kPoison;                                // the poison value, or no state at all
  uint64_t p = entry & ((1ull << 40) - 1);
  uint32_t k = (uint32_t)(entry >> 40) & 15u, z = (uint32_t)(entry >> 44) & 63u;
  const uint64_t lo = lane * g.sub_bits, hi = lo + g.sub_bits;
  if (p < lo || p >= hi || p > g.bits || k >= g.bpm) return kPoison;
  while (p < hi) {                                                // every turn adds at least one bit to p
    const uint32_t c = (g.bpm == 1 || k < g.luma) ? 0u : 1u + (k - g.luma);   // k < bpm = luma + 2: c <= 2
    const PlanHuff& t = tabs[z == 0 ? c : 3u + c];
    const uint32_t q = (uint32_t)(p - span_bit0), w = q >> 5;      // w + 1 <= span_words: staged
    const uint64_t win = ((uint64_t)__builtin_bswap32(span[span_at(w)]) << 32 | __builtin_bswap32(span[span_at(w + 1)])) << (q & 31u);
    const bool at_dc = z == 0;
    uint32_t used;
    const uint32_t r = jpegsym::step(t, win, g.bits - p, z, &used, sink);
    if (r == jpegsym::kBad) return kPoison;
    if (at_dc) ++*count;
    p += used;
    if (r == jpegsym::kBlockEnd) k = k + 1 == g.bpm ? 0u : k + 1, z = 0;
  }
  return pack_state(p, k, z);
}

__global__ __launch_bounds__(256) void jpeg_entropy_sync_kernel(const uint8_t* __restrict__ plan, Geom g, int round, uint64_t* __restrict__ entry,
                                                                uint64_t* __restrict__ exit_, uint32_t* __restrict__ count, uint64_t* __restrict__ edge,
                                                                uint32_t* __restrict__ changed) {
  __shared__ uint32_t tabs[kTabWords];
  __shared__ uint32_t span[kSpanWords + kSpanPad];
  __shared__ uint64_t s_exit[256];
  const uint32_t L = blockDim.x, t = threadIdx.x, wg = blockIdx.x;
  const uint64_t lane = (uint64_t)wg * L + t;
  const bool active = lane < g.n_lanes;
  const uint64_t last = min((uint64_t)(wg + 1) * L, (uint64_t)g.n_lanes) - 1;   // the workgroup's last lane (its first is inside: the grid is n_wgs)
  uint64_t wg_entry = 0;                                          // subsequence 0 starts block 0's DC symbol at bit 0
  if (wg > 0) wg_entry = round == 0 ? pack_state((uint64_t)wg * L * g.sub_bits, 0, 0) : edge[(size_t)((round - 1) & 1) * g.n_wgs + wg - 1];
  if (round > 0 && entry[(uint64_t)wg * L] == wg_entry) {         // the whole workgroup: no barrier is split
    if (t == 0) edge[(size_t)(round & 1) * g.n_wgs + wg] = exit_[last];
    return;
  }
  const uint32_t span_words = L * g.sub_bits / 32;
  stage(plan, g, span_words, tabs, span);
  const PlanHuff* huff = reinterpret_cast<const PlanHuff*>(tabs);
  const uint64_t bit0 = (uint64_t)wg * span_words * 32;
  NoSink sink;
  uint64_t cur_entry = kPoison, cur_exit = kPoison;
  uint32_t cur_count = 0;
  if (active) {
    if (round == 0) {
      cur_entry = t == 0 ? wg_entry : pack_state(lane * g.sub_bits, 0, 0);
      cur_exit = decode_lane(span, bit0, huff, g, lane, cur_entry, &cur_count, sink);
    } else {
      cur_entry = entry[lane], cur_exit = exit_[lane], cur_count = count[lane];
    }
  }
  s_exit[t] = cur_exit;
  __syncthreads();
  for (uint32_t it = 0; it < L; ++it) {                           // lane j is final after j + 1 turns
    const uint64_t want = t == 0 ? wg_entry : s_exit[t - 1];
    const bool again = active && want != cur_entry;
    if (!__syncthreads_or(again)) break;                          // (the barrier also parts the reads above from the writes below)
    if (again) {
      cur_entry = want;
      cur_exit = decode_lane(span, bit0, huff, g, lane, cur_entry, &cur_count, sink);
      s_exit[t] = cur_exit;
    }
    __syncthreads();
  }
  if (active) {
    entry[lane] = cur_entry, exit_[lane] = cur_exit, count[lane] = cur_count;
    if (lane == last) edge[(size_t)(round & 1) * g.n_wgs + wg] = cur_exit;
  }
  if (t == 0) changed[round] = 1u;
}

__global__ __launch_bounds__(256) void jpeg_entropy_write_kernel(const uint8_t* __restrict__ plan, Geom g, const uint64_t* __restrict__ entry,
                                                                 const uint64_t* __restrict__ exit_, const uint32_t* __restrict__ blockoff,
                                                                 int16_t* __restrict__ dense, uint32_t* __restrict__ aclen, uint32_t* __restrict__ status) {
  __shared__ uint32_t tabs[kTabWords];
  __shared__ uint32_t span[kSpanWords + kSpanPad];
  const uint32_t L = blockDim.x, span_words = L * g.sub_bits / 32;
  stage(plan, g, span_words, tabs, span);
  const uint64_t lane = (uint64_t)blockIdx.x * L + threadIdx.x;
  if (lane >= g.n_lanes) return;                                  // no barrier below
  const uint64_t e = entry[lane];
  if (e != (lane == 0 ? 0ull : exit_[lane - 1])) atomicOr(status, kJpegEntropyNotConverged);
  const uint32_t base = blockoff[lane];
  WriteSink sink{dense, aclen, status, g.n_blocks, base - 1u, base, 0u};   // an entry inside a block: the one before the first that begins here
  uint32_t cnt;
  const uint64_t x = decode_lane(span, (uint64_t)blockIdx.x * span_words * 32, reinterpret_cast<const PlanHuff*>(tabs), g, lane, e, &cnt, sink);
  sink.flush();
  // the data ends here: the blocks complete by now must be all of them (the last lane's clean exit stands at the last bit)
  if (lane == g.n_lanes - 1 && x != kPoison && sink.next_b - (((x >> 44) & 63u) ? 1u : 0u) < g.n_blocks) atomicOr(status, kJpegEntropyInvalid);
}

__device__ __forceinline__ uint32_t comp_of(uint32_t b, const Geom& g) {
  if (g.bpm == 1) return 0;
  const uint32_t k = b % g.bpm;
  return k < g.luma ? 0u : 1u + (k - g.luma);
}

// vals[c][b]: block b's DC difference where b belongs to component c, else 0
__global__ __launch_bounds__(256) void jpeg_entropy_dcvals_kernel(const int16_t* __restrict__ dense, Geom g, uint32_t* __restrict__ vals) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= g.n_blocks) return;
  const uint32_t c = comp_of(b, g), d = (uint32_t)(int)dense[(size_t)b * 64];
  for (uint32_t cc = 0; cc < g.ncomp; ++cc) vals[(size_t)cc * g.n_blocks + b] = cc == c ? d : 0u;
}

__global__ __launch_bounds__(256) void jpeg_entropy_dc_kernel(int16_t* __restrict__ dense, Geom g, const uint32_t* __restrict__ pref, const uint32_t* __restrict__ aclen,
                                                              uint32_t* __restrict__ lens, uint32_t* __restrict__ status) {
  const uint32_t b = blockIdx.x * 256 + threadIdx.x;
  if (b >= g.n_blocks) return;
  const int pred = (int)(pref[(size_t)comp_of(b, g) * g.n_blocks + b] + (uint32_t)(int)dense[(size_t)b * 64]);
  if (pred < -32768 || pred > 32767) atomicOr(status, kJpegEntropyInvalid);
  dense[(size_t)b * 64] = (int16_t)pred;
  lens[b] = max(min(aclen[b], 64u), pred ? 1u : 0u);
}

// One lane per (block, position): the runs to coef[]; the first workgroup also writes the record's header and quantisers and the
// frame's result words.
__global__ __launch_bounds__(256) void jpeg_entropy_pack_kernel(const uint8_t* __restrict__ plan, jpeg::RecordHeader hd, const int16_t* __restrict__ dense,
                                                                uint8_t* __restrict__ rec, int rounds, uint32_t* __restrict__ state) {
  const uint32_t nb = hd.n_blocks;
  const uint32_t* offsets = reinterpret_cast<const uint32_t*>(rec + jpeg::kOffsetsOffset);
  int16_t* coef = reinterpret_cast<int16_t*>(rec + jpeg::kOffsetsOffset + 4 * ((size_t)nb + 1));
  if (blockIdx.x == 0) {
    const uint32_t n_coef = min(offsets[nb], 64u * nb);
    hd.n_coef = n_coef, hd.bytes = (uint32_t)(jpeg::kOffsetsOffset + 4 * ((size_t)nb + 1) + 2 * (size_t)n_coef);   // record_bytes()
    uint32_t* out = reinterpret_cast<uint32_t*>(rec);
    const uint32_t* h = reinterpret_cast<const uint32_t*>(&hd);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(plan + jpeg::kPlanQuantOffset);
    for (uint32_t i = threadIdx.x; i < jpeg::kOffsetsOffset / 4; i += 256) out[i] = i < sizeof(hd) / 4 ? h[i] : q[i - sizeof(hd) / 4];
    if (threadIdx.x == 0) {
      uint32_t used = 1;
      for (int r = 1; r < rounds; ++r) used += state[kStChanged + r] ? 1u : 0u;
      state[kStRounds] = used;
    }
  }
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, b = i >> 6;
  const uint32_t z = (uint32_t)(i & 63);
  if (b >= nb) return;
  const uint32_t first = offsets[b], end = offsets[b + 1];
  if (end < first || z >= end - first || (size_t)first + z >= (size_t)64 * nb) return;
  coef[(size_t)first + z] = dense[i];
}

}  // namespace

jpeg::RecordHeader JpegEntropy::record_header(const jpeg::PlanHeader& ph) {
  jpeg::RecordHeader hd;
  memset(&hd, 0, sizeof hd);
  hd.magic = jpeg::kMagic;
  hd.width = ph.width, hd.height = ph.height, hd.ncomp = ph.ncomp, hd.hs = ph.hs, hd.vs = ph.vs, hd.mcus_x = ph.mcus_x, hd.mcus_y = ph.mcus_y;
  hd.n_blocks = ph.n_blocks, hd.n_coef = 64u * ph.n_blocks;
  hd.bytes = (uint32_t)jpeg::record_bytes(hd.n_blocks, hd.n_coef);
  for (int c = 0; c < 3; ++c) hd.bw[c] = ph.bw[c], hd.bh[c] = ph.bh[c];
  return hd;
}

void JpegEntropy::pack_launch(hipStream_t s, const uint8_t* d_plan, const jpeg::RecordHeader& hd, const int16_t* d_dense, uint8_t* d_rec, int rounds, uint32_t* d_state) {
  hipLaunchKernelGGL(jpeg_entropy_pack_kernel, dim3((unsigned)(((size_t)hd.n_blocks * 64 + 255) / 256)), dim3(256), 0, s, d_plan, hd, d_dense, d_rec, rounds, d_state);
}

JpegEntropy::JpegEntropy(gtx_ctx* ctx, size_t max_blocks, size_t max_stream_bytes, int min_sub_bits)
    : ctx_(ctx), max_blocks_(max_blocks), max_stream_bytes_(max_stream_bytes), min_sub_bits_(min_sub_bits) {
  if (!ctx) fail(GTX_ERR_INVALID, "ctx is NULL");
  if (!jpeg_entropy_sub_bits_ok(min_sub_bits) || max_blocks == 0 || max_blocks > ((size_t)1 << 25) || max_stream_bytes > ((size_t)1 << 31))
    fail(GTX_ERR_INVALID, "jpeg_entropy: %zu blocks, %zu bytes of stream at %d bits a lane", max_blocks, max_stream_bytes, min_sub_bits);
  GTX_HIP(hipSetDevice(ctx->device));
  max_lanes_ = std::max<size_t>(1, (max_stream_bytes * 8 + (size_t)min_sub_bits - 1) / (size_t)min_sub_bits);
  const size_t max_wgs = (max_lanes_ + 127) / 128;
  d_entry_.alloc(max_lanes_ * sizeof(uint64_t));
  d_exit_.alloc(max_lanes_ * sizeof(uint64_t));
  d_count_.alloc(max_lanes_ * sizeof(uint32_t));
  d_blockoff_.alloc(max_lanes_ * sizeof(uint32_t));
  d_edge_.alloc(2 * max_wgs * sizeof(uint64_t));
  d_lane_tiles_.alloc((max_lanes_ + kJpegScanTile - 1) / kJpegScanTile * sizeof(uint32_t));
  d_state_.alloc(kStWords * sizeof(uint32_t));
  d_dense_.alloc(max_blocks * 64 * sizeof(int16_t));
  d_aclen_.alloc(max_blocks * sizeof(uint32_t));
  d_lens_.alloc(max_blocks * sizeof(uint32_t));
  d_dcvals_.alloc(3 * max_blocks * sizeof(uint32_t));
  d_dcpref_.alloc(3 * max_blocks * sizeof(uint32_t));
  d_block_tiles_.alloc((max_blocks + kJpegScanTile - 1) / kJpegScanTile * sizeof(uint32_t));
}

void JpegEntropy::enqueue(const uint8_t* d_plan, const jpeg::PlanHeader& ph, int sub_bits, int rounds, uint8_t* d_rec) {
  if (sub_bits == 0) sub_bits = std::max(kJpegEntropySubBits, min_sub_bits_);
  if (rounds == 0) rounds = kJpegEntropyRounds;
  if (!d_plan || !d_rec) fail(GTX_ERR_INVALID, "jpeg_entropy: NULL buffer");
  if (!jpeg_entropy_sub_bits_ok(sub_bits) || sub_bits < min_sub_bits_) fail(GTX_ERR_INVALID, "jpeg_entropy: %d bits a lane (256, 512, 1024 or 2048; this decoder: %d or more)", sub_bits, min_sub_bits_);
  if (rounds < 1 || rounds > kJpegEntropyMaxRounds) fail(GTX_ERR_INVALID, "jpeg_entropy: %d rounds (1..%d)", rounds, kJpegEntropyMaxRounds);
  const uint32_t nb = ph.n_blocks, luma = ph.hs * ph.vs;
  if (nb == 0 || nb > max_blocks_ || ph.stream_bytes > max_stream_bytes_ || ph.stream_bits != 8 * (uint64_t)ph.stream_bytes)
    fail(GTX_ERR_INVALID, "jpeg_entropy: a plan of %u blocks and %u stream bytes for a decoder of %zu and %zu", nb, ph.stream_bytes, max_blocks_, max_stream_bytes_);
  Geom g;
  g.bits = ph.stream_bits, g.n_words = (ph.stream_bytes + 3) / 4, g.sub_bits = (uint32_t)sub_bits;
  g.n_lanes = (uint32_t)std::max<uint64_t>(1, (g.bits + (uint64_t)sub_bits - 1) / (uint64_t)sub_bits);
  const unsigned L = (unsigned)jpeg_entropy_lanes(sub_bits);
  g.n_wgs = (g.n_lanes + L - 1) / L;
  g.ncomp = ph.ncomp, g.luma = luma, g.bpm = ph.ncomp == 1 ? 1u : luma + 2u, g.n_blocks = nb;
  if (g.n_lanes > max_lanes_ || g.bpm > 6 || (ph.ncomp != 1 && ph.ncomp != 3)) fail(GTX_ERR_INTERNAL, "jpeg_entropy: %u lanes, %u blocks an MCU", g.n_lanes, g.bpm);
  GTX_HIP(hipSetDevice(ctx_->device));
  hipStream_t s = ctx_->stream;
  uint32_t* state = d_state_.as<uint32_t>();
  const jpeg::RecordHeader hd = record_header(ph);
  GTX_HIP(hipMemsetAsync(state, 0, kStWords * sizeof(uint32_t), s));
  GTX_HIP(hipMemsetAsync(d_dense_.p, 0, (size_t)nb * 64 * sizeof(int16_t), s));
  GTX_HIP(hipMemsetAsync(d_aclen_.p, 0, (size_t)nb * sizeof(uint32_t), s));
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3(g.n_wgs), dim3(L), 0, s, d_plan, g, r, d_entry_.as<uint64_t>(), d_exit_.as<uint64_t>(), d_count_.as<uint32_t>(),
                       d_edge_.as<uint64_t>(), state + kStChanged);
  jpegscan::scan_launch<uint32_t>(s, d_count_.as<const uint32_t>(), g.n_lanes, nullptr, 0xFFFFFFFFu, d_lane_tiles_.as<uint32_t>(), d_blockoff_.as<uint32_t>(),
                                  state + kStClosing);
  hipLaunchKernelGGL(jpeg_entropy_write_kernel, dim3(g.n_wgs), dim3(L), 0, s, d_plan, g, d_entry_.as<const uint64_t>(), d_exit_.as<const uint64_t>(),
                     d_blockoff_.as<const uint32_t>(), d_dense_.as<int16_t>(), d_aclen_.as<uint32_t>(), state + kStStatus);
  const unsigned block_wgs = (nb + 255) / 256;
  hipLaunchKernelGGL(jpeg_entropy_dcvals_kernel, dim3(block_wgs), dim3(256), 0, s, d_dense_.as<const int16_t>(), g, d_dcvals_.as<uint32_t>());
  for (uint32_t c = 0; c < g.ncomp; ++c)
    jpegscan::scan_launch<uint32_t>(s, d_dcvals_.as<const uint32_t>() + (size_t)c * nb, nb, nullptr, 0xFFFFFFFFu, d_block_tiles_.as<uint32_t>(),
                                    d_dcpref_.as<uint32_t>() + (size_t)c * nb, state + kStClosing + 1);
  hipLaunchKernelGGL(jpeg_entropy_dc_kernel, dim3(block_wgs), dim3(256), 0, s, d_dense_.as<int16_t>(), g, d_dcpref_.as<const uint32_t>(), d_aclen_.as<const uint32_t>(),
                     d_lens_.as<uint32_t>(), state + kStStatus);
  uint32_t* offsets = reinterpret_cast<uint32_t*>(d_rec + jpeg::kOffsetsOffset);
  jpegscan::scan_launch<uint32_t>(s, d_lens_.as<const uint32_t>(), nb, nullptr, 64u, d_block_tiles_.as<uint32_t>(), offsets, offsets + nb);
  pack_launch(s, d_plan, hd, d_dense_.as<const int16_t>(), d_rec, rounds, state);
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
