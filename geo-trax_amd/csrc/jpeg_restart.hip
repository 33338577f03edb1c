// Baseline JPEG with restart intervals, the entropy half of reading, on the GPU: what cv2.VideoCapture.read()
// (geotrax/extract.py:146) does before the inverse DCT, for frames that carry a DRI segment. At every RSTn the stream is byte
// aligned, the DC predictors are zero and the MCU index is known, so an interval decodes with no knowledge of the others: no
// synchronisation rounds, no convergence check, no DC prefix sum (compare csrc/jpeg_entropy.hip, the route for scans without
// markers). The host walks the header, removes stuffing and markers and notes where every interval starts
// (jpeg::plan_intervals()).
//
//   jpeg_restart_kernel        one lane per restart interval, the intervals of up to kJpegRestartMaxFrames frames in one launch. A
//                              workgroup (one wave) belongs to one frame and stages that frame's six Huffman tables in LDS; the
//                              stream is read straight from global memory, a lane's two current words kept in registers. Lane i
//                              starts at byte start[i] with block 0 of MCU i * Ri and zero predictors, decodes its MCUs with
//                              the symbol step of csrc/jpeg_symbol.hpp (the one the self-synchronising route uses) and writes
//                              coefficients, DC resolved, into the zeroed dense [n_blocks][64], and each block's length.
//   jpegscan::scan_* <u32>     block lengths -> offset[] of the record
//   jpeg_entropy_pack_kernel   the runs compacted into coef[]; header, quantisers (csrc/jpeg_entropy.hip)
//
// The state machine is total. A code in no table, a run that leaves the block, a DC category above 15, a DC value outside
// int16, an interval whose bits end before its blocks do, and an interval in front of a marker with 8 or more unread bits
// behind its last block (the parser's "marker is not where the interval ends") set the frame's status word; the host parser
// then decodes the frame and words the refusal. Bits at or past start[i + 1] read as zero and cannot be consumed, so no lane
// uses a bit of another interval; every load is bounded by the stream's padded length, every table index by jpeg_symbol.hpp,
// every block index by the lane's own range. Every step consumes at least one bit, so a lane's loop ends.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "detector.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_restart.hpp"
#include "jpeg_scan.hpp"
#include "jpeg_symbol.hpp"

namespace gtx {
namespace {
using jpeg::PlanHuff;

constexpr int kTabWords = 6 * (int)sizeof(PlanHuff) / 4;

struct Frame {
  const uint8_t* plan;
  int16_t* dense;
  uint32_t* lens;
  uint32_t* status;
  uint32_t first_wg;                                              // the frame's first workgroup in the launch
  uint32_t n_intervals, restart, n_mcus, bpm, luma, n_blocks;
  uint32_t stream_at, stream_bytes;                               // offset of the clean stream in the plan; its length
};
struct Batch {
  Frame f[kJpegRestartMaxFrames];
  uint32_t n;
};

// A lane's side of the decode: the block it is in, the predictors of its interval, the block's length so far.
struct LaneSink {
  int16_t* dense;
  uint32_t* lens;
  uint32_t b, c;                                                  // the block being decoded (inside the lane's range), its component
  int pred[3];
  uint32_t len;
  bool bad;
  __device__ __forceinline__ void begin() { len = 0; }
  __device__ __forceinline__ void dc(int diff) {
    pred[c] += diff;                                              // |diff| < 2^15 and pred is checked every time: no overflow
    if (pred[c] < -32768 || pred[c] > 32767) bad = true;
    dense[(size_t)b * 64] = (int16_t)pred[c];
    len = pred[c] ? 1u : 0u;
  }
  __device__ __forceinline__ void ac(uint32_t z, int v) {          // z in 1..63
    dense[(size_t)b * 64 + z] = (int16_t)v;
    len = z + 1;
  }
  __device__ __forceinline__ void end() { lens[b] = len; }
  __device__ __forceinline__ void poisoned(bool) { bad = true; }
};

__global__ __launch_bounds__(kJpegRestartLanes) void jpeg_restart_kernel(Batch batch) {
  __shared__ uint32_t tabs[kTabWords];
  uint32_t fi = 0;                                                // the workgroup's frame: the last whose first workgroup is not past it
  for (uint32_t k = 1; k < batch.n && k < (uint32_t)kJpegRestartMaxFrames; ++k)
    if (batch.f[k].first_wg <= blockIdx.x) fi = k;
  const Frame& f = batch.f[fi];
  const uint32_t* src_t = reinterpret_cast<const uint32_t*>(f.plan + jpeg::kPlanHuffOffset);
  for (int i = (int)threadIdx.x; i < kTabWords; i += kJpegRestartLanes) tabs[i] = src_t[i];
  __syncthreads();
  const uint32_t i = (blockIdx.x - f.first_wg) * kJpegRestartLanes + threadIdx.x;
  if (i >= f.n_intervals) return;                                 // no barrier below
  const PlanHuff* huff = reinterpret_cast<const PlanHuff*>(tabs);
  const uint32_t* start = reinterpret_cast<const uint32_t*>(f.plan + jpeg::kPlanStreamOffset);
  const uint32_t* stream = reinterpret_cast<const uint32_t*>(f.plan + f.stream_at);
  const uint32_t n_words = (f.stream_bytes + 3) / 4;
  const uint32_t byte1 = min(start[i + 1], f.stream_bytes), byte0 = min(start[i], byte1);
  const uint64_t bit0 = 8ull * byte0, bits = 8ull * (byte1 - byte0);
  const uint64_t mcu0 = (uint64_t)i * f.restart, mcu1 = min(mcu0 + f.restart, (uint64_t)f.n_mcus);
  const uint32_t b_end = (uint32_t)min(mcu1 * f.bpm, (uint64_t)f.n_blocks);
  LaneSink sink{f.dense, f.lens, (uint32_t)min(mcu0 * f.bpm, (uint64_t)f.n_blocks), 0u, {0, 0, 0}, 0u, false};
  uint64_t p = 0;                                                 // bits of the interval consumed
  uint32_t k = 0, z = 0;                                          // block within the MCU; zigzag index, 0 = the DC symbol comes next
  uint32_t cw = 0xFFFFFFF0u, w0 = 0, w1 = 0;                      // stream words cw, cw + 1 (none yet: no word index comes near)
  while (sink.b < b_end) {
    const uint32_t c = (f.bpm == 1 || k < f.luma) ? 0u : min(1u + (k - f.luma), 2u);
    sink.c = c;
    const uint64_t q = bit0 + p;
    const uint32_t w = (uint32_t)(q >> 5);
    if (w != cw) {
      w0 = w == cw + 1 ? w1 : (w < n_words ? stream[w] : 0u);
      w1 = w + 1 < n_words ? stream[w + 1] : 0u;
      cw = w;
    }
    uint64_t win = ((uint64_t)__builtin_bswap32(w0) << 32 | __builtin_bswap32(w1)) << (q & 31u);
    const uint64_t left = bits - p;
    if (left < 64) win = left ? win & (~0ull << (64 - left)) : 0ull;   // bits of the next interval read as zero
    uint32_t used;
    const uint32_t r = jpegsym::step(huff[z == 0 ? c : 3u + c], win, left, z, &used, sink);
    if (r == jpegsym::kBad || sink.bad) {
      sink.bad = true;
      break;
    }
    p += used;
    if (r == jpegsym::kBlockEnd) ++sink.b, k = k + 1 == f.bpm ? 0u : k + 1, z = 0;
  }
  // a marker follows every interval but the last: the pad bits of one byte at most may stand in front of it
  if (!sink.bad && i + 1 < f.n_intervals && bits - p >= 8) sink.bad = true;
  if (sink.bad) atomicOr(f.status, kJpegRestartInvalid);
}

}  // namespace

JpegRestart::JpegRestart(gtx_ctx* ctx, int max_frames, size_t max_blocks) : ctx_(ctx), max_frames_(max_frames), max_blocks_(max_blocks) {
  if (!ctx) fail(GTX_ERR_INVALID, "ctx is NULL");
  if (max_frames < 1 || max_frames > 4096 || max_blocks == 0 || max_blocks > ((size_t)1 << 25))
    fail(GTX_ERR_INVALID, "jpeg_restart: %d frames of %zu blocks", max_frames, max_blocks);
  GTX_HIP(hipSetDevice(ctx->device));
  const size_t n = (size_t)max_frames;
  d_dense_.alloc(n * max_blocks * 64 * sizeof(int16_t));
  d_lens_.alloc(n * max_blocks * sizeof(uint32_t));
  d_tiles_.alloc(n * ((max_blocks + kJpegScanTile - 1) / kJpegScanTile) * sizeof(uint32_t));
  d_state_.alloc(n * 2 * sizeof(uint32_t));
}

void JpegRestart::enqueue(int n, const uint8_t* const* d_plans, const jpeg::PlanHeader* phs, uint8_t* const* d_recs) {
  if (n < 1 || n > max_frames_ || !d_plans || !phs || !d_recs) fail(GTX_ERR_INVALID, "jpeg_restart: %d frames for a decoder of %d", n, max_frames_);
  GTX_HIP(hipSetDevice(ctx_->device));
  hipStream_t s = ctx_->stream;
  const size_t tiles_per = (max_blocks_ + kJpegScanTile - 1) / kJpegScanTile;
  for (int first = 0; first < n; first += kJpegRestartMaxFrames) {
    const int count = std::min(n - first, kJpegRestartMaxFrames);
    Batch batch;
    memset(&batch, 0, sizeof batch);
    uint32_t wgs = 0;
    for (int j = 0; j < count; ++j) {
      const int k = first + j;
      const jpeg::PlanHeader& ph = phs[k];
      const uint32_t nb = ph.n_blocks, luma = ph.hs * ph.vs, bpm = ph.ncomp == 1 ? 1u : luma + 2u;
      const uint64_t n_mcus = (uint64_t)ph.mcus_x * ph.mcus_y;
      if (!d_plans[k] || !d_recs[k] || ph.magic != jpeg::kIntervalPlanMagic || nb == 0 || nb > max_blocks_ || ph.restart == 0 || bpm > 6 ||
          (ph.ncomp != 1 && ph.ncomp != 3) || n_mcus * bpm != nb || ph.reserved != jpeg::interval_count(n_mcus, ph.restart))
        fail(GTX_ERR_INVALID, "jpeg_restart: frame %d is no interval plan of at most %zu blocks", k, max_blocks_);
      Frame& f = batch.f[j];
      f.plan = d_plans[k];
      f.dense = d_dense_.as<int16_t>() + (size_t)k * max_blocks_ * 64;
      f.lens = d_lens_.as<uint32_t>() + (size_t)k * max_blocks_;
      f.status = d_state_.as<uint32_t>() + 2 * (size_t)k;
      f.first_wg = wgs;
      f.n_intervals = ph.reserved, f.restart = ph.restart, f.n_mcus = (uint32_t)n_mcus, f.bpm = bpm, f.luma = luma, f.n_blocks = nb;
      f.stream_at = (uint32_t)jpeg::interval_stream_offset(f.n_intervals), f.stream_bytes = ph.stream_bytes;
      wgs += (f.n_intervals + kJpegRestartLanes - 1) / kJpegRestartLanes;
      GTX_HIP(hipMemsetAsync(f.dense, 0, (size_t)nb * 64 * sizeof(int16_t), s));
      GTX_HIP(hipMemsetAsync(f.lens, 0, (size_t)nb * sizeof(uint32_t), s));
      GTX_HIP(hipMemsetAsync(f.status, 0, 2 * sizeof(uint32_t), s));
    }
    batch.n = (uint32_t)count;
    hipLaunchKernelGGL(jpeg_restart_kernel, dim3(wgs), dim3(kJpegRestartLanes), 0, s, batch);
    for (int j = 0; j < count; ++j) {
      const int k = first + j;
      const Frame& f = batch.f[j];
      uint32_t* offsets = reinterpret_cast<uint32_t*>(d_recs[k] + jpeg::kOffsetsOffset);
      jpegscan::scan_launch<uint32_t>(s, f.lens, f.n_blocks, nullptr, 64u, d_tiles_.as<uint32_t>() + (size_t)k * tiles_per, offsets, offsets + f.n_blocks);
      JpegEntropy::pack_launch(s, d_plans[k], JpegEntropy::record_header(phs[k]), f.dense, d_recs[k], 1, f.status);
    }
  }
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
