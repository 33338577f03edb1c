// The multi-workgroup exclusive prefix sum of the JPEG sink (device code, included by csrc/jpeg_enc.hip and csrc/jpeg_huff.hip):
// uint32 values in tiles of kJpegScanTile -> offsets of type Off. The record's coefficient offsets are uint32 (a record's sizes
// are); the entropy coder's bit and byte offsets are uint64. Three launches: tile sums, the scan of the sums in one workgroup,
// the offsets inside every tile.
//
// The count of values is either the host's (n_dev == NULL) or read from HBM when the launch runs: *n_dev holds a bit count and
// the values are the per-chunk counts of the stuff pass, one per kJpegStuffChunk bytes of ceil(*n_dev / 8). The grid is then
// sized for the largest count and workgroups past the real one leave at once.
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_enc.hpp"

namespace gtx {
namespace jpegscan {

constexpr int kScanLanes = 256, kScanPer = kJpegScanTile / kScanLanes;
static_assert(kScanPer * kScanLanes == kJpegScanTile, "a tile is a whole number of values per lane");

__device__ __forceinline__ uint64_t stuff_chunks(uint64_t bits) { return ((bits + 7) / 8 + kJpegStuffChunk - 1) / kJpegStuffChunk; }
__device__ __forceinline__ uint64_t count_of(const uint64_t* n_dev, uint64_t n) { return n_dev ? stuff_chunks(*n_dev) : n; }

// the workgroup's inclusive scan of one value per lane; *total: the sum over the workgroup. Every lane must call it.
template <typename T>
__device__ __forceinline__ T block_scan_inclusive(T v, T* s /* [kScanLanes] */, T* total) {
  const int t = (int)threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < kScanLanes; off <<= 1) {
    const T add = t >= off ? s[t - off] : (T)0;
    __syncthreads();
    s[t] += add;
    __syncthreads();
  }
  const T incl = s[t];
  *total = s[kScanLanes - 1];
  __syncthreads();                                                // s may be written again by the caller's next round
  return incl;
}

// clamp: every value is taken as min(value, clamp) (a block length is at most 64 whatever the buffer holds)
template <typename Off>
__global__ __launch_bounds__(kScanLanes) void scan_sums_kernel(const uint32_t* __restrict__ vals, uint64_t n_host, const uint64_t* __restrict__ n_dev,
                                                                uint32_t clamp, Off* __restrict__ tile_sum) {
  __shared__ Off s[kScanLanes];
  const uint64_t n = count_of(n_dev, n_host);
  if ((uint64_t)blockIdx.x * kJpegScanTile >= n) return;           // the whole workgroup: no barrier is split
  const uint64_t base = (uint64_t)blockIdx.x * kJpegScanTile + (uint64_t)threadIdx.x * kScanPer;
  Off v = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j)
    if (base + j < n) v += min(vals[base + j], clamp);
  Off total;
  block_scan_inclusive<Off>(v, s, &total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// One workgroup: tile_sum[0, n_tiles) -> its exclusive prefix sum in place; the grand total goes to *closing.
template <typename Off>
__global__ __launch_bounds__(kScanLanes) void scan_tiles_kernel(Off* __restrict__ tile_sum, uint64_t n_host, const uint64_t* __restrict__ n_dev,
                                                                 Off* __restrict__ closing) {
  __shared__ Off s[kScanLanes];
  const uint64_t n = count_of(n_dev, n_host), n_tiles = (n + kJpegScanTile - 1) / kJpegScanTile;
  Off carry = 0;
  for (uint64_t first = 0; first < n_tiles; first += kScanLanes) {
    const uint64_t i = first + threadIdx.x;
    const Off v = i < n_tiles ? tile_sum[i] : (Off)0;
    Off total;
    const Off incl = block_scan_inclusive<Off>(v, s, &total);
    if (i < n_tiles) tile_sum[i] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) *closing = carry;
}

template <typename Off>
__global__ __launch_bounds__(kScanLanes) void scan_apply_kernel(const uint32_t* __restrict__ vals, uint64_t n_host, const uint64_t* __restrict__ n_dev,
                                                                 uint32_t clamp, const Off* __restrict__ tile_off, Off* __restrict__ offsets) {
  __shared__ Off s[kScanLanes];
  const uint64_t n = count_of(n_dev, n_host);
  if ((uint64_t)blockIdx.x * kJpegScanTile >= n) return;
  const uint64_t base = (uint64_t)blockIdx.x * kJpegScanTile + (uint64_t)threadIdx.x * kScanPer;
  uint32_t l[kScanPer];
  Off v = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    l[j] = base + j < n ? min(vals[base + j], clamp) : 0u;
    v += l[j];
  }
  Off total;
  Off run = tile_off[blockIdx.x] + block_scan_inclusive<Off>(v, s, &total) - v;
#pragma unroll
  for (int j = 0; j < kScanPer; ++j) {
    if (base + j < n) offsets[base + j] = run;
    run += l[j];
  }
}

// The three launches. n_max sizes the grids (n itself when the count is the host's); closing: where the grand total goes.
template <typename Off>
inline void scan_launch(hipStream_t s, const uint32_t* vals, uint64_t n_max, const uint64_t* n_dev, uint32_t clamp, Off* tiles, Off* offsets, Off* closing) {
  const unsigned n_tiles = (unsigned)((n_max + kJpegScanTile - 1) / kJpegScanTile);
  hipLaunchKernelGGL(scan_sums_kernel<Off>, dim3(n_tiles), dim3(kScanLanes), 0, s, vals, n_max, n_dev, clamp, tiles);
  hipLaunchKernelGGL(scan_tiles_kernel<Off>, dim3(1), dim3(kScanLanes), 0, s, tiles, n_max, n_dev, closing);
  hipLaunchKernelGGL(scan_apply_kernel<Off>, dim3(n_tiles), dim3(kScanLanes), 0, s, vals, n_max, n_dev, clamp, (const Off*)tiles, offsets);
}

}  // namespace jpegscan
}  // namespace gtx
