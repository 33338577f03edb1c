// One symbol of a baseline JPEG scan decoded from a plan's tables (device code, included by csrc/jpeg_entropy.hip and
// csrc/jpeg_restart.hip): the table walk of the host parser's decode() and the DC / AC rules of its block loop, as one total
// step. Both GPU entropy routes decode with it, so a symbol means the same on either; what differs is where a lane starts and
// what its sink does with the values.
//
// The caller hands over the next 64 bits of the stream (`win`, bits past the data are zero) and how many of them are real
// (`left`); a symbol that would use a bit past `left` is refused, like the parser's consume(). Every table index is bounded here.
#pragma once
#include <hip/hip_runtime.h>

#include "jpeg_parse.hpp"

namespace gtx {
namespace jpegsym {

// What step() returns.
constexpr uint32_t kBad = 0;          // no such code, a DC category above 15, a run that leaves the block, or too few bits left
constexpr uint32_t kGo = 1;           // the block goes on (z is the next zigzag index, 1..63)
constexpr uint32_t kBlockEnd = 2;     // EOB, a ZRL that leaves the block, or coefficient 63: the next symbol is a DC symbol

__device__ __forceinline__ int extend(uint32_t v, uint32_t s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }   // s in 1..15

// The code at the top of `top` (16 bits): its length (0: in no table) and symbol.
__device__ __forceinline__ void lookup(const jpeg::PlanHuff& t, uint32_t top, uint32_t* len, uint32_t* sym) {
  *len = 0, *sym = 0;
  const uint32_t e = t.look[top >> 7];
  if (e) {
    *len = e >> 8, *sym = e & 255u;
    return;
  }
  for (uint32_t l = 10; l <= 16; ++l) {
    const int code = (int)(top >> (16 - l));
    if (code <= t.maxcode[l]) {
      const int idx = t.valoff[l] + code;
      if (idx >= 0 && idx < (int)min(t.nvals, 256u)) *len = l, *sym = t.vals[idx];
      return;
    }
  }
}

// z == 0: the block's DC symbol (t its component's DC table), else an AC symbol at zigzag index z (t the AC table). *used: the
// bits the symbol and its amplitude took (at least 1 unless kBad). Sink: begin() and dc(difference) for a DC symbol,
// ac(z, value) for a coefficient, end() when the block is complete, poisoned(at_dc) before kBad.
template <class Sink>
__device__ __forceinline__ uint32_t step(const jpeg::PlanHuff& t, uint64_t win, uint64_t left, uint32_t& z, uint32_t* used, Sink& sink) {
  *used = 0;
  uint32_t len, sym;
  lookup(t, (uint32_t)(win >> 48), &len, &sym);
  if (len == 0 || len > 16 || len > left) {                       // no such code, or it ends past the data
    sink.poisoned(z == 0);
    return kBad;
  }
  if (z == 0) {                                                   // DC: the category, then that many bits
    const uint32_t s = sym;
    if (s > 15 || len + s > left) {
      sink.poisoned(true);
      return kBad;
    }
    sink.begin();
    sink.dc(s ? extend((uint32_t)((win << len) >> (64 - s)), s) : 0);
    *used = len + s, z = 1;
    return kGo;
  }
  const uint32_t r = sym >> 4, s = sym & 15u;
  bool done = false;
  if (s == 0) {
    *used = len;
    if (r != 15) done = true;                                     // EOB
    else if ((z += 16) >= 64) done = true;                        // ZRL; the parser's loop ends without a word when it leaves the block
  } else {
    z += r;
    if (z > 63 || len + s > left) {
      sink.poisoned(false);
      return kBad;
    }
    sink.ac(z, extend((uint32_t)((win << len) >> (64 - s)), s));
    *used = len + s;
    if (++z == 64) done = true;
  }
  if (!done) return kGo;
  sink.end();
  return kBlockEnd;
}

}  // namespace jpegsym
}  // namespace gtx
