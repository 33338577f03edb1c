// Device-side access to "map" tensors (rtdetr_kernels.hpp: NHWC activations in the net's format, DT_F16 / DT_F32 / DT_F32S = the pair
// format of split_format.hpp) for the kernels that run on them next to the convolutions: rtdetr_kernels.hip (depthwise convolutions,
// C2PSA's attention, ...) and area_attn.hip (YOLO12's area attention). Include from a .hip file only; everything here is file-local.
#pragma once
#include "common.hpp"

namespace gtx {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

// ---- 8-channel groups in the three activation formats; e = element index of the group's first channel (a multiple of 8)
template <int FMT> __device__ __forceinline__ void load8(const void* base, size_t e, float v[8]) {
  const char* b = static_cast<const char*>(base);
  if constexpr (FMT == DT_F16) {
    const half8 h = *reinterpret_cast<const half8*>(b + e * 2);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
  } else if constexpr (FMT == DT_F32) {
    const float4 a = *reinterpret_cast<const float4*>(b + e * 4), c = *reinterpret_cast<const float4*>(b + e * 4 + 16);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = c.x; v[5] = c.y; v[6] = c.z; v[7] = c.w;
  } else {                                                       // pair format: 8 hi halves then 8 lo halves (split_format.hpp)
    const half8 hi = *reinterpret_cast<const half8*>(b + e * 4), lo = *reinterpret_cast<const half8*>(b + e * 4 + 16);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)hi[i] + (float)lo[i];
  }
}
template <int FMT> __device__ __forceinline__ void store8(void* base, size_t e, const float v[8], bool& sat) {
  char* b = static_cast<char*>(base);
  if constexpr (FMT == DT_F16) {
    half8 h;
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = (_Float16)v[i];
    *reinterpret_cast<half8*>(b + e * 2) = h;
  } else if constexpr (FMT == DT_F32) {
    *reinterpret_cast<float4*>(b + e * 4) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(b + e * 4 + 16) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    half8 hi, lo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x = __builtin_amdgcn_fmed3f(v[i], -65504.f, 65504.f);   // a NaN comes out as -65504, like the convolutions' split
      sat |= x != v[i];
      hi[i] = (_Float16)x;
      lo[i] = (_Float16)(x - (float)hi[i]);                                // x - hi is exact in fp32
    }
    *reinterpret_cast<half8*>(b + e * 4) = hi;
    *reinterpret_cast<half8*>(b + e * 4 + 16) = lo;
  }
}
template <int FMT> __device__ __forceinline__ float load1(const void* base, size_t e) {
  const char* b = static_cast<const char*>(base);
  if constexpr (FMT == DT_F16) return (float)*reinterpret_cast<const _Float16*>(b + e * 2);
  else if constexpr (FMT == DT_F32) return *reinterpret_cast<const float*>(b + e * 4);
  else {
    const char* g = b + (e & ~(size_t)7) * 4 + 2 * (e & 7);
    return (float)*reinterpret_cast<const _Float16*>(g) + (float)*reinterpret_cast<const _Float16*>(g + 16);
  }
}
// Four consecutive channels (e a multiple of 4) in the three activation formats: half a group of the pair format
template <int FMT> __device__ __forceinline__ void load4(const void* base, size_t e, float v[4]) {
  const char* b = static_cast<const char*>(base);
  if constexpr (FMT == DT_F16) {
    const half4 h = *reinterpret_cast<const half4*>(b + e * 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)h[i];
  } else if constexpr (FMT == DT_F32) {
    const float4 a = *reinterpret_cast<const float4*>(b + e * 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
    const char* g = b + (e & ~(size_t)7) * 4 + 2 * (e & 7);
    const half4 hi = *reinterpret_cast<const half4*>(g), lo = *reinterpret_cast<const half4*>(g + 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (float)hi[i] + (float)lo[i];
  }
}
template <int FMT> __device__ __forceinline__ void store4(void* base, size_t e, const float v[4], bool& sat) {
  char* b = static_cast<char*>(base);
  if constexpr (FMT == DT_F16) {
    half4 h;
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = (_Float16)v[i];
    *reinterpret_cast<half4*>(b + e * 2) = h;
  } else if constexpr (FMT == DT_F32) {
    *reinterpret_cast<float4*>(b + e * 4) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    half4 hi, lo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float x = __builtin_amdgcn_fmed3f(v[i], -65504.f, 65504.f);
      sat |= x != v[i];
      hi[i] = (_Float16)x;
      lo[i] = (_Float16)(x - (float)hi[i]);
    }
    char* g = b + (e & ~(size_t)7) * 4 + 2 * (e & 7);
    *reinterpret_cast<half4*>(g) = hi;
    *reinterpret_cast<half4*>(g + 16) = lo;
  }
}

// Runs the statement once with F = the format as a compile-time constant, then checks the launch
#define RT_FMT(fmt, ...)                                                           \
  do {                                                                             \
    switch (fmt) {                                                                 \
      case DT_F16: { constexpr int F = DT_F16; __VA_ARGS__; } break;               \
      case DT_F32: { constexpr int F = DT_F32; __VA_ARGS__; } break;               \
      case DT_F32S: { constexpr int F = DT_F32S; __VA_ARGS__; } break;             \
      default: fail(-3, "rtdetr: unknown activation format %d", (int)(fmt));       \
    }                                                                              \
    GTX_HIP(hipGetLastError());                                                    \
  } while (0)

__device__ __forceinline__ void flag_sat(int* sat, bool s) {
  if (sat && s) *sat = 1;
}

}  // namespace
}  // namespace gtx
