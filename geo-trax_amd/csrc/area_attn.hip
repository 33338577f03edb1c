// YOLO12's area attention and A2C2f's per-channel residual (see area_attn.hpp). gfx950 only.
//
// What bounds them at the product's 1920 x 1920 input (yolo12s: 4 heads; the stride-16 map has 14 400 tokens = 4 bands of 3 600):
//   area_attn_kernel     the fp32 matrix pipe (v_mfma_f32_16x16x4_f32) and the exponentials: 2 * (32 + 32) FLOPs and one exp per
//                        query-key pair, 4 heads x 4 bands x 3 600^2 pairs per image; K / V are re-read from L2 once per 64 queries
//   scale_add_kernel     HBM (two maps read, one written)
#include "area_attn.hpp"
#include "map_format_device.hpp"

#include <cfloat>

namespace gtx {
namespace {

struct AreaAttn {
  RtMap qkv, out;
  int heads, area;
  int head_stride, k_off, v_off;     // channel of head h's q: coff + h * head_stride; its k / v: + k_off / + v_off
};

// psa_attn_kernel's scheme (rtdetr_kernels.hip: a wave owns 16 queries and walks the keys 16 at a time on v_mfma_f32_16x16x4_f32, the
// probabilities stay in the lanes that computed them, K / V tiles of kAreaAttnKeyTile keys go through LDS with the next stage
// prefetched into registers, online softmax with the running row maximum subtracted) restricted to a band: workgroup (x, y, z) takes
// 64 queries of band y / heads, head y % heads, image z, and its keys are that band's tokens only,
//   S^T[key][query]  = sum_32 K Q * 32^-0.5        8 MFMAs per 16 x 16 tile
//   O^T[dim][query] += sum_key V[key][dim] P^T     8 MFMAs (two 16-dim tiles x four key groups)
// The band length is whatever h w / area is: key slots past the band's end are masked by index before the maximum and get
// probability zero (their LDS rows are zero-filled, never read from HBM), query rows past it are neither read nor stored.
template <int FMT>
__global__ __launch_bounds__(256) void area_attn_kernel(AreaAttn a, int* sat) {
  constexpr int KS = kAreaAttnKeyTile, PK = 36, PV = 36;
  static_assert(KS == 64, "the staging below gives each of 256 threads one 8-channel group of K and one of V");
  __shared__ float s_k[KS * PK];
  __shared__ float s_v[KS * PV];
  const RtMap& qkv = a.qkv;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lc = lane & 15, kk = lane >> 4;
  const int band = blockIdx.y / a.heads, head = blockIdx.y - band * a.heads, n = blockIdx.z;
  const int T = qkv.h * qkv.w, Tb = T / a.area;                 // Tb tokens per band: the launcher refuses T % area != 0
  const size_t tok0 = (size_t)n * T + (size_t)band * Tb;        // the band's first token
  const int chq = qkv.coff + head * a.head_stride, chk = chq + a.k_off, chv = chq + a.v_off;
  const int q0 = blockIdx.x * 64 + wave * 16;
  const float scale = 0.17677669529663687f;      // head_dim^-0.5, head_dim = 32
  float qf[8];                                     // B operand of the first product: Q[query lc][4 i + kk], scaled
  {
    const int qi = q0 + lc;
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[i] = qi < Tb ? load1<FMT>(qkv.ptr, (tok0 + qi) * qkv.cstride + chq + 4 * i + kk) * scale : 0.f;
  }
  floatx4 o[2];                                    // O^T[dim 16 t + 4 kk + r][query lc]
#pragma unroll
  for (int t = 0; t < 2; ++t) o[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  float m = -FLT_MAX, l = 0.f;
  float pk[8], pv[8];                              // the next stage's rows: one 8-channel group of K and one of V per thread
  const int kr = threadIdx.x >> 2, g = threadIdx.x & 3;
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) pk[e] = pv[e] = 0.f;
    if (k0 + kr < Tb) {
      load8<FMT>(qkv.ptr, (tok0 + k0 + kr) * qkv.cstride + chk + g * 8, pk);
      load8<FMT>(qkv.ptr, (tok0 + k0 + kr) * qkv.cstride + chv + g * 8, pv);
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < Tb; k0 += KS) {
    __syncthreads();
    {
      float* d = &s_k[kr * PK + g * 8];
      *reinterpret_cast<float4*>(d) = make_float4(pk[0], pk[1], pk[2], pk[3]);
      *reinterpret_cast<float4*>(d + 4) = make_float4(pk[4], pk[5], pk[6], pk[7]);
      d = &s_v[kr * PV + g * 8];
      *reinterpret_cast<float4*>(d) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      *reinterpret_cast<float4*>(d + 4) = make_float4(pv[4], pv[5], pv[6], pv[7]);
    }
    if (k0 + KS < Tb) fetch(k0 + KS);
    __syncthreads();
    const int nk = min(KS, Tb - k0);
    for (int t0 = 0; t0 < nk; t0 += 16) {
      floatx4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 8; ++i) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(s_k[(t0 + lc) * PK + 4 * i + kk], qf[i], sc, 0, 0, 0);
      float mx = -FLT_MAX;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (t0 + 4 * kk + r >= nk) sc[r] = -FLT_MAX;          // keys past the band's end
        mx = fmaxf(mx, sc[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));                     // key t0 is never masked: finite for every query column
      const float mn = fmaxf(m, mx), resc = __expf(m - mn);
      float p[4], ps = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) { p[r] = sc[r] > -FLT_MAX ? __expf(sc[r] - mn) : 0.f; ps += p[r]; }
      ps += __shfl_xor(ps, 16);
      ps += __shfl_xor(ps, 32);
      l = l * resc + ps;
      m = mn;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) o[t][r] *= resc;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vr = &s_v[(t0 + 4 * kk + r) * PV];
#pragma unroll
        for (int t = 0; t < 2; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[16 * t + lc], p[r], o[t], 0, 0, 0);
      }
    }
  }
  const int qi = q0 + lc;
  if (qi >= Tb) return;
  const float inv = 1.f / l;
  bool s = false;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int d = 16 * t + 4 * kk;                 // the lane's four channels of this tile
    const float r4[4] = {o[t][0] * inv, o[t][1] * inv, o[t][2] * inv, o[t][3] * inv};
    store4<FMT>(a.out.ptr, (tok0 + qi) * a.out.cstride + a.out.coff + head * 32 + d, r4, s);
  }
  flag_sat(sat, s);
}

template <int FMT>
__global__ __launch_bounds__(256) void scale_add_kernel(RtMap y, RtMap x, RtMap out, size_t pixels, const float* __restrict__ gamma, int* sat) {
  const int groups = y.c / 8;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= pixels * groups) return;
  const int g = (int)(t % groups);
  const size_t pix = t / groups;
  float vy[8], vx[8];
  load8<FMT>(y.ptr, pix * y.cstride + y.coff + g * 8, vy);
  load8<FMT>(x.ptr, pix * x.cstride + x.coff + g * 8, vx);
  const float4 g0 = *reinterpret_cast<const float4*>(gamma + g * 8), g1 = *reinterpret_cast<const float4*>(gamma + g * 8 + 4);
  const float gm[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) vx[j] = fmaf(gm[j], vy[j], vx[j]);
  bool s = false;
  store8<FMT>(out.ptr, pix * out.cstride + out.coff + g * 8, vx, s);
  flag_sat(sat, s);
}

}  // namespace

void launch_area_attention(int fmt, const RtMap& qkv, const RtMap& out, int n, int heads, int area, bool planar, int* sat, hipStream_t s) {
  GTX_CHECK(n > 0 && heads > 0 && qkv.c == heads * 96 && out.c == heads * 32 && qkv.h == out.h && qkv.w == out.w && qkv.h > 0 && qkv.w > 0,
            "area_attention: %d heads on %d -> %d channels", heads, qkv.c, out.c);
  GTX_CHECK(qkv.cstride % 8 == 0 && qkv.coff % 8 == 0 && out.cstride % 8 == 0 && out.coff % 8 == 0 && qkv.coff + qkv.c <= qkv.cstride && out.coff + out.c <= out.cstride,
            "area_attention: channel strides / offsets must be multiples of 8 and hold the slices");
  GTX_CHECK(area_attention_fits(qkv.h, qkv.w, area), "area_attention: a %d x %d map (%d positions) does not cut into %d equal areas", qkv.w, qkv.h, qkv.h * qkv.w, area);
  GTX_CHECK((long)heads * area <= 65535 && n <= 65535, "area_attention: %d heads x %d areas x %d images exceed the grid", heads, area, n);
  const int C = heads * 32;
  const AreaAttn a{qkv, out, heads, area, planar ? 32 : 96, planar ? C : 32, planar ? 2 * C : 64};
  const dim3 grid(cdiv(qkv.h * qkv.w / area, 64), heads * area, n);
  RT_FMT(fmt, hipLaunchKernelGGL(area_attn_kernel<F>, grid, dim3(256), 0, s, a, sat));
}

void launch_scale_add(int fmt, const RtMap& y, const RtMap& x, const RtMap& out, int n, const float* gamma, int* sat, hipStream_t s) {
  GTX_CHECK(n > 0 && y.c > 0 && y.c % 8 == 0 && x.c == y.c && out.c == y.c && x.h == y.h && x.w == y.w && out.h == y.h && out.w == y.w,
            "scale_add: maps of %d, %d and %d channels", y.c, x.c, out.c);
  GTX_CHECK(y.cstride % 8 == 0 && y.coff % 8 == 0 && x.cstride % 8 == 0 && x.coff % 8 == 0 && out.cstride % 8 == 0 && out.coff % 8 == 0,
            "scale_add: channel strides / offsets must be multiples of 8");
  const size_t pixels = (size_t)n * y.h * y.w, total = pixels * (y.c / 8);
  RT_FMT(fmt, hipLaunchKernelGGL(scale_add_kernel<F>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, y, x, out, pixels, gamma, sat));
}

}  // namespace gtx
