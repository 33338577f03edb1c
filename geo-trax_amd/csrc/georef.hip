// The per-row transform chain of the georeference stage in one pass:
//   frame pixel --H--> orthophoto pixel --affine geotransform--> latitude/longitude --transverse Mercator--> metres
// (geotrax/georeference.py:173-177 calling apply_homography :599-605, ortho2geo :608-615, geo2local :618-628).
// f64 throughout; one thread per point, structure-of-arrays in and out, so every access is a coalesced 8-B
// stream: 16 B in, up to 48 B out per point -- HBM-bound by construction, the ~40 f64 transcendental calls per
// point hide under it. The projection is the Krueger series to 6th order (sub-millimetre inside a zone); the
// reference gets the same numbers from pyproj.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "detector.hpp"
#include "geometry.hpp"

namespace gtx {

namespace {
struct ChainDev {
  double H[9];
  double ortho[6];        // lng0, lat0, dlng, dlat, skew_x, skew_y
  int projected;
  double lon0_rad, e, A, k0, fe, fn;
  double alpha[6];
};

// One point through the chain. east / north are written only for a projected chain.
__device__ __forceinline__ void chain_point(const ChainDev& c, double px, double py, double& u, double& v, double& la, double& lo,
                                            double& east, double& north) {
  // cv2.perspectiveTransform: w == 0 maps to (0, 0)
  const double w = c.H[6] * px + c.H[7] * py + c.H[8];
  const double s = fabs(w) > 2.220446049250313e-16 ? 1.0 / w : 0.0;
  u = (c.H[0] * px + c.H[1] * py + c.H[2]) * s;
  v = (c.H[3] * px + c.H[4] * py + c.H[5]) * s;
  la = c.ortho[1] + c.ortho[3] * v + c.ortho[5] * u;
  lo = c.ortho[0] + c.ortho[2] * u + c.ortho[4] * v;
  if (!c.projected) return;
  constexpr double kDeg = 0.017453292519943295;
  const double phi = la * kDeg, lam = lo * kDeg - c.lon0_rad;
  const double sp = sin(phi);
  const double t = sinh(atanh(sp) - c.e * atanh(c.e * sp));      // tangent of the conformal latitude
  const double cl = cos(lam);
  const double xi_p = atan2(t, cl), eta_p = asinh(sin(lam) / hypot(t, cl));
  double xi = xi_p, eta = eta_p;
#pragma unroll
  for (int j = 1; j <= 6; ++j) {
    xi += c.alpha[j - 1] * sin(2 * j * xi_p) * cosh(2 * j * eta_p);
    eta += c.alpha[j - 1] * cos(2 * j * xi_p) * sinh(2 * j * eta_p);
  }
  east = c.fe + c.k0 * (c.A * eta);
  north = c.fn + c.k0 * (c.A * xi);
}

__global__ __launch_bounds__(256) void georef_points_kernel(const ChainDev c, const double* __restrict__ x, const double* __restrict__ y,
                                                            int n, double* __restrict__ ox, double* __restrict__ oy,
                                                            double* __restrict__ lat, double* __restrict__ lon,
                                                            double* __restrict__ east, double* __restrict__ north) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double u, v, la, lo, e = 0.0, nn = 0.0;
  chain_point(c, x[i], y[i], u, v, la, lo, e, nn);
  if (ox) ox[i] = u;
  if (oy) oy[i] = v;
  if (lat) lat[i] = la;
  if (lon) lon[i] = lo;
  if (!c.projected) return;
  if (east) east[i] = e;
  if (north) north[i] = nn;
}

// The chain's constants from the ABI's parameter block.
ChainDev make_chain(const gtx_georef_chain& ch) {
  ChainDev c{};
  for (int i = 0; i < 9; ++i) c.H[i] = ch.H[i];
  for (int i = 0; i < 6; ++i) c.ortho[i] = ch.ortho[i];
  c.projected = ch.projected;
  if (ch.projected) {
    GTX_CHECK(ch.flattening > 0 && ch.flattening < 0.1 && ch.semi_major > 0, "georef_points: ellipsoid a=%g f=%g", ch.semi_major, ch.flattening);
    const double f = ch.flattening, nn = f / (2 - f);
    const double n2 = nn * nn, n3 = n2 * nn, n4 = n2 * n2, n5 = n4 * nn, n6 = n3 * n3;
    c.A = ch.semi_major / (1 + nn) * (1 + n2 / 4 + n4 / 64 + n6 / 256);
    c.alpha[0] = nn / 2 - 2 * n2 / 3 + 5 * n3 / 16 + 41 * n4 / 180 - 127 * n5 / 288 + 7891 * n6 / 37800;
    c.alpha[1] = 13 * n2 / 48 - 3 * n3 / 5 + 557 * n4 / 1440 + 281 * n5 / 630 - 1983433 * n6 / 1935360;
    c.alpha[2] = 61 * n3 / 240 - 103 * n4 / 140 + 15061 * n5 / 26880 + 167603 * n6 / 181440;
    c.alpha[3] = 49561 * n4 / 161280 - 179 * n5 / 168 + 6601661 * n6 / 7257600;
    c.alpha[4] = 34729 * n5 / 80640 - 3418889 * n6 / 1995840;
    c.alpha[5] = 212378941 * n6 / 319334400;
    c.e = std::sqrt(f * (2 - f));
    c.lon0_rad = ch.lon0_deg * 0.017453292519943295;
    c.k0 = ch.k0; c.fe = ch.false_easting; c.fn = ch.false_northing;
  }
  return c;
}
}  // namespace

void georef_points(gtx_ctx* ctx, const gtx_georef_chain& ch, const double* x, const double* y, int n, double* ox, double* oy,
                   double* lat, double* lon, double* east, double* north) {
  GTX_CHECK(n >= 0, "georef_points: n = %d", n);
  if (n == 0) return;
  GTX_HIP(hipSetDevice(ctx->device));
  const ChainDev c = make_chain(ch);
  const size_t bytes = sizeof(double) * (size_t)n;
  double* outs_h[6] = {ox, oy, lat, lon, ch.projected ? east : nullptr, ch.projected ? north : nullptr};
  int n_out = 0;
  for (double* p : outs_h) n_out += p != nullptr;
  DevBuf din(2 * bytes), dout(std::max<size_t>(n_out, 1) * bytes);
  hipStream_t s = ctx->stream;
  GTX_HIP(hipMemcpyAsync(din.p, x, bytes, hipMemcpyHostToDevice, s));
  GTX_HIP(hipMemcpyAsync(din.as<double>() + n, y, bytes, hipMemcpyHostToDevice, s));
  double* outs_d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int k = 0, j = 0; k < 6; ++k)
    if (outs_h[k]) outs_d[k] = dout.as<double>() + (size_t)(j++) * n;
  hipLaunchKernelGGL(georef_points_kernel, dim3(cdiv(n, 256)), dim3(256), 0, s, c, din.as<double>(), din.as<double>() + n, n, outs_d[0],
                     outs_d[1], outs_d[2], outs_d[3], outs_d[4], outs_d[5]);
  GTX_HIP(hipGetLastError());
  for (int k = 0; k < 6; ++k)
    if (outs_h[k]) GTX_HIP(hipMemcpyAsync(outs_h[k], outs_d[k], bytes, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------------------------------------------------------------------
// The stage's per-track columns (gtx_op_georef_tracks): what geotrax_amd/georeference.py computes on the host after
// the chain -- calculate_visibility, convert_dimensions, compute_kinematics, assign_road_section_lane -- on the table where the
// chain left it. The host's plan (rows sorted by track, segment bounds, used rows and gap-filled length per track) fixes where
// everything goes; nothing is appended through a counter, so two runs write the same bits. Nine launches:
//   rows     chain (the kernel above), visibility (+ NaN into speed / accel), lanes
//   tracks   dimensions (one lane per track), compaction (one workgroup per track: use-mask, block scan, then a second scan over the
//            used rows' frame gaps for each sample's place in the gap-filled series; both totals are checked against the plan)
//   samples  gap fill (one lane per used row writes its sample and the fills in front of it), acceleration + scatter
//   series   speed, correlate (one lane per point of the concatenated series; a binary search over the plan's offsets finds the track)
// A track's series lives in HBM scratch whatever its length; the correlate kernel's 2 * radius + 1 reads per point are neighbouring
// lanes' reads shifted by one, which L1 / L2 serve -- no LDS staging (an hour-long track would not fit, a 150-point one gains nothing
// measurable next to the launches, tools/georef_tracks_time.py). numpy's and scipy's operation sequences are kept, one rounding per
// operation, hence no contraction from here on:
#pragma clang fp contract(off)

namespace {
struct TracksDev {
  int n, n_tracks, n_used_total, n_exp, n_quads, radius, symmetric, boundary;
  const double *bbox, *dims, *quads, *weights;
  const int *frame, *interp, *order, *seg, *n_used, *used_off, *exp_off;
  double *ox, *oy, *xl, *yl;                                   // the chain's outputs
  unsigned char* vis;
  double *length_m, *width_m, *speed, *accel;
  int* quad;
  int *cidx, *ctrack, *epos, *ok, *err;                        // per used row: its table row, its track, its place in the series
  double *xs, *ys, *sp, *sv, *tl, *tw;                         // series scratch (positions, speed, smoothed speed); per-track dimensions
  double margin, x_lim, y_lim, cx, cy, fps, conv;
};

__device__ __forceinline__ double dev_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// calculate_visibility, one lane per row; speed / accel start as NaN (rows the kinematics never reach keep it)
__global__ __launch_bounds__(256) void tracks_visibility_kernel(const TracksDev p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const double x = p.bbox[4 * (size_t)i], y = p.bbox[4 * (size_t)i + 1], w = p.bbox[4 * (size_t)i + 2], h = p.bbox[4 * (size_t)i + 3];
  const bool v = (x - w / 2 > p.margin) && (x + w / 2 < p.x_lim) && (y - h / 2 > p.margin) && (y + h / 2 < p.y_lim);
  p.vis[i] = v ? 1 : 0;
  p.speed[i] = dev_nan();
  p.accel[i] = dev_nan();
}

// convert_dimensions, one lane per track: the first row in file order decides (the stable sort puts it first in the segment)
__global__ __launch_bounds__(256) void tracks_dims_kernel(const TracksDev p, const ChainDev c) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= p.n_tracks) return;
  const int row = p.order[p.seg[t]];
  const double l = p.dims[2 * (size_t)row], w = p.dims[2 * (size_t)row + 1];
  double len = dev_nan(), wid = dev_nan();
  if (!isnan(l) && !isnan(w)) {
    double u, v, la, lo, e0 = 0, n0 = 0, e1 = 0, n1 = 0, e2 = 0, n2 = 0;
    chain_point(c, p.cx, p.cy, u, v, la, lo, e0, n0);
    chain_point(c, p.cx, p.cy + w / 2, u, v, la, lo, e1, n1);
    chain_point(c, p.cx + l / 2, p.cy, u, v, la, lo, e2, n2);
    const double lx = e0 - e2, ly = n0 - n2, wx = e0 - e1, wy = n0 - n1;
    len = 2 * sqrt(lx * lx + ly * ly);
    wid = 2 * sqrt(wx * wx + wy * wy);
  }
  p.tl[t] = len;
  p.tw[t] = wid;
}

// inclusive scan over the workgroup's 256 lanes (4 waves of 64); every lane calls it
__device__ __forceinline__ long long block_scan_incl(long long v, long long* wsum, long long& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long y = __shfl_up(v, d);
    if (lane >= d) v += y;
  }
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  long long off = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long s = wsum[k];
    if (k < wave) off += s;
    total += s;
  }
  __syncthreads();                                             // wsum is written again by the next call
  return v + off;
}

// One workgroup per track: broadcast of the dimensions, use = visibility & (is_interpolated == 0), the used rows compacted in
// order into cidx / ctrack at the plan's offset, then every used row's place in the gap-filled series (epos). A slot past the
// plan's count is never written; a count or a series length that differs from the plan marks the track (ok = 0, err = track + 1).
__global__ __launch_bounds__(256) void tracks_compact_kernel(const TracksDev p) {
  __shared__ long long wsum[4];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int s0 = p.seg[t], s1 = p.seg[t + 1], nu = p.n_used[t], uo = p.used_off[t];
  const double len = p.tl[t], wid = p.tw[t];
  long long running = 0;
  for (int base = s0; base < s1; base += 256) {
    const int i = base + tid;
    const int row = i < s1 ? p.order[i] : -1;
    bool use = false;
    if (row >= 0) {
      p.length_m[row] = len;
      p.width_m[row] = wid;
      use = p.vis[row] != 0 && (p.interp == nullptr || p.interp[row] == 0);
    }
    long long total;
    const long long k = running + block_scan_incl(use ? 1 : 0, wsum, total) - 1;
    if (use && k < nu) {
      p.cidx[uo + k] = row;
      p.ctrack[uo + k] = t;
    }
    running += total;
  }
  if (running != nu) {
    if (tid == 0) { p.ok[t] = 0; atomicMax(p.err, t + 1); }
    return;
  }
  if (nu < 3) {                                                 // compute_kinematics skips the track: its rows keep NaN
    if (tid == 0) p.ok[t] = 0;
    return;
  }
  __syncthreads();                                              // cidx as this workgroup wrote it
  long long carry = 0;
  for (int base = 0; base < nu; base += 256) {
    const int j = base + tid;
    long long per = 0;
    if (j > 0 && j < nu) {
      const long long gap = (long long)p.frame[p.cidx[uo + j]] - (long long)p.frame[p.cidx[uo + j - 1]];
      per = gap > 1 ? gap : 1;                                  // its fills, then the sample; a repeated frame number adds one point
    }
    long long total;
    const long long pos = carry + block_scan_incl(per, wsum, total);
    if (j < nu) p.epos[uo + j] = (int)(pos < 0x7fffffffll ? pos : 0x7fffffffll);
    carry += total;
  }
  const bool good = carry + 1 == (long long)p.exp_off[t + 1] - (long long)p.exp_off[t];
  if (tid == 0) {
    p.ok[t] = good ? 1 : 0;
    if (!good) atomicMax(p.err, t + 1);
  }
}

// interpolate_missing_points, one lane per used row: its own sample, and in front of it the fills of the frames skipped since the
// track's previous used row: x[i-1] + step * ((x[i] - x[i-1]) / gap)
__global__ __launch_bounds__(256) void tracks_fill_kernel(const TracksDev p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n_used_total) return;
  const int t = p.ctrack[j];
  if (t < 0 || !p.ok[t]) return;
  const int base = p.exp_off[t], row = p.cidx[j], pj = p.epos[j];
  const double x = p.xl[row], y = p.yl[row];
  p.xs[base + pj] = x;
  p.ys[base + pj] = y;
  if (j == p.used_off[t]) return;
  const int prev = p.cidx[j - 1];
  const long long gap = (long long)p.frame[row] - (long long)p.frame[prev];
  if (gap <= 1) return;
  const int pp = p.epos[j - 1];                                 // pp + gap == pj: the compaction kernel checked the sum
  const double x0 = p.xl[prev], y0 = p.yl[prev];
  const double dx = (x - x0) / (double)gap, dy = (y - y0) / (double)gap;
  for (long long step = 1; step < gap; ++step) {
    p.xs[base + pp + step] = x0 + (double)step * dx;
    p.ys[base + pp + step] = y0 + (double)step * dy;
  }
}

// the track whose series holds point g of the concatenated series: exp_off[t] <= g < exp_off[t + 1] (tracks without a series have
// an empty range and are never found)
__device__ __forceinline__ int series_track(const TracksDev& p, int g) {
  int lo = 0, hi = p.n_tracks;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (p.exp_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// compute_speed over the gap-filled series: sqrt(dx^2 + dy^2) * fps, one value less than points
__global__ __launch_bounds__(256) void tracks_speed_kernel(const TracksDev p) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.n_exp) return;
  const int t = series_track(p, g);
  if (!p.ok[t] || g + 1 >= p.exp_off[t + 1]) return;
  const double dx = p.xs[g + 1] - p.xs[g], dy = p.ys[g + 1] - p.ys[g];
  p.sp[g] = sqrt(dx * dx + dy * dy) * p.fps;
}

// sample i of a series of m values continued past its ends: half-sample symmetric reflection with period 2 m, or the end value
__device__ __forceinline__ double series_at(const double* in, int i, int m, int boundary) {
  if (i < 0 || i >= m) {
    if (boundary == 1) {
      i = i < 0 ? 0 : m - 1;
    } else {
      const int period = 2 * m;
      i %= period;
      if (i < 0) i += period;
      if (i >= m) i = period - 1 - i;
    }
  }
  return in[i];
}

// apply_filter: each track's speed series correlated with the host's weights (LDS) in scipy.ndimage.correlate1d's order
__global__ __launch_bounds__(256) void tracks_correlate_kernel(const TracksDev p) {
  extern __shared__ double w_lds[];
  const int r = p.radius;
  for (int k = threadIdx.x; k <= 2 * r; k += blockDim.x) w_lds[k] = p.weights[k];
  __syncthreads();
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= p.n_exp) return;
  const int t = series_track(p, g);
  if (!p.ok[t]) return;
  const int base = p.exp_off[t], m = p.exp_off[t + 1] - base - 1, e = g - base;
  if (e >= m) return;
  const double* in = p.sp + base;
  double acc;
  if (p.symmetric) {
    acc = in[e] * w_lds[r];
    if (e - r >= 0 && e + r < m) {
      for (int k = r; k >= 1; --k) acc += (in[e - k] + in[e + k]) * w_lds[r - k];
    } else {
      for (int k = r; k >= 1; --k) acc += (series_at(in, e - k, m, p.boundary) + series_at(in, e + k, m, p.boundary)) * w_lds[r - k];
    }
  } else {
    acc = series_at(in, e + r, m, p.boundary) * w_lds[2 * r];
    for (int k = -r; k < r; ++k) acc += series_at(in, e + k, m, p.boundary) * w_lds[r + k];
  }
  p.sv[g] = acc;
}

// compute_acceleration and the scatter back to the table, one lane per used row: the series with a NaN in front (speed) or two
// (acceleration), read at the sample's place
__global__ __launch_bounds__(256) void tracks_scatter_kernel(const TracksDev p) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= p.n_used_total) return;
  const int t = p.ctrack[j];
  if (t < 0 || !p.ok[t]) return;
  const int row = p.cidx[j], pos = p.epos[j];
  const double* v = p.sv + p.exp_off[t];
  p.speed[row] = pos >= 1 ? v[pos - 1] * p.conv : dev_nan();
  p.accel[row] = pos >= 2 ? (v[pos - 1] - v[pos - 2]) * p.fps : dev_nan();
}

// assign_road_section_lane, one lane per row over the quads in LDS: _points_in_quad's rule (crossing parity with px < xint, points
// with cross == 0 inside an edge's bounding box excluded), the first containing quad in file order
__global__ __launch_bounds__(256) void tracks_lanes_kernel(const TracksDev p) {
  extern __shared__ double q_lds[];
  for (int k = threadIdx.x; k < 8 * p.n_quads; k += blockDim.x) q_lds[k] = p.quads[k];
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const double px = p.ox[i], py = p.oy[i];
  int found = -1;
  for (int q = 0; q < p.n_quads && found < 0; ++q) {
    const double* c = q_lds + 8 * q;
    bool inside = false, on_edge = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double x1 = c[2 * k], y1 = c[2 * k + 1], x2 = c[2 * ((k + 1) & 3)], y2 = c[2 * ((k + 1) & 3) + 1];
      const double cross = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1);
      const bool within = fmin(x1, x2) <= px && px <= fmax(x1, x2) && fmin(y1, y2) <= py && py <= fmax(y1, y2);
      on_edge |= cross == 0 && within;
      const bool straddles = (y1 > py) != (y2 > py);
      const double xint = x1 + (py - y1) * (x2 - x1) / (y2 - y1);
      inside ^= straddles && px < xint;
    }
    if (inside && !on_edge) found = q;
  }
  p.quad[i] = found;
}

// the timing events of one call; create() may throw half way: the destructor of the (complete) object releases what exists
struct Events {
  hipEvent_t e[GTX_GEOREF_TRACKS_MS] = {};
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  void create() { for (auto& v : e) GTX_HIP(hipEventCreate(&v)); }
  ~Events() { for (auto v : e) if (v) (void)hipEventDestroy(v); }
};
thread_local float g_tracks_ms[GTX_GEOREF_TRACKS_MS] = {};
}  // namespace

void georef_tracks_last_ms(float* ms) { std::memcpy(ms, g_tracks_ms, sizeof g_tracks_ms); }

void georef_tracks(gtx_ctx* ctx, const gtx_georef_chain& ch, const gtx_georef_tracks_cfg& cfg, const GeorefTracksArgs& a) {
  std::memset(g_tracks_ms, 0, sizeof g_tracks_ms);
  const int n = a.n, T = cfg.n_tracks;
  if (n == 0) return;
  GTX_HIP(hipSetDevice(ctx->device));
  const ChainDev c = make_chain(ch);
  std::vector<int> used_off((size_t)T + 1, 0);
  for (int t = 0; t < T; ++t) used_off[t + 1] = used_off[t] + a.n_used[t];
  const int U = used_off[T], E = a.exp_off[T];

  size_t room = 0;
  auto take = [&room](size_t bytes) { const size_t o = room; room += (bytes + 255) / 256 * 256; return o; };
  const size_t nd = sizeof(double) * (size_t)n, ni = sizeof(int) * (size_t)n;
  const size_t o_x = take(nd), o_y = take(nd), o_bbox = take(4 * nd), o_dims = take(2 * nd), o_frame = take(ni), o_interp = take(ni),
               o_order = take(ni), o_seg = take(sizeof(int) * ((size_t)T + 1)), o_nused = take(sizeof(int) * (size_t)T),
               o_uoff = take(sizeof(int) * ((size_t)T + 1)), o_eoff = take(sizeof(int) * ((size_t)T + 1)),
               o_quads = take(sizeof(double) * 8 * (size_t)a.n_quads), o_w = take(sizeof(double) * (size_t)a.n_weights);
  size_t o_out[10];                                              // ox, oy, lat, lon, east, north, length, width, speed, accel
  for (auto& o : o_out) o = take(nd);
  const size_t o_vis = take((size_t)n), o_quad = take(ni), o_cidx = take(sizeof(int) * (size_t)U), o_ctrack = take(sizeof(int) * (size_t)U),
               o_epos = take(sizeof(int) * (size_t)U), o_ok = take(sizeof(int) * (size_t)T), o_err = take(sizeof(int)),
               o_xs = take(sizeof(double) * (size_t)E), o_ys = take(sizeof(double) * (size_t)E), o_sp = take(sizeof(double) * (size_t)E),
               o_sv = take(sizeof(double) * (size_t)E), o_tl = take(sizeof(double) * (size_t)T), o_tw = take(sizeof(double) * (size_t)T);
  DevBuf buf(room);
  char* base = buf.as<char>();
  auto D = [base](size_t o) { return reinterpret_cast<double*>(base + o); };
  auto I = [base](size_t o) { return reinterpret_cast<int*>(base + o); };

  TracksDev p{};
  p.n = n; p.n_tracks = T; p.n_used_total = U; p.n_exp = E; p.n_quads = a.n_quads;
  p.radius = a.n_weights / 2; p.symmetric = a.symmetric; p.boundary = cfg.boundary;
  p.bbox = D(o_bbox); p.dims = D(o_dims); p.quads = D(o_quads); p.weights = D(o_w);
  p.frame = I(o_frame); p.interp = a.interp ? I(o_interp) : nullptr; p.order = I(o_order); p.seg = I(o_seg); p.n_used = I(o_nused);
  p.used_off = I(o_uoff); p.exp_off = I(o_eoff);
  p.ox = D(o_out[0]); p.oy = D(o_out[1]); p.xl = D(o_out[4]); p.yl = D(o_out[5]);
  p.vis = reinterpret_cast<unsigned char*>(base + o_vis);
  p.length_m = D(o_out[6]); p.width_m = D(o_out[7]); p.speed = D(o_out[8]); p.accel = D(o_out[9]);
  p.quad = I(o_quad); p.cidx = I(o_cidx); p.ctrack = I(o_ctrack); p.epos = I(o_epos); p.ok = I(o_ok); p.err = I(o_err);
  p.xs = D(o_xs); p.ys = D(o_ys); p.sp = D(o_sp); p.sv = D(o_sv); p.tl = D(o_tl); p.tw = D(o_tw);
  p.margin = (double)cfg.visibility_margin;
  p.x_lim = (double)(cfg.frame_w - cfg.visibility_margin - 1);
  p.y_lim = (double)(cfg.frame_h - cfg.visibility_margin - 1);
  p.cx = (double)cfg.frame_w / 2; p.cy = (double)cfg.frame_h / 2;
  p.fps = cfg.fps; p.conv = cfg.conversion_factor;

  hipStream_t s = ctx->stream;
  Events ev;
  ev.create();
  int ne = 0;
  auto mark = [&] { GTX_HIP(hipEventRecord(ev.e[ne++], s)); };
  auto up = [&](size_t o, const void* src, size_t bytes) { if (bytes) GTX_HIP(hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, s)); };
  mark();
  up(o_x, a.x, nd); up(o_y, a.y, nd); up(o_bbox, a.bbox, 4 * nd); up(o_dims, a.dims, 2 * nd); up(o_frame, a.frame, ni);
  if (a.interp) up(o_interp, a.interp, ni);
  up(o_order, a.order, ni); up(o_seg, a.seg, sizeof(int) * ((size_t)T + 1)); up(o_nused, a.n_used, sizeof(int) * (size_t)T);
  up(o_uoff, used_off.data(), sizeof(int) * ((size_t)T + 1)); up(o_eoff, a.exp_off, sizeof(int) * ((size_t)T + 1));
  up(o_quads, a.quads, sizeof(double) * 8 * (size_t)a.n_quads); up(o_w, a.weights, sizeof(double) * (size_t)a.n_weights);
  if (U > 0) GTX_HIP(hipMemsetAsync(base + o_ctrack, 0xFF, sizeof(int) * (size_t)U, s));   // -1: a slot the compaction did not reach
  GTX_HIP(hipMemsetAsync(base + o_err, 0, sizeof(int), s));
  mark();
  const dim3 blk(256), rows(cdiv(n, 256));
  hipLaunchKernelGGL(georef_points_kernel, rows, blk, 0, s, c, D(o_x), D(o_y), n, D(o_out[0]), D(o_out[1]), D(o_out[2]), D(o_out[3]), D(o_out[4]),
                     D(o_out[5]));
  mark();
  hipLaunchKernelGGL(tracks_visibility_kernel, rows, blk, 0, s, p);
  mark();
  hipLaunchKernelGGL(tracks_dims_kernel, dim3(cdiv(T, 256)), blk, 0, s, p, c);
  mark();
  hipLaunchKernelGGL(tracks_compact_kernel, dim3(T), blk, 0, s, p);
  mark();
  if (U > 0) hipLaunchKernelGGL(tracks_fill_kernel, dim3(cdiv(U, 256)), blk, 0, s, p);
  mark();
  if (E > 0) hipLaunchKernelGGL(tracks_speed_kernel, dim3(cdiv(E, 256)), blk, 0, s, p);
  mark();
  if (E > 0) hipLaunchKernelGGL(tracks_correlate_kernel, dim3(cdiv(E, 256)), blk, sizeof(double) * (size_t)a.n_weights, s, p);
  mark();
  if (U > 0) hipLaunchKernelGGL(tracks_scatter_kernel, dim3(cdiv(U, 256)), blk, 0, s, p);
  mark();
  hipLaunchKernelGGL(tracks_lanes_kernel, rows, blk, sizeof(double) * 8 * (size_t)std::max(a.n_quads, 1), s, p);
  GTX_HIP(hipGetLastError());
  mark();
  int err = 0;
  GTX_HIP(hipMemcpyAsync(&err, base + o_err, sizeof(int), hipMemcpyDeviceToHost, s));
  double* outs_h[10] = {a.ox, a.oy, a.lat, a.lon, a.east, a.north, a.length_m, a.width_m, a.speed, a.accel};
  for (int k = 0; k < 10; ++k)
    if (outs_h[k]) GTX_HIP(hipMemcpyAsync(outs_h[k], base + o_out[k], nd, hipMemcpyDeviceToHost, s));
  if (a.vis) GTX_HIP(hipMemcpyAsync(a.vis, base + o_vis, (size_t)n, hipMemcpyDeviceToHost, s));
  if (a.quad) GTX_HIP(hipMemcpyAsync(a.quad, base + o_quad, ni, hipMemcpyDeviceToHost, s));
  mark();
  GTX_HIP(hipStreamSynchronize(s));
  float kernels = 0.f;
  for (int k = 0; k < 9; ++k) {
    GTX_HIP(hipEventElapsedTime(&g_tracks_ms[k], ev.e[k + 1], ev.e[k + 2]));
    kernels += g_tracks_ms[k];
  }
  GTX_HIP(hipEventElapsedTime(&g_tracks_ms[9], ev.e[0], ev.e[1]));
  GTX_HIP(hipEventElapsedTime(&g_tracks_ms[10], ev.e[10], ev.e[11]));
  g_tracks_ms[11] = kernels;
  if (err) fail(GTX_ERR_INVALID, "georef_tracks: the plan does not fit the table: track %d of %d has another count of used rows or another "
                                 "gap-filled length than n_used / exp_off say", err - 1, T);
}

}  // namespace gtx
