// The host half of the robust homography solver (homography.hpp): plain C++, f64, no GPU.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "homography.hpp"

namespace gtx {

// Robust refinement of the RANSAC winner. Keypoints sit on integer pixels of their pyramid level,
// so matches carry 1-2 px of localisation noise in full-resolution pixels -- comparable to the
// RANSAC threshold. A hard inlier cut at the threshold throws away (and biases) much of the
// evidence. Instead: keep every match within 3x the threshold of the winner and minimise the
// geometric transfer error with iteratively re-weighted Gauss-Newton (Tukey biweight, scale from
// the median residual), h33 = 1, in normalised coordinates.
bool refine_homography(const float* pairs, int n_pairs, int frame_w, int frame_h, double thr, bool affine, const double H0[9], double Hout[9],
                       int* n_inliers) {
  const FrameNorm norm(frame_w, frame_h);
  const double cx = norm.cx, cy = norm.cy, sc = norm.sc;
  const size_t n = (size_t)n_pairs;
  const int np = affine ? 6 : 8;                     // affine: h31 = h32 = 0 stay as they are, six parameters move
  const size_t min_pts = affine ? 3 : 4;
  double H[9];
  std::memcpy(H, H0, sizeof H);
  const double inv0 = 1.0 / H[8];
  for (double& v : H) v *= inv0;
  // to normalised coordinates: Hn = T H T^-1
  auto to_norm = [&](const double* Hp, double* Hn) {
    const double is = 1.0 / sc;
    double M[9];  // M = H T^-1, T^-1 = [[is,0,cx],[0,is,cy],[0,0,1]]
    for (int r = 0; r < 3; ++r) {
      M[r * 3 + 0] = Hp[r * 3 + 0] * is;
      M[r * 3 + 1] = Hp[r * 3 + 1] * is;
      M[r * 3 + 2] = Hp[r * 3 + 0] * cx + Hp[r * 3 + 1] * cy + Hp[r * 3 + 2];
    }
    for (int k = 0; k < 3; ++k) {  // Hn = T M, T = [[sc,0,-sc cx],[0,sc,-sc cy],[0,0,1]]
      Hn[0 + k] = sc * M[0 + k] - sc * cx * M[6 + k];
      Hn[3 + k] = sc * M[3 + k] - sc * cy * M[6 + k];
      Hn[6 + k] = M[6 + k];
    }
    const double inv = 1.0 / Hn[8];
    for (int i = 0; i < 9; ++i) Hn[i] *= inv;
  };
  auto from_norm = [&](const double* Hn, double* Hp) {
    const double is = 1.0 / sc;
    double M[9];  // M = Hn T
    for (int r = 0; r < 3; ++r) {
      M[r * 3 + 0] = Hn[r * 3 + 0] * sc;
      M[r * 3 + 1] = Hn[r * 3 + 1] * sc;
      M[r * 3 + 2] = Hn[r * 3 + 2] - sc * (Hn[r * 3 + 0] * cx + Hn[r * 3 + 1] * cy);
    }
    for (int k = 0; k < 3; ++k) {
      Hp[0 + k] = is * M[0 + k] + cx * M[6 + k];
      Hp[3 + k] = is * M[3 + k] + cy * M[6 + k];
      Hp[6 + k] = M[6 + k];
    }
    const double inv = 1.0 / Hp[8];
    for (int i = 0; i < 9; ++i) Hp[i] *= inv;
  };
  std::vector<double> x(n), y(n), u(n), v(n);
  for (size_t i = 0; i < n; ++i) {
    const float* p = pairs + 4 * i;
    x[i] = (p[0] - cx) * sc; y[i] = (p[1] - cy) * sc;
    u[i] = (p[2] - cx) * sc; v[i] = (p[3] - cy) * sc;
  }
  double h[9];
  to_norm(H, h);
  auto residual = [&](size_t i, double& rx, double& ry, double& w) {
    w = h[6] * x[i] + h[7] * y[i] + 1.0;
    rx = (h[0] * x[i] + h[1] * y[i] + h[2]) / w - u[i];
    ry = (h[3] * x[i] + h[4] * y[i] + h[5]) / w - v[i];
  };
  // support set: within 3 thresholds of the winner (fixed over the iterations)
  std::vector<int> sup;
  const double lim = 3.0 * thr * sc;
  for (size_t i = 0; i < n; ++i) {
    double rx, ry, w;
    residual(i, rx, ry, w);
    if (std::fabs(w) > 1e-9 && rx * rx + ry * ry <= lim * lim) sup.push_back((int)i);
  }
  if (sup.size() < min_pts) return false;
  std::vector<double> un(sup.size());
  for (int iter = 0; iter < 8; ++iter) {
    for (size_t k = 0; k < sup.size(); ++k) {
      double rx, ry, w;
      residual(sup[k], rx, ry, w);
      un[k] = std::sqrt(rx * rx + ry * ry) / sc;   // pixels
    }
    std::vector<double> tmp = un;
    std::nth_element(tmp.begin(), tmp.begin() + tmp.size() / 2, tmp.end());
    const double sigma = std::max(1.4826 * tmp[tmp.size() / 2], 0.05);
    const double c = 4.685 * sigma;
    double A[64] = {0}, g[8] = {0};
    for (size_t k = 0; k < sup.size(); ++k) {
      const int i = sup[k];
      if (un[k] >= c) continue;
      const double t = 1.0 - (un[k] / c) * (un[k] / c);
      const double wt = t * t;
      double rx, ry, w;
      residual(i, rx, ry, w);
      const double iw = 1.0 / w, px = rx + u[i], py = ry + v[i];
      const double Jx[8] = {x[i] * iw, y[i] * iw, iw, 0, 0, 0, -px * x[i] * iw, -px * y[i] * iw};
      const double Jy[8] = {0, 0, 0, x[i] * iw, y[i] * iw, iw, -py * x[i] * iw, -py * y[i] * iw};
      for (int a = 0; a < np; ++a) {
        g[a] += wt * (Jx[a] * rx + Jy[a] * ry);
        for (int b = a; b < np; ++b) A[a * 8 + b] += wt * (Jx[a] * Jx[b] + Jy[a] * Jy[b]);
      }
    }
    for (int a = 0; a < np; ++a)
      for (int b = 0; b < a; ++b) A[a * 8 + b] = A[b * 8 + a];
    // Cholesky solve A d = g
    double Lc[64] = {0};
    bool ok = true;
    for (int i = 0; i < np && ok; ++i)
      for (int j = 0; j <= i; ++j) {
        double s = A[i * 8 + j];
        for (int k = 0; k < j; ++k) s -= Lc[i * 8 + k] * Lc[j * 8 + k];
        if (i == j) {
          if (!(s > 0)) { ok = false; break; }
          Lc[i * 8 + i] = std::sqrt(s);
        } else {
          Lc[i * 8 + j] = s / Lc[j * 8 + j];
        }
      }
    if (!ok) break;
    double yv[8], d[8];
    for (int i = 0; i < np; ++i) {
      double s = g[i];
      for (int k = 0; k < i; ++k) s -= Lc[i * 8 + k] * yv[k];
      yv[i] = s / Lc[i * 8 + i];
    }
    for (int i = np - 1; i >= 0; --i) {
      double s = yv[i];
      for (int k = i + 1; k < np; ++k) s -= Lc[k * 8 + i] * d[k];
      d[i] = s / Lc[i * 8 + i];
    }
    double step = 0;
    for (int a = 0; a < np; ++a) { h[a] -= d[a]; step = std::max(step, std::fabs(d[a])); }
    if (step < 1e-14) break;
  }
  from_norm(h, H);
  int cnt = 0;
  const double t2 = thr * sc * thr * sc;
  for (size_t i = 0; i < n; ++i) {
    double rx, ry, w;
    residual(i, rx, ry, w);
    if (rx * rx + ry * ry <= t2) ++cnt;
  }
  if (n_inliers) *n_inliers = cnt;
  if (cnt < (int)min_pts) return false;
  std::memcpy(Hout, H, sizeof H);
  return true;
}

}  // namespace gtx
