// The least-squares plane of ef_map_planes' refinement (ef_planes.inc: k_plane_fit): from the nine double sums over the
// winner's inliers to the refined model.  It compiles for the host and the device (as ef_unionfind.hpp does): tests/plane_fit_main.cpp runs
// the same text under g++ -ffp-contract=off, and tests/planeref.py restates it line by line in Python floats (IEEE doubles).
//   ARITHMETIC  only +, -, *, / and sqrt in double, each correctly rounded on every target and never contracted, in the written order: the
//               result is the same bits wherever it runs.  No library call but the square root, no fabs, no comparison that a NaN could turn:
//               every test is written so that a NaN takes the "give up" side.
//   INPUT       S[0..2] = sums of q.x, q.y, q.z; S[3..8] = sums of xx, xy, xz, yy, yz, zz with q = (double)p - (double)a over the m inliers; a =
//               the anchor (the winner's first sample); hn, hd = the winning hypothesis's plane.
//   METHOD      mean = S1 / m, C_ij = S2_ij / m - mean_i * mean_j; a cyclic Jacobi eigen-decomposition of C with EF_PLANE_FIT_SWEEPS sweeps over
//               the pairs (0,1), (0,2), (1,2) (a 3 x 3 symmetric matrix is diagonal to rounding after five; the number is fixed so that nothing
//               depends on a convergence test); the normal is the eigenvector of the smallest eigenvalue (ties: the lowest index), normalised,
//               flipped to the hypothesis's side; d = -(n . (a + mean)).
//   OUTPUT      false, and nothing written, when m < 3 or anything along the way is not finite: the caller keeps the hypothesis's plane.
//   PARTS       plane_fit_eigen (the moments to the diagonalised A, V) and plane_fit_normal (the choice, the normalisation, the flip) are shared
//               with normal_fit, the per-surfel fit of ef_map_normals, and with smooth_fit at the end of this file, the weighted per-surfel fit
//               of ef_map_smooth; plane_fit adds the offset and the thickness.
#pragma once

#if defined(__HIPCC__)
#define EF_PF_HD __host__ __device__ __forceinline__
#else
#define EF_PF_HD inline
#endif

namespace efm {

constexpr int EF_PLANE_FIT_SWEEPS = 8;

EF_PF_HD bool plane_fit_finite(double x) { return x - x == 0.0; }   // false for an infinity and for a NaN

// One Jacobi rotation in the plane (p, q), p < q, r the third index: A <- J^T A J, V <- V J (the classical formulas: Rutishauser's update of the
// two diagonal entries by t * a_pq, the off-diagonal pair through c and s).  a_pq == 0 (or NaN: the comparison is false) rotates nothing.
EF_PF_HD void plane_fit_rotate(double A[3][3], double V[3][3], int p, int q, int r) {
  const double apq = A[p][q];
  if (!(apq < 0.0 || apq > 0.0)) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double root = __builtin_sqrt(theta * theta + 1.0);
  const double t = theta < 0.0 ? -1.0 / (root - theta) : 1.0 / (root + theta);   // the smaller root of t^2 + 2 theta t - 1 = 0
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
  const double s = t * c;
  A[p][p] = A[p][p] - t * apq;
  A[q][q] = A[q][q] + t * apq;
  A[p][q] = 0.0;
  A[q][p] = 0.0;
  const double arp = A[r][p], arq = A[r][q];
  A[r][p] = c * arp - s * arq;
  A[p][r] = A[r][p];
  A[r][q] = s * arp + c * arq;
  A[q][r] = A[r][q];
#pragma GCC unroll 3
  for (int k = 0; k < 3; ++k) {
    const double vkp = V[k][p], vkq = V[k][q];
    V[k][p] = c * vkp - s * vkq;
    V[k][q] = s * vkp + c * vkq;
  }
}

// The part both fits share, up to the diagonalised matrix: mean = S1 / m, the covariance A, the fixed sweeps; A's diagonal then holds the
// eigenvalues and V's columns the eigenvectors.  false when m < 3 or the covariance is not finite.
// md = the divisor of the moments: (double)m for the unweighted fits, the sum of the weights for smooth_fit below (the one text for both).
EF_PF_HD bool plane_fit_eigen_w(const double S[9], unsigned m, double md, double A[3][3], double V[3][3], double mean[3]) {
  if (m < 3u) return false;
  const double mx = S[0] / md, my = S[1] / md, mz = S[2] / md;
  A[0][0] = S[3] / md - mx * mx;
  A[0][1] = S[4] / md - mx * my;
  A[0][2] = S[5] / md - mx * mz;
  A[1][1] = S[6] / md - my * my;
  A[1][2] = S[7] / md - my * mz;
  A[2][2] = S[8] / md - mz * mz;
  A[1][0] = A[0][1];
  A[2][0] = A[0][2];
  A[2][1] = A[1][2];
  if (!plane_fit_finite(A[0][0]) || !plane_fit_finite(A[0][1]) || !plane_fit_finite(A[0][2]) || !plane_fit_finite(A[1][1]) ||
      !plane_fit_finite(A[1][2]) || !plane_fit_finite(A[2][2]))
    return false;
  V[0][0] = V[1][1] = V[2][2] = 1.0;
  V[0][1] = V[0][2] = V[1][0] = V[1][2] = V[2][0] = V[2][1] = 0.0;
  for (int sweep = 0; sweep < EF_PLANE_FIT_SWEEPS; ++sweep) {
    plane_fit_rotate(A, V, 0, 1, 2);
    plane_fit_rotate(A, V, 0, 2, 1);
    plane_fit_rotate(A, V, 1, 2, 0);
  }
  mean[0] = mx;
  mean[1] = my;
  mean[2] = mz;
  return true;
}
EF_PF_HD bool plane_fit_eigen(const double S[9], unsigned m, double A[3][3], double V[3][3], double mean[3]) {
  return plane_fit_eigen_w(S, m, (double)m, A, V, mean);
}

// The eigenvector of the smallest eigenvalue (ties: the lowest index), normalised and flipped to hn's side (a zero or NaN hn flips nothing).
// n = the normal, l = the three diagonal entries, lambda = the chosen one, flipped = whether the sign was turned.  false, and nothing written,
// when the choice or the normalisation is not finite.
EF_PF_HD bool plane_fit_normal(const double A[3][3], const double V[3][3], const float hn[3], double n[3], double l[3], double* lambda_out,
                               bool* flipped) {
  // (every entry is read unconditionally and chosen by value: a choice between two ADDRESSES of V would put the matrix into the device's scratch)
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  const double v00 = V[0][0], v10 = V[1][0], v20 = V[2][0], v01 = V[0][1], v11 = V[1][1], v21 = V[2][1], v02 = V[0][2], v12 = V[1][2], v22 = V[2][2];
  double lambda = l0, nx = v00, ny = v10, nz = v20;
  if (l1 < lambda) { lambda = l1; nx = v01; ny = v11; nz = v21; }
  if (l2 < lambda) { lambda = l2; nx = v02; ny = v12; nz = v22; }
  if (!plane_fit_finite(lambda)) return false;
  const double len = __builtin_sqrt((nx * nx + ny * ny) + nz * nz);
  if (!(len > 0.0) || !plane_fit_finite(len)) return false;
  nx = nx / len;
  ny = ny / len;
  nz = nz / len;
  const bool flip = (nx * (double)hn[0] + ny * (double)hn[1]) + nz * (double)hn[2] < 0.0;
  if (flip) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
  n[0] = nx;
  n[1] = ny;
  n[2] = nz;
  l[0] = l0;
  l[1] = l1;
  l[2] = l2;
  *lambda_out = lambda;
  *flipped = flip;
  return true;
}

EF_PF_HD bool plane_fit(const double S[9], unsigned m, const float a[3], const float hn[3], float n_out[3], float* d_out, float* thickness_out) {
  double A[3][3], V[3][3], mean[3], n[3], l[3], lambda;
  bool flipped;
  if (!plane_fit_eigen(S, m, A, V, mean)) return false;
  if (!plane_fit_normal(A, V, hn, n, l, &lambda, &flipped)) return false;
  const double nx = n[0], ny = n[1], nz = n[2], mx = mean[0], my = mean[1], mz = mean[2];
  const double d = -((nx * ((double)a[0] + mx) + ny * ((double)a[1] + my)) + nz * ((double)a[2] + mz));
  const double th = __builtin_sqrt(lambda > 0.0 ? lambda : 0.0);
  if (!plane_fit_finite(nx) || !plane_fit_finite(ny) || !plane_fit_finite(nz) || !plane_fit_finite(d) || !plane_fit_finite(th)) return false;
  const float fx = (float)nx, fy = (float)ny, fz = (float)nz, fd = (float)d, ft = (float)th;
  if (!plane_fit_finite((double)fd) || !plane_fit_finite((double)ft)) return false;   // (|n| <= 1: only d and the thickness can leave f32's range)
  n_out[0] = fx;
  n_out[1] = fy;
  n_out[2] = fz;
  *d_out = fd;
  *thickness_out = ft;
  return true;
}

// ---- the normals' entry point (ef_normals.inc: k_normal_join; "Estimate normals, curvature and spacing" of include/ef_hip.h) ----
constexpr int NORMAL_FIT_GAVE_UP = 0, NORMAL_FIT_ESTIMATED = 1, NORMAL_FIT_DEGENERATE = 2;

// From the nine sums over the m members of a neighbourhood (the anchor is the row's own position, so no plane offset is formed) to the
// oriented normal, the surface variation and the verdict.  With e_i = max(l_i, 0) by comparison: curvature = emin / ((e_0 + e_1) + e_2),
// 0 when the sum is not > 0; DEGENERATE iff !(emid > (double)line_ratio * emax), emax and emid chosen by comparisons.  Every output is
// written in every case: n_out, curvature_out and flipped_out are zeros and false unless the return value is NORMAL_FIT_ESTIMATED; l_out = the
// three diagonal entries of the diagonalised covariance as computed (not clamped), zeros when the fit gave up.
EF_PF_HD int normal_fit(const double S[9], unsigned m, const float hn[3], float line_ratio, float n_out[3], float* curvature_out, bool* flipped_out,
                        double l_out[3]) {
  n_out[0] = n_out[1] = n_out[2] = 0.0f;
  *curvature_out = 0.0f;
  *flipped_out = false;
  l_out[0] = l_out[1] = l_out[2] = 0.0;
  double A[3][3], V[3][3], mean[3], n[3], l[3], lambda;
  bool flipped;
  if (!plane_fit_eigen(S, m, A, V, mean)) return NORMAL_FIT_GAVE_UP;
  if (!plane_fit_normal(A, V, hn, n, l, &lambda, &flipped)) return NORMAL_FIT_GAVE_UP;
  if (!plane_fit_finite(l[0]) || !plane_fit_finite(l[1]) || !plane_fit_finite(l[2]) || !plane_fit_finite(n[0]) || !plane_fit_finite(n[1]) ||
      !plane_fit_finite(n[2]))
    return NORMAL_FIT_GAVE_UP;
  l_out[0] = l[0];
  l_out[1] = l[1];
  l_out[2] = l[2];
  const double e0 = l[0] > 0.0 ? l[0] : 0.0, e1 = l[1] > 0.0 ? l[1] : 0.0, e2 = l[2] > 0.0 ? l[2] : 0.0;
  const double emin = lambda > 0.0 ? lambda : 0.0;
  // the greatest and the median of three by comparisons: lo / hi of the first two, then the third against both
  const double lo = e1 < e0 ? e1 : e0, hi = e1 < e0 ? e0 : e1;
  const double emax = e2 > hi ? e2 : hi;
  const double emid = e2 > hi ? hi : (e2 < lo ? lo : e2);
  if (!(emid > (double)line_ratio * emax)) return NORMAL_FIT_DEGENERATE;
  const double sum = (e0 + e1) + e2;
  n_out[0] = (float)n[0];
  n_out[1] = (float)n[1];
  n_out[2] = (float)n[2];
  *curvature_out = sum > 0.0 ? (float)(emin / sum) : 0.0f;
  *flipped_out = flipped;
  return NORMAL_FIT_ESTIMATED;
}

// ---- the smoothing's entry point (ef_smooth.inc: k_smooth_step; "Smooth the map's positions" of include/ef_hip.h) ----
// normal_fit for WEIGHTED moments: S = the nine weighted sums about the row's own position, W = 1 + the sum of the weights (the divisor of the
// moments), m = c + 1 = the members of the neighbourhood (the "fewer than three" test only).  From plane_fit_eigen_w on it is normal_fit's
// text: the same choice, normalisation and flip to hn's side, the same finiteness checks, DEGENERATE test and curvature.  What the projection
// needs comes back in double: n_out = the unit normal, mean_out = the weighted mean of the differences.  Every output is written in every
// case: zeros unless the return value is NORMAL_FIT_ESTIMATED.  With unit weights (W == (double)m) normal, curvature and verdict are
// normal_fit's bit for bit.
EF_PF_HD int smooth_fit(const double S[9], double W, unsigned m, const float hn[3], float line_ratio, double n_out[3], double mean_out[3],
                        float* curvature_out) {
  n_out[0] = n_out[1] = n_out[2] = 0.0;
  mean_out[0] = mean_out[1] = mean_out[2] = 0.0;
  *curvature_out = 0.0f;
  double A[3][3], V[3][3], mean[3], n[3], l[3], lambda;
  bool flipped;
  if (!plane_fit_eigen_w(S, m, W, A, V, mean)) return NORMAL_FIT_GAVE_UP;
  if (!plane_fit_normal(A, V, hn, n, l, &lambda, &flipped)) return NORMAL_FIT_GAVE_UP;
  if (!plane_fit_finite(l[0]) || !plane_fit_finite(l[1]) || !plane_fit_finite(l[2]) || !plane_fit_finite(n[0]) || !plane_fit_finite(n[1]) ||
      !plane_fit_finite(n[2]))
    return NORMAL_FIT_GAVE_UP;
  const double e0 = l[0] > 0.0 ? l[0] : 0.0, e1 = l[1] > 0.0 ? l[1] : 0.0, e2 = l[2] > 0.0 ? l[2] : 0.0;
  const double emin = lambda > 0.0 ? lambda : 0.0;
  const double lo = e1 < e0 ? e1 : e0, hi = e1 < e0 ? e0 : e1;
  const double emax = e2 > hi ? e2 : hi;
  const double emid = e2 > hi ? hi : (e2 < lo ? lo : e2);
  if (!(emid > (double)line_ratio * emax)) return NORMAL_FIT_DEGENERATE;
  const double sum = (e0 + e1) + e2;
  n_out[0] = n[0];
  n_out[1] = n[1];
  n_out[2] = n[2];
  mean_out[0] = mean[0];
  mean_out[1] = mean[1];
  mean_out[2] = mean[2];
  *curvature_out = sum > 0.0 ? (float)(emin / sum) : 0.0f;
  return NORMAL_FIT_ESTIMATED;
}

}  // namespace efm
