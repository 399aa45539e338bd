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

EF_PF_HD bool plane_fit(const double S[9], unsigned m, const float a[3], const float hn[3], float n_out[3], float* d_out, float* thickness_out) {
  if (m < 3u) return false;
  const double md = (double)m;
  const double mx = S[0] / md, my = S[1] / md, mz = S[2] / md;
  double A[3][3], V[3][3];
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
  if ((nx * (double)hn[0] + ny * (double)hn[1]) + nz * (double)hn[2] < 0.0) {
    nx = -nx;
    ny = -ny;
    nz = -nz;
  }
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

}  // namespace efm
