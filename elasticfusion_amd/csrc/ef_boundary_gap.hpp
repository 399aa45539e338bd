// The angular gap of a surfel's neighbourhood seen along its normal (ef_map_boundaries, include/ef_hip.h "Find the map's boundaries": FRAME,
// PROJECTION, TURN and GAP; ef_boundary.inc: k_boundary_join).  This text IS the definition.  It compiles for the host and the
// device (as ef_plane_fit.hpp does): tests/boundary_gap_main.cpp runs the same text under g++ -ffp-contract=off, and tests/boundaryref.py
// restates it line by line in Python floats (IEEE doubles).
//   ARITHMETIC  only +, -, *, / and sqrt in double, each correctly rounded on every target and never contracted, in the written order, and
//               the absolute value, which is exact: the result is the same bits wherever it runs.  Every test is written so that a NaN takes
//               the "no direction" / "t = 0" side.
//   INPUT       m = the row's normal (f32, any length); p = the row's position and px / py / pz = the positions of its neighbours in
//               neighbour order (f32), of which the first c are used (c <= K).
//   OUTPUT      BOUNDARY_GAP_DEGENERATE when the normal has no direction or no used neighbour has one in the tangent plane; otherwise
//               BOUNDARY_GAP_OK and *G = the widest turn, in [0, 4], that no direction interrupts.
//   TURN        divisions only, no inverse trigonometry: t = quadrant + sin / (|sin| + |cos|) of the counter-clockwise angle, which is
//               monotone in the angle (1 = 90 degrees, 2 = 180, 3 = 270).  c = x_j * y_i - y_j * x_i is EXACTLY antisymmetric in IEEE
//               arithmetic (the two products commute and a - b = -(b - a)), and d is symmetric, so TURN(j, i) and TURN(i, j) always see the
//               same |c| and the same d: two directions agree on whether they coincide (t = 0), and of a group of coincident directions
//               exactly one (the highest slot) looks past the group.
//   SHAPE       the outer loop over the slots is rolled and reads slot j through a chain of selects, the inner one is unrolled: every index
//               of x[] and y[] is a compile-time constant, so on the device the arrays stay in registers, and the 16 x 16 pair loop is 16
//               turns of code, not 240.
#pragma once

#if defined(__HIPCC__)
#define EF_BG_HD __host__ __device__ __forceinline__
#else
#define EF_BG_HD inline
#endif

namespace efm {

constexpr int BOUNDARY_GAP_OK = 0, BOUNDARY_GAP_DEGENERATE = 1;

EF_BG_HD bool boundary_finite(double x) { return x - x == 0.0; }   // false for an infinity and for a NaN

// FRAME: e1 = e x h and e2 = h x e1 for h = m / |m| and e = the axis of the smallest |h_i|; false when (m . m) is not finite and positive
EF_BG_HD bool boundary_frame(const float m[3], double e1[3], double e2[3]) {
  const double ax = (double)m[0], ay = (double)m[1], az = (double)m[2];
  const double nn = (ax * ax + ay * ay) + az * az;
  if (!(boundary_finite(nn) && nn > 0.0)) return false;
  const double len = __builtin_sqrt(nn);
  const double hx = ax / len, hy = ay / len, hz = az / len;
  int i0 = 0;
  double low = __builtin_fabs(hx);
  if (__builtin_fabs(hy) < low) { i0 = 1; low = __builtin_fabs(hy); }
  if (__builtin_fabs(hz) < low) i0 = 2;
  const double ex = i0 == 0 ? 1.0 : 0.0, ey = i0 == 1 ? 1.0 : 0.0, ez = i0 == 2 ? 1.0 : 0.0;
  e1[0] = ey * hz - ez * hy;
  e1[1] = ez * hx - ex * hz;
  e1[2] = ex * hy - ey * hx;
  e2[0] = hy * e1[2] - hz * e1[1];
  e2[1] = hz * e1[0] - hx * e1[2];
  e2[2] = hx * e1[1] - hy * e1[0];
  return true;
}

// PROJECTION of one neighbour: q = (double)p_j - (double)p_s; true iff (x, y) is a DIRECTION
EF_BG_HD bool boundary_project(const double e1[3], const double e2[3], const float p[3], float tx, float ty, float tz, double* x, double* y) {
  const double qx = (double)tx - (double)p[0], qy = (double)ty - (double)p[1], qz = (double)tz - (double)p[2];
  *x = (qx * e1[0] + qy * e1[1]) + qz * e1[2];
  *y = (qx * e2[0] + qy * e2[1]) + qz * e2[2];
  return boundary_finite(*x) && boundary_finite(*y) && __builtin_fabs(*x) + __builtin_fabs(*y) > 0.0;
}

// TURN(j, i) for two directions; i_below_j: slot i < slot j
EF_BG_HD double boundary_turn(double xj, double yj, double xi, double yi, bool i_below_j) {
  const double d = xj * xi + yj * yi;
  const double c = xj * yi - yj * xi;
  const double s = __builtin_fabs(d) + __builtin_fabs(c);
  double t;
  if (s == 0.0 || !boundary_finite(s)) t = 0.0;
  else if (d >= 0.0 && c >= 0.0) t = c / s;
  else if (d < 0.0) t = 2.0 - c / s;
  else t = 4.0 + c / s;
  if (t == 0.0 && i_below_j) t = 4.0;
  return t;
}

// GAP over the slots whose bit is set in dirs (all below c): g_j starts at 4 and is replaced by every smaller TURN(j, i), i ascending; G starts
// at +0.0 and is replaced by every greater g_j, j ascending
template <int K>
EF_BG_HD double boundary_widest(const double (&x)[K], const double (&y)[K], unsigned dirs, int c) {
  double G = 0.0;
#pragma GCC unroll 1
  for (int j = 0; j < c; ++j) {
    if (!((dirs >> j) & 1u)) continue;
    double xj = x[0], yj = y[0];
#pragma GCC unroll 16
    for (int s = 1; s < K; ++s)
      if (s == j) { xj = x[s]; yj = y[s]; }
    double g = 4.0;
#pragma GCC unroll 16
    for (int i = 0; i < K; ++i) {
      if (i == j || !((dirs >> i) & 1u)) continue;
      const double t = boundary_turn(xj, yj, x[i], y[i], i < j);
      if (t < g) g = t;
    }
    if (g > G) G = g;
  }
  return G;
}

// the whole definition for one row: frame, projections of the first c neighbours, the widest gap
template <int K>
EF_BG_HD int boundary_gap(const float m[3], const float p[3], const float (&px)[K], const float (&py)[K], const float (&pz)[K], int c, double* G) {
  double e1[3], e2[3];
  if (!boundary_frame(m, e1, e2)) return BOUNDARY_GAP_DEGENERATE;
  double x[K], y[K];
  unsigned dirs = 0u;
#pragma GCC unroll 16
  for (int j = 0; j < K; ++j) {
    x[j] = 0.0;
    y[j] = 0.0;
    if (j < c && boundary_project(e1, e2, p, px[j], py[j], pz[j], &x[j], &y[j])) dirs |= 1u << j;
  }
  if (!dirs) return BOUNDARY_GAP_DEGENERATE;
  *G = boundary_widest<K>(x, y, dirs, c);
  return BOUNDARY_GAP_OK;
}

}  // namespace efm
