// wg_footcons_geom.hpp -- the geometry of the ZMP polytopes, once, for the host call (wg_footcons.cpp) and the kernel
// (wg_footcons_device.hpp): support classification, sole corners, the 8-point hull, half-plane forms, the polytope fill.
//
//   FootConstraintsAsLinearSystem::BuildLinearConstraintInequalities  src/Mathematics/FootConstraintsAsLinearSystem.cpp:258-539
//   FootConstraintsAsLinearSystem::ComputeLinearSystem                :97-256
//   FootConstraintsAsLinearSystem::FindSimilarConstraints             :55-92
//   ComputeConvexHull::DoComputeConvexHull                            src/Mathematics/ConvexHull.cpp:88-203
//
// Plain C++ that a HIP translation unit compiles for both sides: WG_FC_HD is `__host__ __device__` there and nothing elsewhere,
// and nothing here names a kernel, LDS or a block index.  The functions work on one lane's point scratch, kFcSlots points
// addressed through FcPts<kStride>: [slot][64 lanes] in LDS in the kernel (kStride = 64), a local array on the host (kStride = 1).
// The library is built with -ffp-contract=off, / and sqrt are IEEE on both sides and sin / cos are include/wg_trig.h: the
// same bytes from both.
#pragma once
#include <cmath>

#include "../../include/wg_mpc.h"
#ifdef __HIP__
#define WG_FC_HD __host__ __device__
#else
#define WG_FC_HD
#endif
#define WG_FC_INLINE WG_FC_HD inline __attribute__((always_inline))
#ifndef WG_TRIG_FN
#define WG_TRIG_FN WG_FC_HD static inline
#endif
#include "../../include/wg_trig.h"

namespace wg {

constexpr int kFcSlots = 17;             // hull scratch per lane: 9 points (corners, then the hull) + 8 (the ordered candidates)
constexpr double kFcPi = 3.14159265358979323846;
enum { kFcInherit = 0, kFcRight = 1, kFcLeft = 2, kFcDouble = 3 };   // 1..3: the reference's states

// the state the reference's three tests give sample (stepType, left z, right z), or kFcInherit when none of them holds
WG_FC_INLINE int fc_classify(int ltype, double lz, double rz) {
  const double lifting = 0.00001;
  if (ltype >= 10) return kFcDouble;
  if (lz > lifting) return kFcLeft;      // the reference's state 2: the LEFT foot is in the air
  if (rz > lifting) return kFcRight;
  if (rz < lifting && lz < lifting) return kFcDouble;
  return kFcInherit;
}

// one lane's hull scratch: point s at [2 s + {0, 1}][lane of kStride]
template <int kStride>
struct FcPts {
  double *base;
  WG_FC_INLINE double &x(int s) const { return base[(2 * s) * kStride]; }
  WG_FC_INLINE double &y(int s) const { return base[(2 * s + 1) * kStride]; }
};

WG_FC_INLINE double fc_cross(double ox, double oy, double ax, double ay, double bx, double by) {
  const double x1 = ax - ox, x2 = bx - ox, y1 = ay - oy, y2 = by - oy;
  return x1 * y2 - x2 * y1;
}

// the four corners of the sole at (fx, fy), heading theta (degrees), into slots s0 .. s0 + 3 (counter-clockwise)
template <int kStride>
WG_FC_HD inline void fc_corners(const FcPts<kStride> &P, int s0, double fx, double fy, double theta, double hw, double hh) {
  const double s = wg_sin(theta * kFcPi / 180.0), c = wg_cos(theta * kFcPi / 180.0);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const double sx = j < 2 ? 1.0 : -1.0, sy = (j == 1 || j == 2) ? 1.0 : -1.0;
    P.x(s0 + j) = fx + (sx * hw * c - sy * hh * s);
    P.y(s0 + j) = fy + (sx * hw * s + sy * hh * c);
  }
}

// Graham scan about the lowest point: the 8 points in slots 0..7 -> the hull in slots 0.. (returned size; 0: fewer than two
// directions).  The reference keeps the candidates in a std::set ordered by the sign of the cross product about p0; two
// candidates in the same direction are reduced to the farther one before the insertion.  Slots 9..16 hold them, in ascending
// polar angle.
template <int kStride>
WG_FC_HD inline int fc_hull8(const FcPts<kStride> &P) {
  const int O = 9;
  double p0x = P.x(0), p0y = P.y(0);
  for (int i = 0; i < 8; i++)
    if (P.y(i) < p0y) { p0x = P.x(i); p0y = P.y(i); }
  int no = 0;
  for (int i = 0; i < 8; i++) {
    const double px = P.x(i), py = P.y(i);
    bool insert = true;
    for (int k = 0; k < no;) {
      const double kx = P.x(O + k), ky = P.y(O + k);
      if (fc_cross(p0x, p0y, kx, ky, px, py) == 0.0) {
        const double dk = sqrt((kx - p0x) * (kx - p0x) + (ky - p0y) * (ky - p0y));
        const double dp = sqrt((px - p0x) * (px - p0x) + (py - p0y) * (py - p0y));
        if (dk <= dp) {
          for (int q = k; q < no - 1; q++) { P.x(O + q) = P.x(O + q + 1); P.y(O + q) = P.y(O + q + 1); }
          no--;
          continue;
        }
        insert = false;
      }
      k++;
    }
    if (!insert) continue;
    int pos = 0;
    bool equivalent = false;
    for (; pos < no; pos++) {
      const double kx = P.x(O + pos), ky = P.y(O + pos);
      if (fc_cross(p0x, p0y, px, py, kx, ky) > 0.0) break;            // p orders before the candidate
      if (!(fc_cross(p0x, p0y, kx, ky, px, py) > 0.0)) equivalent = true;
    }
    if (!equivalent) {
      for (int q = no; q > pos; q--) { P.x(O + q) = P.x(O + q - 1); P.y(O + q) = P.y(O + q - 1); }
      P.x(O + pos) = px; P.y(O + pos) = py;
      no++;
    }
  }
  if (no < 2) return 0;
  int nh = 0;
  P.x(nh) = p0x; P.y(nh) = p0y; nh++;
  P.x(nh) = P.x(O); P.y(nh) = P.y(O); nh++;
  P.x(nh) = P.x(O + 1); P.y(nh) = P.y(O + 1); nh++;
  for (int it = 2; it < no; it++) {
    const double ix = P.x(O + it), iy = P.y(O + it);
    while (nh >= 2 && !(fc_cross(P.x(nh - 2), P.y(nh - 2), P.x(nh - 1), P.y(nh - 1), ix, iy) > 0.0)) nh--;
    P.x(nh) = ix; P.y(nh) = iy; nh++;
  }
  return nh;
}

// the half plane left of the edge p -> q as a x + c y + b >= 0; (ax_, ay_) is the point the reference takes the offset at
WG_FC_INLINE void fc_half_plane(double px, double py, double qx, double qy, double ax_, double ay_, double &a, double &c, double &b) {
  if (fabs(qx - px) > 1e-7) {
    double x1, y1, x2, y2, lmul = -1.0;
    if (qx < px) {
      lmul = 1.0;
      x1 = qx; y1 = qy; x2 = px; y2 = py;
    } else {
      x1 = px; y1 = py; x2 = qx; y2 = qy;
    }
    a = (y2 - y1) / (x2 - x1);
    b = (ay_ - a * ax_);
    a = lmul * a;
    b = lmul * b;
    c = -lmul;
  } else {
    c = 0.0;
    a = -1.0;
    b = qx;
    if (qy < py) {
      a = -a;
      b = -b;
    }
  }
}

// the polytope of the hull in slots 0..n-1, written straight to *out, every byte of it (rows >= n and pad_ zero); the rows'
// (a, c) go through slots 9.. for FindSimilarConstraints.  false: the reference's "not a polytope" (n < 2 or n > 8), *out untouched
template <int kStride>
WG_FC_HD inline bool fc_polytope(const FcPts<kStride> &P, int n, wg_zmp_polytope_t *out) {
  if (n < 2 || n > WG_POLY_MAX_ROWS) return false;
  const int O = 9;
  double cx = 0.0, cy = 0.0;
  for (int i = 0; i < WG_POLY_MAX_ROWS; i++) {
    double a = 0.0, c = 0.0, b = 0.0;
    if (i < n) {
      cx += P.x(i);
      cy += P.y(i);
      if (i < n - 1)
        fc_half_plane(P.x(i), P.y(i), P.x(i + 1), P.y(i + 1), P.x(i), P.y(i), a, c, b);     // offset at the edge's first point
      else
        fc_half_plane(P.x(n - 1), P.y(n - 1), P.x(0), P.y(0), P.x(0), P.y(0), a, c, b);    // closing edge: at its last point
      P.x(O + i) = a; P.y(O + i) = c;
    }
    out->A[i][0] = a; out->A[i][1] = c; out->B[i] = b;
  }
  out->nrows = n;
  out->pad_ = 0;
  out->centre[0] = cx / (double)n;
  out->centre[1] = cy / (double)n;
  const int half = n == 4 ? 2 : (n == 6 ? 3 : 0);         // FindSimilarConstraints knows rectangles and hexagons
  for (int k = 0; k < WG_POLY_MAX_ROWS; k++) {
    int sim = 0;
    if (k >= half && k < 2 * half && P.x(O + k - half) == -P.x(O + k) && P.y(O + k - half) == -P.y(O + k)) sim = -half;
    out->similar[k] = sim;
  }
  return true;
}

}  // namespace wg
