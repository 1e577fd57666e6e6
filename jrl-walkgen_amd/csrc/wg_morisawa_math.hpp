// wg_morisawa_math.hpp -- the arithmetic of the Morisawa-2007 analytic walk (AnalyticalMorisawaCompact), once, for the host calls
// (wg_morisawa_solve / _sample / _length: wg_morisawa.cpp) and the kernels (wg_morisawa_kernels.hpp).
//
//   InitializeBasicVariables                       src/ZMPRefTrajectoryGeneration/AnalyticalMorisawaCompact.cpp:170-224
//   BuildAndSolveCOMZMPForASetOfSteps              :360-512   (IgnoreFirstRelativeFoot = true, DoNotPrepareLastFoot = false)
//   GetZMPDiscretization / FillQueues / OnLine     :514-579, 2230-2290, 648-723 (analytic branch)
//   ComputeW                                       :831-942
//   ComputeZ1 / ComputeZj / ComputeZm / BuildingTheZMatrix   :944-1164
//   TransfertTheCoefficientsToTrajectories         :1166-1233
//   AnalyticalZMPCOGTrajectory                     src/Mathematics/AnalyticalZMPCOGTrajectory.cpp:175-196, 276-282, 386-410,
//                                                  425-456, 472-507
//   LeftAndRightFootTrajectoryGenerationMultiple   src/FootTrajectoryGeneration/LeftAndRightFootTrajectoryGenerationMultiple.cpp
//                                                  :107-166, 168-572 (Continuity = false)
//   FootTrajectoryGenerationMultiple::Compute      FootTrajectoryGenerationMultiple.cpp:128-135
//   FootTrajectoryGenerationStandard               FootTrajectoryGenerationStandard.cpp:188-227, 307-333
//   Polynome3/4/5, Polynome::Compute               src/Mathematics/PolynomeFoot.cpp:59-79, 122-146, 226-240, Polynome.cpp:44-64
//
// Plain C++ that a HIP translation unit compiles for both sides: WG_MO_HD is `__host__ __device__` there and nothing elsewhere,
// and nothing here names a kernel or a block index.  mo_solve is a list of phases; a phase is a loop over independent outputs,
// `for (e = x.lane(); e < count; e += x.lanes())`, and x.sync() stands between a phase and the next one that reads what it
// wrote.  The host runs it with one lane and no fence (MoHostExec), the kernel with the 64 lanes of a wavefront and WG_WSYNC.
// Every output element keeps one order of operations whichever lane computes it -- the reference's where it has one (ComputeW's
// r1 / r2, Polynome::Compute, the running sums of the interval times), the stated one in the elimination -- and the library is
// built with -ffp-contract=off, / and sqrt are IEEE on both sides, sin / cos are include/wg_trig.h, cosh / sinh are mo_coshsinh
// below: host and kernel give the same bytes.
//
// The reference solves Z y = w with LAPACK (dgetrf_ once, dgesvx_ with its refinement per axis, :263-357).  LAPACK is not part
// of this project: mo_lu is a right-looking LU with partial pivoting and no refinement; parity with the reference is by
// tolerance (tests/test_morisawa_golden.py, tests/test_morisawa_host.py).
//
// Two forms of the solve: mo_solve / mo_lu, dense, a row of Z per lane, up to WG_MORISAWA_MAX_STEPS steps (n <= 64), and
// mo_solve_long / mo_band_lu, Z as a row band of 16 words, a lane per element of the elimination's live window, up to
// WG_MORISAWA_LONG_MAX_STEPS steps (n <= 264).  The band takes the dense form's pivots and gives its values; mo_sample reads the
// blocks of both through their layouts.  mo_resolve / mo_resolve_long (at the end of the file) re-plan a walk from a solved block's
// kept factor: the solves' bytes without building or eliminating Z.
//
// Quirks of the reference kept on purpose, each marked where it is reproduced: g is 9.86 (:1106), the ZMP twin's
// sTc = fabs(9.86 / (z_com - z_zmp)) (AnalyticalZMPCOGTrajectory.cpp:401), and the right-support branch clears the LEFT foot's
// dz (LeftAndRightFootTrajectoryGenerationMultiple.cpp:419).
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/wg_mpc.h"
#ifdef __HIP__
#define WG_MO_HD __host__ __device__
#else
#define WG_MO_HD
#endif
#define WG_MO_INLINE WG_MO_HD inline __attribute__((always_inline))
#ifndef WG_TRIG_FN
#define WG_TRIG_FN WG_MO_HD static inline
#endif
#include "../../include/wg_trig.h"

namespace wg {

constexpr double kMoPi = 3.14159265358979323846;   // M_PI
constexpr double kMoG = 9.86;                      // the reference's g on this path (:1106), not 9.81
constexpr double kMoArgMax = 40.0;                 // cosh / sinh are made for [0, 40]
constexpr double kMoWalkArgMax = WG_MORISAWA_WALK_ARG_MAX;   // a walk is accurate up to here: the method in float64, see the header

// a double is finite iff x - x == 0 (inf - inf and nan - nan are nan)
WG_MO_INLINE bool mo_finite(double x) { return x - x == 0.0; }
// the admission of a gait's timing, for every solve and re-plan: no omega_j dT_j beyond the bound of accuracy (a NaN is beyond it)
WG_MO_INLINE bool mo_args_ok(const wg_morisawa_model_t &m, double omega) {
  return omega * (m.t_single * 3.0) <= kMoWalkArgMax && omega * m.t_double <= kMoWalkArgMax;
}
WG_MO_INLINE double mo_abs(double x) { return x < 0.0 ? -x : (x == 0.0 ? 0.0 : x); }

// ---- cosh and sinh of x in [0, 40] as a fixed sequence of IEEE +, -, *, / (no libm, no ocml) ----------------------------------
// exp: k = nearest integer of x / ln 2, r = x - k ln 2 in two words (the high word has 32 significant bits, k < 64: k * hi is
// exact), e^r = 1 + 2 r / (2 - c) with c = r - r^2 P(r^2) (the well-known fdlibm scheme and coefficients), times 2^k made of
// exact products.  cosh = e/2 + 1/(2e); sinh = e/2 - 1/(2e) from 1 up, and the odd series x + x^3/3! + .. + x^21/21! below 1,
// where the difference would cancel.  Measured against 50-digit values: see tests/test_morisawa_host.py.
WG_MO_INLINE double mo_exp(double x) {
  const double ln2hi = 6.93147180369123816490e-01, ln2lo = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00;
  const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
               P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
  const int k = (int)(invln2 * x + 0.5);
  const double hi = x - k * ln2hi, lo = k * ln2lo;
  const double r = hi - lo;
  const double t = r * r;
  const double c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
  double s = 1.0;
  if (k & 1) s *= 2.0;
  if (k & 2) s *= 4.0;
  if (k & 4) s *= 16.0;
  if (k & 8) s *= 256.0;
  if (k & 16) s *= 65536.0;
  if (k & 32) s *= 4294967296.0;
  return y * s;
}
WG_MO_INLINE void mo_coshsinh(double x, double &ch, double &sh) {
  const double e = mo_exp(x);
  const double h = 0.5 * e, g = 0.5 / e;
  ch = h + g;
  if (x >= 1.0) {
    sh = h - g;
  } else {
    const double z = x * x;
    double p = 1.0 / 51090942171709440000.0;                  // 1 / 21!
    p = 1.0 / 121645100408832000.0 + z * p;                    // 1 / 19!
    p = 1.0 / 355687428096000.0 + z * p;                       // 1 / 17!
    p = 1.0 / 1307674368000.0 + z * p;                         // 1 / 15!
    p = 1.0 / 6227020800.0 + z * p;                            // 1 / 13!
    p = 1.0 / 39916800.0 + z * p;                              // 1 / 11!
    p = 1.0 / 362880.0 + z * p;                                // 1 / 9!
    p = 1.0 / 5040.0 + z * p;                                  // 1 / 7!
    p = 1.0 / 120.0 + z * p;                                   // 1 / 5!
    p = 1.0 / 6.0 + z * p;                                     // 1 / 3!
    sh = x + x * (z * p);
  }
}

// ---- the trajectory block of one gait -------------------------------------------------------------------------------------------
// Offsets in doubles.  imax = 2 smax + 1 intervals, nmax = 4 smax + 8 unknowns.  What a gait does not use stays zero, so blocks
// compare as bytes.  The LU factor is last; in the work area (LDS in the kernel) its rows are nmax + 1 apart (lane i owns row i:
// an odd pitch keeps the 64 lanes of a column access on different banks), in the block they are nmax apart.
struct MoLayout {
  int smax, imax, nmax;
  int o_dT, o_om, o_tref;                  // [imax] each
  int o_zx, o_cx, o_zy, o_cy;              // [imax][5]: ZMP and CoG polynomials of x, of y
  int o_vx, o_wx, o_vy, o_wy;              // [imax]: the hyperbolic weights
  int o_left, o_right;                     // [imax][6][6]: x y z theta omega omega2, coefficients 0 .. 5
  int o_nat;                               // ints: left_type[imax], right_type[imax]
  int o_zpx, o_zpy;                        // [imax]: the ZMP profile (ZMPProfil)
  int o_sup;                               // [smax][3]: the absolute support feet
  int o_rhs;                               // [4][nmax]: w of x, w of y, y of x, y of y
  int o_piv;                               // ints [nmax]
  int o_lu;                                // [nmax][nmax]
  int words;                               // block size in doubles, a multiple of 16
  // work area only, behind the image with the padded LU
  int o_seg;                               // [imax][2][12]: per interval and foot, start (6) and target (6) of the six axes
  int work_words;                          // 65 280 B at smax = 14: within the 64 KiB a kernel has without asking
};
constexpr int kMoHdr = 16;                 // header: ints n_steps, n_int, n, smax; doubles com height [2], sum of dT [3]
WG_MO_INLINE MoLayout mo_layout(int smax) {
  MoLayout L;
  L.smax = smax; L.imax = 2 * smax + 1; L.nmax = 4 * smax + 8;
  int o = kMoHdr;
  const int I = L.imax;
  L.o_dT = o; o += I; L.o_om = o; o += I; L.o_tref = o; o += I;
  L.o_zx = o; o += 5 * I; L.o_cx = o; o += 5 * I; L.o_zy = o; o += 5 * I; L.o_cy = o; o += 5 * I;
  L.o_vx = o; o += I; L.o_wx = o; o += I; L.o_vy = o; o += I; L.o_wy = o; o += I;
  L.o_left = o; o += 36 * I; L.o_right = o; o += 36 * I;
  L.o_nat = o; o += I;
  L.o_zpx = o; o += I; L.o_zpy = o; o += I;
  L.o_sup = o; o += 3 * smax;
  L.o_rhs = o; o += 4 * L.nmax;
  L.o_piv = o; o += L.nmax / 2;
  L.o_lu = o;
  L.words = (o + L.nmax * L.nmax + 15) & ~15;
  int w = o + L.nmax * (L.nmax + 1);
  L.o_seg = w; w += 24 * I;
  L.work_words = w;
  return L;
}

struct MoHostExec {
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() const {}
  void argmax_first(double &, int &) const {}
};

// Polynome::Compute / ComputeDerivative (Polynome.cpp:44-64) on nc coefficients
WG_MO_INLINE double mo_poly(const double *c, int nc, double t) {
  double r = 0.0, pt = 1.0;
  for (int i = 0; i < nc; i++) {
    r += c[i] * pt;
    pt *= t;
  }
  return r;
}
WG_MO_INLINE double mo_dpoly(const double *c, int nc, double t) {
  double r = 0, pt = 1;
  for (int i = 1; i < nc; i++) {
    r += i * c[i] * pt;
    pt *= t;
  }
  return r;
}

// the coefficients of axis a (0 x, 1 y: Polynome5::SetParameters with no initial acceleration; 2 z: Polynome4; 3 .. 5 theta,
// omega, omega2: Polynome3) over FT from p0 with speed v0 to FP (FootTrajectoryGenerationStandard.cpp:188-227).  c[6], unused = 0.
WG_MO_INLINE void mo_foot_axis(int a, double FT, double FP, double p0, double v0, double *c) {
  for (int i = 0; i < 6; i++) c[i] = 0.0;
  if (a < 2) {                                                 // PolynomeFoot.cpp:226-240
    const double InitAcc = 0.0;
    double tmp;
    c[0] = p0;
    c[1] = v0;
    c[2] = InitAcc / 2.0;
    tmp = FT * FT * FT;
    c[3] = (-3.0 / 2.0 * InitAcc * FT * FT - 6.0 * v0 * FT - 10.0 * p0 + 10.0 * FP) / tmp;
    tmp = tmp * FT;
    c[4] = (3.0 / 2.0 * InitAcc * FT * FT + 8.0 * v0 * FT + 15.0 * p0 - 15.0 * FP) / tmp;
    tmp = tmp * FT;
    c[5] = (-1.0 / 2.0 * InitAcc * FT * FT - 3.0 * v0 * FT - 6.0 * p0 + 6.0 * FP) / tmp;
  } else if (a == 2) {                                         // :122-146, FP is the height in the middle
    double tmp;
    c[0] = p0;
    c[1] = v0;
    tmp = FT * FT;
    if (tmp != 0.0) {
      c[2] = (-4.0 * v0 * FT - 11.0 * p0 + 16.0 * FP) / tmp;
      tmp = tmp * FT;
      c[3] = (5.0 * v0 * FT + 18.0 * p0 - 32.0 * FP) / tmp;
      tmp = tmp * FT;
      c[4] = (-2.0 * v0 * FT - 8.0 * p0 + 16.0 * FP) / tmp;
    }
  } else {                                                     // :59-79
    double tmp;
    c[0] = p0;
    c[1] = v0;
    tmp = FT * FT;
    if (FT != 0.0) {
      c[2] = (3 * FP - 3 * p0 - 2 * v0 * FT) / tmp;
      c[3] = (v0 * FT + 2 * p0 - 2 * FP) / (tmp * FT);
    }
  }
}
WG_MO_INLINE int mo_foot_nc(int a) { return a < 2 ? 6 : (a == 2 ? 5 : 4); }

// InitializeBasicVariables :172-197
WG_MO_INLINE double mo_dT(const wg_morisawa_model_t &m, int j, int I) {
  if (j == 0 || j == I - 1) return m.t_single * 3.0;
  return j % 2 == 0 ? m.t_single : m.t_double;
}
// the sum of the interval times in index order from 0.0: ComputePreviewControlTimeWindow (AnalyticalMorisawaAbstract.hh:266-271),
// SetStartingTimeIntervalsAndHeightVariation's reftime (AnalyticalZMPCOGTrajectory.cpp:300-305).  upto = I: the whole walk.
WG_MO_INLINE double mo_tref(const wg_morisawa_model_t &m, int upto, int I) {
  double reftime = 0;
  for (int j = 0; j < upto; j++) reftime += mo_dT(m, j, I);
  return reftime;
}
WG_MO_INLINE bool mo_time_ok(double t) { return mo_finite(t) && t > 0.0; }
// what the model alone decides: times, step height, omega
WG_MO_INLINE bool mo_model_ok(const wg_morisawa_model_t &m) {
  return mo_time_ok(m.T) && mo_time_ok(m.t_single) && mo_time_ok(m.t_double) && mo_finite(m.step_height) && mo_finite(m.omega);
}

// FillQueues' loop (:2242) on the trajectory's own clock: t_start, then one addition of T per sample, while t <= the sum of the
// interval times.  The sample at exactly that sum exists only if the additions land on or below it: with the reference's short
// walk (7 steps from 2 t_single at T = 0.005) they end 1e-13 above it and the walk has 1588 samples, the rows of its golden file.
// cap: the family's own, WG_MORISAWA_MAX_STEPS or WG_MORISAWA_LONG_MAX_STEPS
WG_MO_INLINE int mo_length(const wg_morisawa_model_t &m, int S, double t_start, int cap = WG_MORISAWA_MAX_STEPS) {
  if (!mo_model_ok(m) || S < 2 || S > cap || !mo_finite(t_start) || t_start < 0.0) return WG_MORISAWA_BAD_INPUT;
  const double total = mo_tref(m, 2 * S + 1, 2 * S + 1);
  int n = 0;
  for (double t = t_start; t <= total; t += m.T) {
    if (n == (1 << 24)) return WG_MORISAWA_CAPACITY;
    n++;
  }
  return n;
}

// ---- the serial part of InitializeFromRelativeSteps (:204-539): support feet, and per interval each foot's start and target ------
struct MoFoot { double p[6]; };          // x y z theta omega omega2; every speed of the reference's records is 0 on this path
WG_MO_INLINE void mo_seg_put(double *W, const MoLayout &L, int idx, const MoFoot &li, const MoFoot &lf, int lnat, const MoFoot &ri,
                             const MoFoot &rf, int rnat) {
  double *s = W + L.o_seg + 24 * idx;
  for (int a = 0; a < 6; a++) { s[a] = li.p[a]; s[6 + a] = lf.p[a]; s[12 + a] = ri.p[a]; s[18 + a] = rf.p[a]; }
  int *nat = reinterpret_cast<int *>(W + L.o_nat);
  nat[idx] = lnat;
  nat[L.imax + idx] = rnat;
}
WG_MO_HD inline void mo_feet_chain(const wg_morisawa_model_t &m, const wg_rel_step_t *steps, int S, const double *feet6, double *W,
                                   const MoLayout &L) {
  MoFoot Li, Ri, Lf, Rf;
  for (int a = 0; a < 6; a++) Li.p[a] = Ri.p[a] = Lf.p[a] = Rf.p[a] = 0.0;
  Li.p[0] = feet6[0]; Li.p[1] = feet6[1]; Li.p[3] = feet6[2];
  Ri.p[0] = feet6[3]; Ri.p[1] = feet6[4]; Ri.p[3] = feet6[5];
  int lnat = 0, rnat = 0;
  // who is the first support foot (:218-241, IgnoreFirst = true)
  int SupportFoot = 1;
  double CurrentAbsTheta, c, s, MM[2][2], Or[2][2], CS[2][3], v2[2];
  if (steps[0].sy < 0) {
    SupportFoot = -1;
    CurrentAbsTheta = Ri.p[3]; v2[0] = Ri.p[0]; v2[1] = Ri.p[1];
  } else {
    CurrentAbsTheta = Li.p[3]; v2[0] = Li.p[0]; v2[1] = Li.p[1];
  }
  c = wg_cos(CurrentAbsTheta * kMoPi / 180.0);
  s = wg_sin(CurrentAbsTheta * kMoPi / 180.0);
  CS[0][0] = c; CS[0][1] = -s; CS[1][0] = s; CS[1][1] = c;
  CS[0][2] = v2[0]; CS[1][2] = v2[1];
  int idx = 0;
  double *sup = W + L.o_sup;
  for (int i = 0; i < S; i++) {
    if (i != 0) {                                              // the double support before step i (:288-311)
      Li.p[2] = 0; lnat = 11;
      Ri.p[2] = 0; rnat = 9;
      mo_seg_put(W, L, idx, Li, Li, lnat, Ri, Ri, rnat);
      idx++;
    }
    c = wg_cos(steps[i].theta * kMoPi / 180.0);
    s = wg_sin(steps[i].theta * kMoPi / 180.0);
    MM[0][0] = c; MM[0][1] = -s; MM[1][0] = s; MM[1][1] = c;
    CurrentAbsTheta += steps[i].theta;
    for (int k = 0; k < 2; k++)
      for (int l = 0; l < 2; l++) {
        double t = 0;                                          // MAL_RET_A_by_B: the row-by-column sums from 0
        for (int q = 0; q < 2; q++) t += MM[k][q] * CS[q][l];
        Or[k][l] = t;
      }
    for (int k = 0; k < 2; k++) {
      double t = 0;
      t += Or[k][0] * steps[i].sx;
      t += Or[k][1] * steps[i].sy;
      v2[k] = t;
    }
    if (i > 0) {
      for (int k = 0; k < 2; k++)
        for (int l = 0; l < 2; l++) CS[k][l] = Or[k][l];
      for (int k = 0; k < 2; k++) CS[k][2] += v2[k];
      MoFoot &swing = SupportFoot == 1 ? Rf : Lf;
      swing.p[0] = CS[0][2]; swing.p[1] = CS[1][2]; swing.p[2] = m.step_height;
      swing.p[3] = CurrentAbsTheta; swing.p[4] = m.omega; swing.p[5] = 0.0;
      if (SupportFoot == 1) {
        rnat = 1;
        Lf = Li; Lf.p[2] = 0.0; lnat = -1;
      } else {
        lnat = 1;
        Rf = Ri; Rf.p[2] = 0.0; rnat = -1;                     // :417-420: the dz the reference clears here is the LEFT foot's;
      }                                                        // every dz is 0 on this path, so nothing is left to reproduce
    } else {                                                   // :424-448
      Lf = Li; Lf.p[2] = 0.0; Lf.p[4] = 0.0; Lf.p[5] = 0.0; lnat = 11;
      Rf = Ri; Rf.p[2] = 0.0; Rf.p[4] = 0.0; Rf.p[5] = 0.0; rnat = 9;
    }
    if (i != 0) {                                              // the single support of step i (:450-497)
      mo_seg_put(W, L, idx, Li, Lf, lnat, Ri, Rf, rnat);
      idx++;
    }
    if (i == 0 || i == S - 1) {                                // :499-524: the first double support, the two last ones
      const int limitk = i == S - 1 ? 2 : 1;
      for (int lk = 0; lk < limitk; lk++) {
        Lf.p[2] = 0; lnat = -1;
        Rf.p[2] = 0; rnat = -1;
        mo_seg_put(W, L, idx, Lf, Lf, lnat, Rf, Rf, rnat);
        idx++;
      }
    }
    Li = Lf; Ri = Rf;
    sup[3 * i + 0] = CS[0][2]; sup[3 * i + 1] = CS[1][2]; sup[3 * i + 2] = CurrentAbsTheta;
    if (i > 0) SupportFoot = -SupportFoot;
  }
}

// ---- one row of Z (:944-1164): its non-zeros, z[c] for the row's own columns c and nothing else.  They lie in columns
// r - 5 .. r + 4 whatever I is (the start block reaches five to the left, the rows of interval I - 2 four to the right), so the
// band form hands in z = band row - (r - 5) ----------------------------------------------------------------------------------------
WG_MO_INLINE void mo_z_fill(int r, int I, const double *dT, const double *om, const double *chv, const double *shv, double *z) {
  const double T0 = dT[0], O0 = om[0], Sq0 = O0 * O0;
  if (r == 0) { z[0] = 2.0 / Sq0; z[3] = 1.0; return; }        // BuildingTheZMatrix :1125-1129
  if (r == 1) { z[1] = 6.0 / Sq0; z[4] = O0; return; }
  if (r < 6) {                                                 // ComputeZ1
    const double c0 = chv[0], s0 = shv[0];
    double Deltat;
    if (r == 2) {
      Deltat = T0 * T0;
      z[0] = Deltat + 2.0 / Sq0;
      Deltat *= T0;
      z[1] = Deltat + T0 * 6.0 / Sq0;
      Deltat *= T0;
      z[2] = Deltat;
      z[3] = c0; z[4] = s0; z[5] = -1.0;
    } else if (r == 3) {
      Deltat = T0;
      z[0] = 2 * Deltat;
      Deltat *= T0;
      z[1] = 3 * Deltat + 6.0 / Sq0;
      Deltat *= T0;
      z[2] = 4 * Deltat;
      z[3] = O0 * s0; z[4] = O0 * c0; z[6] = -O0;
    } else if (r == 4) {
      Deltat = T0 * T0;
      z[0] = Deltat;
      Deltat *= T0;
      z[1] = Deltat;
      Deltat *= T0;
      z[2] = Deltat - 12 * T0 * T0 / Sq0;
    } else {
      Deltat = T0;
      z[0] = 2.0 * Deltat;
      Deltat *= T0;
      z[1] = 3.0 * Deltat;
      Deltat *= T0;
      z[2] = 4 * Deltat - 24.0 * T0 / Sq0;
    }
    return;
  }
  const double Om = om[I - 1];
  if (r < 2 * I + 2) {                                         // ComputeZj of interval j = 1 .. I - 2
    const int j = 1 + (r - 6) / 2, col = 5 + 2 * (j - 1);
    const double Oj = om[j], c0 = chv[j], s0 = shv[j];
    if (((r - 6) & 1) == 0) {
      z[col] = c0; z[col + 1] = s0;
      if (j != I - 2) z[col + 2] = -1.0;
      else { z[col + 2] = -2.0 / (Om * Om); z[col + 5] = -1.0; }
    } else {
      z[col] = Oj * s0; z[col + 1] = Oj * c0;
      if (j != I - 2) z[col + 3] = -Oj;
      else { z[col + 3] = -6.0 / (Om * Om); z[col + 6] = -Om; }
    }
    return;
  }
  {                                                            // ComputeZm
    const int col = 2 * I + 1, q = r - (2 * I + 2);
    const double Tm = dT[I - 1], Sqm = Om * Om, c0 = chv[I - 1], s0 = shv[I - 1];
    double Deltat;
    if (q == 0) {
      Deltat = Tm;
      Deltat *= Tm;
      z[col] = Deltat + 2.0 / Sqm;
      Deltat *= Tm;
      z[col + 1] = Deltat + Tm * 6.0 / Sqm;
      Deltat *= Tm;
      z[col + 2] = Deltat;
      z[col + 3] = c0; z[col + 4] = s0;
    } else if (q == 1) {
      Deltat = Tm;
      z[col] = 2 * Deltat;
      Deltat *= Tm;
      z[col + 1] = 3 * Deltat + 6.0 / Sqm;
      Deltat *= Tm;
      z[col + 2] = 4 * Deltat;
      z[col + 3] = Om * s0; z[col + 4] = Om * c0;
    } else if (q == 2) {
      Deltat = Tm * Tm;
      z[col] = Deltat;
      Deltat *= Tm;
      z[col + 1] = Deltat;
      Deltat *= Tm;
      z[col + 2] = Deltat - 12 * Tm * Tm / Sqm;
    } else {
      Deltat = Tm;
      z[col] = 2 * Deltat;
      Deltat *= Tm;
      z[col + 1] = 3 * Deltat;
      Deltat *= Tm;
      z[col + 2] = 4 * Deltat - 24.0 * Tm / Sqm;
    }
  }
}
// the dense form: row r into z[0 .. n), everything else of the row zero
WG_MO_HD inline void mo_z_row(int r, int I, const double *dT, const double *om, const double *chv, const double *shv, double *z) {
  const int n = 2 * I + 6;
  for (int c = 0; c < n; c++) z[c] = 0.0;
  mo_z_fill(r, I, dT, om, chv, shv, z);
}

// ---- one entry of w (ComputeW :831-942); cog: the CoG polynomials of the axis [I][5], zp: its ZMP profile ----------------------
WG_MO_HD inline double mo_w_entry(int e, int I, const double *dT, const double *cog, const double *zp, double InitialCoMPos,
                                  double InitialCoMSpeed, double FinalCoMPos) {
  if (e == 0) return InitialCoMPos - zp[0];
  if (e == 1) return InitialCoMSpeed;
  if (e < 6) {                                                 // j == 1
    const double *Next = cog + 5;
    if (e == 2) return Next[0] - zp[0];
    if (e == 3) return Next[1];
    return 0;
  }
  if (e < 2 * I + 2) {                                         // j = 2 .. I - 1, two entries each
    const int j = 2 + (e - 6) / 2;
    const double *Coeffs = cog + 5 * (j - 1), *Next = cog + 5 * j;
    double r1 = 0.0, r2 = 0.0;
    double deltat1 = 1.0, deltat2 = 1.0;
    for (unsigned int k = 0; k < 4; k++) {                     // interval j - 1 is a cubic: four coefficients
      r1 += Coeffs[k] * deltat1;
      deltat1 *= dT[j - 1];
      if (k > 0) {
        r2 += k * Coeffs[k] * deltat2;
        deltat2 *= dT[j - 1];
      }
    }
    if (((e - 6) & 1) == 0) return j != I - 1 ? Next[0] - r1 : zp[j - 1] - r1;
    return j != I - 1 ? Next[1] - r2 : -r2;
  }
  const int q = e - (2 * I + 2);
  if (q == 0 || q == 2) return FinalCoMPos - zp[I - 2];
  return 0.0;
}

// ---- LU of the n x n matrix a (rows `pitch` apart) with both right-hand sides, then both back substitutions ----------------------
// Right-looking, partial pivoting: the pivot of column k is the first row of largest |a_ik| among i >= k, the multiplier is
// a_ik / a_kk, an update is a product and then a difference.  The rows k and p swap whole (the multipliers of earlier columns
// with them, as dgetrf does), so that P Z = L U with piv as LAPACK's ipiv (0-based): a later right-hand side is solved from the
// block alone.  The right-hand sides are eliminated along with the columns -- the forward substitution in its column order --
// and U y = b is solved column by column from the last: y_c = b_c / u_cc, then b_i -= u_ic y_c for i < c.  An element's sequence
// of operations is the same whichever lane owns its row.  false: a zero or non-finite pivot.
template <class X>
WG_MO_HD inline bool mo_lu(const X x, int n, double *a, int pitch, int *piv, double *b0, double *b1) {
  const int l0 = x.lane(), S = x.lanes();
  for (int k = 0; k < n; k++) {
    double best = -1.0;
    int p = -1;
    for (int i = k + ((l0 - k % S + S) % S); i < n; i += S) {  // the rows i >= k this lane owns (i = l0 mod S), ascending
      const double raw = mo_abs(a[i * pitch + k]);
      const double v = mo_finite(raw) ? raw : __builtin_huge_val();
      if (v > best) { best = v; p = i; }
    }
    x.argmax_first(best, p);
    if (!(best > 0.0) || !mo_finite(best)) return false;
    if (l0 == 0) piv[k] = p;
    if (p != k) {
      for (int c = l0; c < n; c += S) {
        const double t = a[k * pitch + c];
        a[k * pitch + c] = a[p * pitch + c];
        a[p * pitch + c] = t;
      }
      if (l0 == 0) {
        double t = b0[k]; b0[k] = b0[p]; b0[p] = t;
        t = b1[k]; b1[k] = b1[p]; b1[p] = t;
      }
    }
    x.sync();
    const double akk = a[k * pitch + k];
    for (int i = k + 1 + ((l0 - (k + 1) % S + S) % S); i < n; i += S) {
      const double mlt = a[i * pitch + k] / akk;
      a[i * pitch + k] = mlt;
      for (int c = k + 1; c < n; c++) {
        const double prod = mlt * a[k * pitch + c];
        a[i * pitch + c] = a[i * pitch + c] - prod;
      }
      const double p0 = mlt * b0[k], p1 = mlt * b1[k];
      b0[i] = b0[i] - p0;
      b1[i] = b1[i] - p1;
    }
    x.sync();
  }
  for (int c = n - 1; c >= 0; c--) {
    const double ucc = a[c * pitch + c];
    const double y0 = b0[c] / ucc, y1 = b1[c] / ucc;
    x.sync();                                                  // every lane has read b[c] before its owner overwrites it
    if (l0 == c % S) { b0[c] = y0; b1[c] = y1; }
    for (int i = l0; i < c; i += S) {
      const double u = a[i * pitch + c];
      const double p0 = u * y0, p1 = u * y1;
      b0[i] = b0[i] - p0;
      b1[i] = b1[i] - p1;
    }
    x.sync();
  }
  return true;
}

// ---- the whole solve of one gait into the work area W (L.work_words doubles) ----------------------------------------------------
// WG_OK, or a code with W in an unspecified state: the caller copies the image out (mo_image_word) only on WG_OK, so a refused
// gait's block stays as it was.  z_dump (host only, may be null): Z before the elimination, n x n, rows n apart.
template <class X>
WG_MO_HD inline int mo_solve(const X x, const wg_morisawa_model_t &m, int smax, const wg_rel_step_t *steps, int S, const double *feet6,
                             const double *com3, double *W, const MoLayout &L, double *z_dump) {
  const int l0 = x.lane(), NL = x.lanes();
  if (S < 2 || S > smax || !mo_model_ok(m)) return WG_MORISAWA_BAD_INPUT;
  const double h = com3[2];
  if (!mo_time_ok(h) || !mo_finite(com3[0]) || !mo_finite(com3[1])) return WG_MORISAWA_BAD_INPUT;
  for (int k = 0; k < 6; k++)
    if (!mo_finite(feet6[k])) return WG_MORISAWA_BAD_INPUT;
  for (int i = 0; i < S; i++)
    if (!mo_finite(steps[i].sx) || !mo_finite(steps[i].sy) || !mo_finite(steps[i].theta)) return WG_MORISAWA_BAD_INPUT;
  const int I = 2 * S + 1, n = 2 * I + 6, P = L.nmax + 1;
  const double omega = sqrt(kMoG / (h - 0.0));                 // BuildingTheZMatrix :1106, lZMP = 0 (:387)
  if (!mo_args_ok(m, omega)) return WG_MORISAWA_BAD_INPUT;

  for (int e = l0; e < L.work_words; e += NL) W[e] = 0.0;
  x.sync();
  double *dT = W + L.o_dT, *om = W + L.o_om, *tref = W + L.o_tref;
  double *chv = W + L.o_vx, *shv = W + L.o_wx;                 // cosh, sinh of omega_j dT_j, until the weights of x take their place
  double *zpx = W + L.o_zpx, *zpy = W + L.o_zpy, *sup = W + L.o_sup;
  double *rhs = W + L.o_rhs, *a = W + L.o_lu;
  int *hdr = reinterpret_cast<int *>(W), *piv = reinterpret_cast<int *>(W + L.o_piv);

  // ---- interval times, their running sums, omega_j, cosh / sinh of omega_j dT_j; lane 0: the feet chain ----
  for (int j = l0; j < I; j += NL) {
    dT[j] = mo_dT(m, j, I);
    om[j] = omega;
    tref[j] = mo_tref(m, j, I);
    mo_coshsinh(omega * dT[j], chv[j], shv[j]);
  }
  if (l0 == 0) {
    hdr[0] = S; hdr[1] = I; hdr[2] = n; hdr[3] = smax;
    W[2] = h;
    W[3] = mo_tref(m, I, I);
    mo_feet_chain(m, steps, S, feet6, W, L);
  }
  x.sync();

  // ---- the ZMP profile (:422-476): the start CoM, every support foot twice, the middle of the last two for the last two ----
  const double finx = 0.5 * (sup[3 * (S - 2)] + sup[3 * (S - 1)]), finy = 0.5 * (sup[3 * (S - 2) + 1] + sup[3 * (S - 1) + 1]);
  for (int j = l0; j < I; j += NL) {
    zpx[j] = j == 0 ? com3[0] : (j >= 2 * S - 1 ? finx : sup[3 * ((j - 1) / 2)]);
    zpy[j] = j == 0 ? com3[1] : (j >= 2 * S - 1 ? finy : sup[3 * ((j - 1) / 2) + 1]);
  }
  // ---- the feet: per interval, foot and axis one polynomial (SetAnInterval :107-166) ----
  for (int e = l0; e < I * 12; e += NL) {
    const int j = e / 12, f = (e - 12 * j) / 6, ax = e - 12 * j - 6 * f;
    const double *sg = W + L.o_seg + 24 * j + 12 * f;
    mo_foot_axis(ax, dT[j], sg[6 + ax], sg[ax], 0.0, W + (f ? L.o_right : L.o_left) + 36 * j + 6 * ax);
  }
  x.sync();

  // ---- Building3rdOrderPolynomial for the interior intervals (AnalyticalZMPCOGTrajectory.cpp:425-456), both axes ----
  for (int e = l0; e < 2 * (I - 2); e += NL) {
    const int ax = e / (I - 2), j = 1 + (e - ax * (I - 2));
    const double *zp = ax ? zpy : zpx;
    double *Zc = W + (ax ? L.o_zy : L.o_zx) + 5 * j, *Cc = W + (ax ? L.o_cy : L.o_cx) + 5 * j;
    const double lTj = dT[j], Omegac = om[j];
    Zc[0] = zp[j - 1];
    Zc[1] = 0;
    Zc[2] = (zp[j] - zp[j - 1]) * 3.0 / (lTj * lTj);
    Zc[3] = -2.0 * Zc[2] / (3.0 * lTj);
    Cc[3] = Zc[3];
    Cc[2] = Zc[2];
    Cc[1] = Zc[1] + Cc[3] * 6 / (Omegac * Omegac);
    Cc[0] = Zc[0] + Cc[2] * 2 / (Omegac * Omegac);
  }
  x.sync();

  // ---- Z row by row, w entry by entry (x: CoM speed 0 at the start, :538-542) ----
  for (int r = l0; r < n; r += NL) mo_z_row(r, I, dT, om, chv, shv, a + r * P);
  for (int e = l0; e < 2 * n; e += NL) {
    const int ax = e / n, q = e - ax * n;
    const double v = mo_w_entry(q, I, dT, W + (ax ? L.o_cy : L.o_cx), ax ? zpy : zpx, ax ? com3[1] : com3[0], 0.0, ax ? finy : finx);
    rhs[ax * L.nmax + q] = v;
    rhs[(2 + ax) * L.nmax + q] = v;
  }
  x.sync();
  if (z_dump) {
    for (int e = l0; e < n * n; e += NL) z_dump[e] = a[(e / n) * P + (e % n)];
    x.sync();
  }

  if (!mo_lu(x, n, a, P, piv, rhs + 2 * L.nmax, rhs + 3 * L.nmax)) return WG_MORISAWA_SINGULAR;

  // ---- TransfertTheCoefficientsToTrajectories (:1166-1233), per axis: the weights, the two quartics and their ZMP twins ----
  for (int e = l0; e < 2 * I; e += NL) {
    const int ax = e / I, j = e - ax * I;
    const double *y = rhs + (2 + ax) * L.nmax;
    const int at = j < I - 1 ? 3 + 2 * j : 2 * I + 4;
    W[(ax ? L.o_vy : L.o_vx) + j] = y[at];
    W[(ax ? L.o_wy : L.o_wx) + j] = y[at + 1];
  }
  for (int e = l0; e < 4; e += NL) {
    const int ax = e >> 1, last = e & 1, j = last ? I - 1 : 0;
    const double *y = rhs + (2 + ax) * L.nmax + (last ? 2 * I + 1 : 0);
    const double *zp = ax ? zpy : zpx;
    double *Cc = W + (ax ? L.o_cy : L.o_cx) + 5 * j, *Zc = W + (ax ? L.o_zy : L.o_zx) + 5 * j;
    for (int k = 2; k <= 4; k++) Cc[k] = y[k - 2];
    Cc[1] = Cc[3] * 6.0 / (om[j] * om[j]);
    Cc[0] = zp[j] + Cc[2] * 2.0 / (om[j] * om[j]);
    // TransfertOneIntervalCoefficientsFromCOGTrajectoryToZMPOne (AnalyticalZMPCOGTrajectory.cpp:386-410): sTc is the
    // reference's |9.86 / (z_com - z_zmp)|, the divisions are its own
    const double sTc = mo_abs(kMoG / (h - 0.0));
    Zc[3] = Cc[3];
    Zc[4] = Cc[4];
    for (unsigned int i = 0; i < 3; ++i) Zc[i] = Cc[i] - ((double)(i + 1.0) * (double)(i + 2.0)) * (Cc[i + 2] / sTc);
  }
  x.sync();
  return WG_OK;
}

// word e of the block from the work area: the image as it is, the LU rows closed up from pitch nmax + 1 to nmax, zeros behind
WG_MO_INLINE double mo_image_word(const double *W, const MoLayout &L, int e) {
  if (e < L.o_lu) return W[e];
  const int q = e - L.o_lu;
  if (q >= L.nmax * L.nmax) return 0.0;
  const int r = q / L.nmax;
  return W[L.o_lu + r * (L.nmax + 1) + (q - r * L.nmax)];
}

// ---- the long walk: Z as a band, up to WG_MORISAWA_LONG_MAX_STEPS steps ----------------------------------------------------------
// Z's non-zeros lie within kMoKl below and kMoKu above the diagonal for every S (mo_z_fill); partial pivoting inside the band lets
// U reach kMoKu + kMoKl to the right.  Row-band storage: position i keeps columns i - 5 .. i + 9 in 15 words, rows kMoBand = 16
// doubles apart, the 16th word zero.  The multipliers of column k stay at the positions where they were made and are not swapped
// by later steps (LAPACK's dgbtf2 / dgbtrs convention): a later right-hand side is solved by, for k ascending, swapping b_k and
// b_piv[k] and then taking the multipliers of positions k + 1 .. k + 5 times b_k off those entries.
constexpr int kMoKl = 5, kMoKu = 4, kMoKuu = kMoKu + kMoKl, kMoBand = 16;
WG_MO_INLINE int mo_band_at(int i, int c) { return i * kMoBand + (c - i + kMoKl); }

// The long block has the short block's sections in the short block's order up to o_piv -- mo_sample reads it through this layout
// unchanged -- then the band [nmax][16] in place of [nmax][nmax].  The header's word 4, the first behind the two doubles and zero
// in a short block, holds the int 1 (int kMoTagInt of the header).  work_words: see mo_work_long.
constexpr int kMoTagInt = 8;
WG_MO_INLINE MoLayout mo_layout_long(int smax) {
  MoLayout L = mo_layout(smax);
  L.words = (L.o_lu + L.nmax * kMoBand + 15) & ~15;
  L.o_seg = -1;
  L.work_words = L.o_lu + L.nmax * kMoBand - 72 * L.imax;
  return L;
}
// The work area of the long solve: the image without the feet's polynomials (72 doubles per interval, which go from the lanes'
// registers to the block), so every section from o_nat on sits 72 imax lower.  The foot records of mo_feet_chain (24 doubles per
// interval) share the band's words, 24 imax <= 16 nmax: they are there before the band is built and again after it has left.
// 19 080 B at smax = 15, 38 800 B at 32, 75 920 B at 64: 8, 4 and 2 gaits on a CU of 160 KiB.
WG_MO_INLINE MoLayout mo_work_long(const MoLayout &L) {
  MoLayout Lw = L;
  const int d = 72 * L.imax;
  Lw.o_left = Lw.o_right = -1;
  Lw.o_nat -= d; Lw.o_zpx -= d; Lw.o_zpy -= d; Lw.o_sup -= d; Lw.o_rhs -= d; Lw.o_piv -= d; Lw.o_lu -= d;
  Lw.o_seg = Lw.o_lu;
  return Lw;
}
// word e of the long block from the work area, for the sections the work area holds (e outside [o_left, o_nat)); zeros behind
WG_MO_INLINE double mo_image_word_long(const double *W, const MoLayout &L, int e) {
  if (e < L.o_left) return W[e];
  if (e >= L.o_lu + L.nmax * kMoBand) return 0.0;
  return W[e - 72 * L.imax];
}

// mo_lu restricted to the band: the same pivots and, element by element, the same operations in the same order minus the
// products with structural zeros, so the same values (at most the sign of a zero differs).  The pivot of column k is the first
// row of largest |a_ik| among k <= i <= min(n - 1, k + 5) -- six words that every lane reads and compares alike, no reduction --;
// the rows k and p swap over columns k .. k + 9 and the right-hand sides; the live window of step k is 5 rows x (9 columns + 2
// right-hand sides) = 55 elements, one per lane, behind the at most five multipliers a_ik / a_kk, a lane each.  U y = b column by
// column from the last, over rows c - 9 .. c - 1.  false: a zero or non-finite pivot.
template <class X>
WG_MO_HD inline bool mo_band_lu(const X x, int n, double *a, int *piv, double *b0, double *b1) {
  const int l0 = x.lane(), NL = x.lanes();
  constexpr int kCols = kMoKuu + 2;                            // 9 columns right of the pivot, then b0 and b1
  for (int k = 0; k < n; k++) {
    const int ilast = k + kMoKl < n - 1 ? k + kMoKl : n - 1, clast = k + kMoKuu < n - 1 ? k + kMoKuu : n - 1;
    double best = -1.0;
    int p = -1;
    for (int i = k; i <= ilast; i++) {
      const double raw = mo_abs(a[mo_band_at(i, k)]);
      const double v = mo_finite(raw) ? raw : __builtin_huge_val();
      if (v > best) { best = v; p = i; }
    }
    if (!(best > 0.0) || !mo_finite(best)) return false;
    if (l0 == 0) piv[k] = p;
    if (p != k) {
      for (int e = l0; e < kCols + 1; e += NL) {               // columns k .. k + 9, b0, b1
        const int c = k + e;
        if (e <= kMoKuu) {
          if (c <= clast) {
            const double t = a[mo_band_at(k, c)];
            a[mo_band_at(k, c)] = a[mo_band_at(p, c)];
            a[mo_band_at(p, c)] = t;
          }
        } else {
          double *b = e == kMoKuu + 1 ? b0 : b1;
          const double t = b[k]; b[k] = b[p]; b[p] = t;
        }
      }
    }
    x.sync();
    const double akk = a[mo_band_at(k, k)];
    for (int i = k + 1 + l0; i <= ilast; i += NL) a[mo_band_at(i, k)] = a[mo_band_at(i, k)] / akk;
    x.sync();
    for (int e = l0; e < kMoKl * kCols; e += NL) {
      const int r = e / kCols, q = e - r * kCols, i = k + 1 + r, c = k + 1 + q;
      if (i > ilast) continue;
      const double mlt = a[mo_band_at(i, k)];
      if (q < kMoKuu) {
        if (c <= clast) {
          const double prod = mlt * a[mo_band_at(k, c)];
          a[mo_band_at(i, c)] = a[mo_band_at(i, c)] - prod;
        }
      } else if (q == kMoKuu) {
        const double p0 = mlt * b0[k];
        b0[i] = b0[i] - p0;
      } else {
        const double p1 = mlt * b1[k];
        b1[i] = b1[i] - p1;
      }
    }
    x.sync();
  }
  for (int c = n - 1; c >= 0; c--) {
    const double ucc = a[mo_band_at(c, c)];
    const double y0 = b0[c] / ucc, y1 = b1[c] / ucc;
    x.sync();                                                  // every lane has read b[c] before lane 0 overwrites it
    if (l0 == 0) { b0[c] = y0; b1[c] = y1; }
    for (int e = l0; e < kMoKuu; e += NL) {
      const int i = c - 1 - e;
      if (i < 0) continue;
      const double u = a[mo_band_at(i, c)];
      const double p0 = u * y0, p1 = u * y1;
      b0[i] = b0[i] - p0;
      b1[i] = b1[i] - p1;
    }
    x.sync();
  }
  return true;
}

// what mo_solve refuses before it touches anything
WG_MO_HD inline bool mo_inputs_ok(const wg_morisawa_model_t &m, int smax, const wg_rel_step_t *steps, int S, const double *feet6,
                                  const double *com3) {
  if (S < 2 || S > smax || !mo_model_ok(m)) return false;
  const double h = com3[2];
  if (!mo_time_ok(h) || !mo_finite(com3[0]) || !mo_finite(com3[1])) return false;
  for (int k = 0; k < 6; k++)
    if (!mo_finite(feet6[k])) return false;
  for (int i = 0; i < S; i++)
    if (!mo_finite(steps[i].sx) || !mo_finite(steps[i].sy) || !mo_finite(steps[i].theta)) return false;
  const double omega = sqrt(kMoG / (h - 0.0));
  return mo_args_ok(m, omega);
}

// ---- the whole long solve of one gait: work area W (mo_layout_long's work_words doubles), block blk ------------------------------
// mo_solve's phases around what LDS holds.  Everything that can refuse comes first and writes W alone: the times, the feet chain
// (for the support feet that the ZMP profile and w need; its foot records lie where the band will), the cubics, w, then the band
// of Z and its factor.  blk is written only from there on, so a refused gait's block stays as it was: the image from W, then the
// feet -- the chain once more, its records now in the words the band has left, and each polynomial from its lane to the block.
// z_dump (host only, may be null): Z before the elimination in row-band form, n x 16.
template <class X>
WG_MO_HD inline int mo_solve_long(const X x, const wg_morisawa_model_t &m, int smax, const wg_rel_step_t *steps, int S,
                                  const double *feet6, const double *com3, double *W, const MoLayout &L, double *blk, double *z_dump) {
  const int l0 = x.lane(), NL = x.lanes();
  if (!mo_inputs_ok(m, smax, steps, S, feet6, com3)) return WG_MORISAWA_BAD_INPUT;
  const MoLayout Lw = mo_work_long(L);
  const int I = 2 * S + 1, n = 2 * I + 6;
  const double h = com3[2];
  const double omega = sqrt(kMoG / (h - 0.0));                 // BuildingTheZMatrix :1106, lZMP = 0 (:387)

  for (int e = l0; e < L.work_words; e += NL) W[e] = 0.0;
  x.sync();
  double *dT = W + Lw.o_dT, *om = W + Lw.o_om, *tref = W + Lw.o_tref;
  double *chv = W + Lw.o_vx, *shv = W + Lw.o_wx;               // cosh, sinh of omega_j dT_j, until the weights of x take their place
  double *zpx = W + Lw.o_zpx, *zpy = W + Lw.o_zpy, *sup = W + Lw.o_sup;
  double *rhs = W + Lw.o_rhs, *a = W + Lw.o_lu;
  int *hdr = reinterpret_cast<int *>(W), *piv = reinterpret_cast<int *>(W + Lw.o_piv);

  // ---- interval times, their running sums, omega_j, cosh / sinh of omega_j dT_j; lane 0: the feet chain ----
  for (int j = l0; j < I; j += NL) {
    dT[j] = mo_dT(m, j, I);
    om[j] = omega;
    tref[j] = mo_tref(m, j, I);
    mo_coshsinh(omega * dT[j], chv[j], shv[j]);
  }
  if (l0 == 0) {
    hdr[0] = S; hdr[1] = I; hdr[2] = n; hdr[3] = smax; hdr[kMoTagInt] = 1;
    W[2] = h;
    W[3] = mo_tref(m, I, I);
    mo_feet_chain(m, steps, S, feet6, W, Lw);
  }
  x.sync();

  // ---- the ZMP profile, the interior cubics, w: as in mo_solve ----
  const double finx = 0.5 * (sup[3 * (S - 2)] + sup[3 * (S - 1)]), finy = 0.5 * (sup[3 * (S - 2) + 1] + sup[3 * (S - 1) + 1]);
  for (int j = l0; j < I; j += NL) {
    zpx[j] = j == 0 ? com3[0] : (j >= 2 * S - 1 ? finx : sup[3 * ((j - 1) / 2)]);
    zpy[j] = j == 0 ? com3[1] : (j >= 2 * S - 1 ? finy : sup[3 * ((j - 1) / 2) + 1]);
  }
  x.sync();
  for (int e = l0; e < 2 * (I - 2); e += NL) {
    const int ax = e / (I - 2), j = 1 + (e - ax * (I - 2));
    const double *zp = ax ? zpy : zpx;
    double *Zc = W + (ax ? Lw.o_zy : Lw.o_zx) + 5 * j, *Cc = W + (ax ? Lw.o_cy : Lw.o_cx) + 5 * j;
    const double lTj = dT[j], Omegac = om[j];
    Zc[0] = zp[j - 1];
    Zc[1] = 0;
    Zc[2] = (zp[j] - zp[j - 1]) * 3.0 / (lTj * lTj);
    Zc[3] = -2.0 * Zc[2] / (3.0 * lTj);
    Cc[3] = Zc[3];
    Cc[2] = Zc[2];
    Cc[1] = Zc[1] + Cc[3] * 6 / (Omegac * Omegac);
    Cc[0] = Zc[0] + Cc[2] * 2 / (Omegac * Omegac);
  }
  x.sync();
  for (int e = l0; e < 2 * n; e += NL) {
    const int ax = e / n, q = e - ax * n;
    const double v = mo_w_entry(q, I, dT, W + (ax ? Lw.o_cy : Lw.o_cx), ax ? zpy : zpx, ax ? com3[1] : com3[0], 0.0, ax ? finy : finx);
    rhs[ax * L.nmax + q] = v;
    rhs[(2 + ax) * L.nmax + q] = v;
  }
  // ---- the band of Z over the chain's foot records, row by row ----
  for (int e = l0; e < L.nmax * kMoBand; e += NL) a[e] = 0.0;
  x.sync();
  for (int r = l0; r < n; r += NL) mo_z_fill(r, I, dT, om, chv, shv, a + mo_band_at(r, 0));
  x.sync();
  if (z_dump) {
    for (int e = l0; e < n * kMoBand; e += NL) z_dump[e] = a[e];
    x.sync();
  }

  if (!mo_band_lu(x, n, a, piv, rhs + 2 * L.nmax, rhs + 3 * L.nmax)) return WG_MORISAWA_SINGULAR;

  // ---- TransfertTheCoefficientsToTrajectories: as in mo_solve ----
  for (int e = l0; e < 2 * I; e += NL) {
    const int ax = e / I, j = e - ax * I;
    const double *y = rhs + (2 + ax) * L.nmax;
    const int at = j < I - 1 ? 3 + 2 * j : 2 * I + 4;
    W[(ax ? Lw.o_vy : Lw.o_vx) + j] = y[at];
    W[(ax ? Lw.o_wy : Lw.o_wx) + j] = y[at + 1];
  }
  for (int e = l0; e < 4; e += NL) {
    const int ax = e >> 1, last = e & 1, j = last ? I - 1 : 0;
    const double *y = rhs + (2 + ax) * L.nmax + (last ? 2 * I + 1 : 0);
    const double *zp = ax ? zpy : zpx;
    double *Cc = W + (ax ? Lw.o_cy : Lw.o_cx) + 5 * j, *Zc = W + (ax ? Lw.o_zy : Lw.o_zx) + 5 * j;
    for (int k = 2; k <= 4; k++) Cc[k] = y[k - 2];
    Cc[1] = Cc[3] * 6.0 / (om[j] * om[j]);
    Cc[0] = zp[j] + Cc[2] * 2.0 / (om[j] * om[j]);
    const double sTc = mo_abs(kMoG / (h - 0.0));               // AnalyticalZMPCOGTrajectory.cpp:401
    Zc[3] = Cc[3];
    Zc[4] = Cc[4];
    for (unsigned int i = 0; i < 3; ++i) Zc[i] = Cc[i] - ((double)(i + 1.0) * (double)(i + 2.0)) * (Cc[i + 2] / sTc);
  }
  x.sync();

  // ---- the image to the block; then the feet: the chain's records where the band was, a polynomial per lane to the block ----
  for (int e = l0; e < L.words; e += NL)
    if (e < L.o_left || e >= L.o_nat) blk[e] = mo_image_word_long(W, L, e);
  x.sync();
  if (l0 == 0) mo_feet_chain(m, steps, S, feet6, W, Lw);
  x.sync();
  for (int e = l0; e < L.imax * 12; e += NL) {
    const int j = e / 12, f = (e - 12 * j) / 6, ax = e - 12 * j - 6 * f;
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < I) {
      const double *sg = W + Lw.o_seg + 24 * j + 12 * f;
      mo_foot_axis(ax, dT[j], sg[6 + ax], sg[ax], 0.0, c);
    }
    double *out = blk + (f ? L.o_right : L.o_left) + 36 * j + 6 * ax;
    for (int k = 0; k < 6; k++) out[k] = c[k];
  }
  x.sync();
  return WG_OK;
}

// ---- a block as the sampler reads it -------------------------------------------------------------------------------------------
WG_MO_INLINE bool mo_block_ok(const double *blk, int smax) {
  const int *hdr = reinterpret_cast<const int *>(blk);
  return hdr[3] == smax && hdr[0] >= 2 && hdr[0] <= smax && hdr[1] == 2 * hdr[0] + 1 && hdr[2] == 2 * hdr[1] + 6;
}
WG_MO_INLINE bool mo_block_ok_long(const double *blk, int smax) {
  return mo_block_ok(blk, smax) && reinterpret_cast<const int *>(blk)[kMoTagInt] == 1;
}
struct MoSample {
  double zx, zy, com[4], left[6], right[6];
  int ltype, rtype;
};
// One sample at trajectory time t: GetIntervalIndexFromTime (AnalyticalZMPCOGTrajectory.cpp:491-507 as FillQueues calls it: from
// interval 0, m_Sensitivity = 0, the earlier interval wins at a boundary), then ComputeZMP / ComputeCOM / ComputeCOMSpeed by
// interval (:175-196, 276-282) and both feet (FootTrajectoryGenerationMultiple.cpp:128-135).
WG_MO_HD inline void mo_sample(const double *blk, const MoLayout &L, double t, MoSample &o) {
  const int I = reinterpret_cast<const int *>(blk)[1];
  const double *dT = blk + L.o_dT, *tref = blk + L.o_tref;
  int j = I - 1;
  for (int lj = 0; lj < I; lj++)
    if (t >= tref[lj] && t <= tref[lj] + dT[lj]) { j = lj; break; }
  const double deltaj = t - tref[j], omj = blk[L.o_om + j];
  const int nc = (j == 0 || j == I - 1) ? 5 : 4;
  double ch, sh;
  mo_coshsinh(omj * deltaj, ch, sh);
  for (int ax = 0; ax < 2; ax++) {
    const double V = blk[(ax ? L.o_vy : L.o_vx) + j], Wt = blk[(ax ? L.o_wy : L.o_wx) + j];
    const double *Cc = blk + (ax ? L.o_cy : L.o_cx) + 5 * j;
    double r = ch * V + sh * Wt;
    r += mo_poly(Cc, nc, deltaj);
    o.com[2 * ax] = r;
    r = omj * sh * V + omj * ch * Wt;
    r += mo_dpoly(Cc, nc, deltaj);
    o.com[2 * ax + 1] = r;
  }
  o.zx = mo_poly(blk + L.o_zx + 5 * j, nc, deltaj);
  o.zy = mo_poly(blk + L.o_zy + 5 * j, nc, deltaj);
  for (int a = 0; a < 6; a++) {
    o.left[a] = mo_poly(blk + L.o_left + 36 * j + 6 * a, mo_foot_nc(a), deltaj);
    o.right[a] = mo_poly(blk + L.o_right + 36 * j + 6 * a, mo_foot_nc(a), deltaj);
  }
  const int *nat = reinterpret_cast<const int *>(blk + L.o_nat);
  o.ltype = nat[j];
  o.rtype = nat[L.imax + j];
}

// samples of a walk whose interval times sum to `total` on the launch's clock (clock[k] = t_start + k additions of T, lcap + 1
// entries): the k with clock[k] <= total are a prefix, its size found by bisection.  lcap + 1: more than the arrays hold.
WG_MO_INLINE int mo_count(const double *clock, int lcap, double total) {
  int lo = 0, hi = lcap + 1;                                   // clock[k] <= total for k < lo, > total for k >= hi
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (clock[mid] <= total) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- the re-plan: a new walk on a solved block's timing, from its kept factor ----------------------------------------------------
// Z depends on the interval times, the CoM height and the step count alone (mo_z_fill), so a block solved for them -- the FACTOR
// BLOCK -- serves every plan (steps, initial feet, start CoM x and y) on that timing: mo_resolve / mo_resolve_long make the block
// that mo_solve / mo_solve_long would make for the plan, byte for byte, without building or eliminating Z (the reference's
// m_NeedToReset: ComputePolynomialWeights2 :263-357 factors once, ResetTheResolutionOfThePolynomial forgets the factor only when
// the times change).  What the timing fixes is copied from the factor block -- header, dT, omega, tref, pivots, factor --, what
// the plan decides runs through the solves' own helpers, and both right-hand sides go through the stored factor with the
// products and differences they meet inside mo_lu / mo_band_lu, in the same order: k ascending, a product and then a difference.
WG_MO_INLINE bool mo_same_bits(double a, double b) {
  long long x, y;
  __builtin_memcpy(&x, &a, sizeof x);
  __builtin_memcpy(&y, &b, sizeof y);
  return x == y;
}
// May gait (m, steps, feet6, com3) be re-planned from the block fac of this family and smax?  fac is a solved block of the family
// (a short block carries no tag, a long block the tag), of this smax; the model's times give the block's dT bit for bit, the
// height is the block's bit for bit, and mo_solve would not refuse the plan at the block's step count.
WG_MO_HD inline bool mo_replan_ok(const wg_morisawa_model_t &m, int smax, bool lng, const double *fac, const MoLayout &L,
                                  const wg_rel_step_t *steps, const double *feet6, const double *com3) {
  const int *hdr = reinterpret_cast<const int *>(fac);
  if (!mo_block_ok(fac, smax) || hdr[kMoTagInt] != (lng ? 1 : 0)) return false;
  const int S = hdr[0], I = hdr[1];
  if (!mo_inputs_ok(m, smax, steps, S, feet6, com3)) return false;
  if (!mo_same_bits(com3[2], fac[2])) return false;
  for (int j = 0; j < I; j++)
    if (!mo_same_bits(mo_dT(m, j, I), fac[L.o_dT + j])) return false;
  return true;
}
// The pivots index the right-hand sides, so a block is a factor block only with each of them among its column's rows: k <= piv[k]
// < n, and within the band's reach (n for the dense factor, kMoKl for the band)
WG_MO_INLINE bool mo_piv_ok(const int *piv, int n, int reach) {
  bool ok = true;
  for (int k = 0; k < n; k++) ok = ok && piv[k] >= k && piv[k] < n && piv[k] - k <= reach;
  return ok;
}

// The phases of mo_solve between the feet chain and the elimination, on the work area W laid out by Lw (mo_layout's own layout,
// or mo_work_long's): the ZMP profile (:422-476), Building3rdOrderPolynomial for the interior intervals, w of x and y into rows 0
// and 1 of rhs and again into rows 2 and 3, where the substitution turns them into y.  dT, omega and the support feet are in W.
template <class X>
WG_MO_HD inline void mo_plan_w(const X x, int S, const double *com3, double *W, const MoLayout &Lw) {
  const int l0 = x.lane(), NL = x.lanes();
  const int I = 2 * S + 1, n = 2 * I + 6;
  const double *dT = W + Lw.o_dT, *om = W + Lw.o_om, *sup = W + Lw.o_sup;
  double *zpx = W + Lw.o_zpx, *zpy = W + Lw.o_zpy, *rhs = W + Lw.o_rhs;
  const double finx = 0.5 * (sup[3 * (S - 2)] + sup[3 * (S - 1)]), finy = 0.5 * (sup[3 * (S - 2) + 1] + sup[3 * (S - 1) + 1]);
  for (int j = l0; j < I; j += NL) {
    zpx[j] = j == 0 ? com3[0] : (j >= 2 * S - 1 ? finx : sup[3 * ((j - 1) / 2)]);
    zpy[j] = j == 0 ? com3[1] : (j >= 2 * S - 1 ? finy : sup[3 * ((j - 1) / 2) + 1]);
  }
  x.sync();
  for (int e = l0; e < 2 * (I - 2); e += NL) {
    const int ax = e / (I - 2), j = 1 + (e - ax * (I - 2));
    const double *zp = ax ? zpy : zpx;
    double *Zc = W + (ax ? Lw.o_zy : Lw.o_zx) + 5 * j, *Cc = W + (ax ? Lw.o_cy : Lw.o_cx) + 5 * j;
    const double lTj = dT[j], Omegac = om[j];
    Zc[0] = zp[j - 1];
    Zc[1] = 0;
    Zc[2] = (zp[j] - zp[j - 1]) * 3.0 / (lTj * lTj);
    Zc[3] = -2.0 * Zc[2] / (3.0 * lTj);
    Cc[3] = Zc[3];
    Cc[2] = Zc[2];
    Cc[1] = Zc[1] + Cc[3] * 6 / (Omegac * Omegac);
    Cc[0] = Zc[0] + Cc[2] * 2 / (Omegac * Omegac);
  }
  x.sync();
  for (int e = l0; e < 2 * n; e += NL) {
    const int ax = e / n, q = e - ax * n;
    const double v = mo_w_entry(q, I, dT, W + (ax ? Lw.o_cy : Lw.o_cx), ax ? zpy : zpx, ax ? com3[1] : com3[0], 0.0, ax ? finy : finx);
    rhs[ax * Lw.nmax + q] = v;
    rhs[(2 + ax) * Lw.nmax + q] = v;
  }
  x.sync();
}

// TransfertTheCoefficientsToTrajectories (:1166-1233) from y in rows 2 and 3 of rhs, as mo_solve has it behind its elimination
template <class X>
WG_MO_HD inline void mo_transfer(const X x, int S, double h, double *W, const MoLayout &Lw) {
  const int l0 = x.lane(), NL = x.lanes();
  const int I = 2 * S + 1;
  const double *om = W + Lw.o_om, *rhs = W + Lw.o_rhs;
  for (int e = l0; e < 2 * I; e += NL) {
    const int ax = e / I, j = e - ax * I;
    const double *y = rhs + (2 + ax) * Lw.nmax;
    const int at = j < I - 1 ? 3 + 2 * j : 2 * I + 4;
    W[(ax ? Lw.o_vy : Lw.o_vx) + j] = y[at];
    W[(ax ? Lw.o_wy : Lw.o_wx) + j] = y[at + 1];
  }
  for (int e = l0; e < 4; e += NL) {
    const int ax = e >> 1, last = e & 1, j = last ? I - 1 : 0;
    const double *y = rhs + (2 + ax) * Lw.nmax + (last ? 2 * I + 1 : 0);
    const double *zp = W + (ax ? Lw.o_zpy : Lw.o_zpx);
    double *Cc = W + (ax ? Lw.o_cy : Lw.o_cx) + 5 * j, *Zc = W + (ax ? Lw.o_zy : Lw.o_zx) + 5 * j;
    for (int k = 2; k <= 4; k++) Cc[k] = y[k - 2];
    Cc[1] = Cc[3] * 6.0 / (om[j] * om[j]);
    Cc[0] = zp[j] + Cc[2] * 2.0 / (om[j] * om[j]);
    const double sTc = mo_abs(kMoG / (h - 0.0));               // AnalyticalZMPCOGTrajectory.cpp:401
    Zc[3] = Cc[3];
    Zc[4] = Cc[4];
    for (unsigned int i = 0; i < 3; ++i) Zc[i] = Cc[i] - ((double)(i + 1.0) * (double)(i + 2.0)) * (Cc[i + 2] / sTc);
  }
  x.sync();
}

// Both right-hand sides through mo_lu's stored factor (P Z = L U, the multipliers swapped along with their rows as dgetrf leaves
// them): piv applied to b for k ascending, a lane per side; the unit-lower solve column by column, k ascending, lanes over the
// rows i > k, each with its row's owner in mo_lu; then U y = b as mo_lu's second loop.  An entry of b travels with its row, so
// at step k it meets the multiplier and the b_k it met inside mo_lu.
template <class X>
WG_MO_HD inline void mo_lu_resolve(const X x, int n, const double *a, int pitch, const int *piv, double *b0, double *b1) {
  const int l0 = x.lane(), S = x.lanes();
  for (int s = l0; s < 2; s += S) {
    double *b = s ? b1 : b0;
    for (int k = 0; k < n; k++) {
      const int p = piv[k];
      const double t = b[k]; b[k] = b[p]; b[p] = t;
    }
  }
  x.sync();
  for (int k = 0; k < n; k++) {
    const double bk0 = b0[k], bk1 = b1[k];
    for (int i = k + 1 + ((l0 - (k + 1) % S + S) % S); i < n; i += S) {
      const double mlt = a[i * pitch + k];
      const double p0 = mlt * bk0, p1 = mlt * bk1;
      b0[i] = b0[i] - p0;
      b1[i] = b1[i] - p1;
    }
    x.sync();
  }
  for (int c = n - 1; c >= 0; c--) {
    const double ucc = a[c * pitch + c];
    const double y0 = b0[c] / ucc, y1 = b1[c] / ucc;
    x.sync();                                                  // every lane has read b[c] before its owner overwrites it
    if (l0 == c % S) { b0[c] = y0; b1[c] = y1; }
    for (int i = l0; i < c; i += S) {
      const double u = a[i * pitch + c];
      const double p0 = u * y0, p1 = u * y1;
      b0[i] = b0[i] - p0;
      b1[i] = b1[i] - p1;
    }
    x.sync();
  }
}

// The same through mo_band_lu's factor, the dgbtrs procedure of include/wg_mpc.h: per k the swap of b_k and b_piv[k], a lane per
// side, then the multipliers of positions k + 1 .. k + 5 times b_k off those entries, a lane per position and side; then U y = b
// over rows c - 9 .. c - 1 as mo_band_lu's second loop.
template <class X>
WG_MO_HD inline void mo_band_resolve(const X x, int n, const double *a, const int *piv, double *b0, double *b1) {
  const int l0 = x.lane(), NL = x.lanes();
  for (int k = 0; k < n; k++) {
    const int ilast = k + kMoKl < n - 1 ? k + kMoKl : n - 1, p = piv[k];
    if (p != k)
      for (int s = l0; s < 2; s += NL) {
        double *b = s ? b1 : b0;
        const double t = b[k]; b[k] = b[p]; b[p] = t;
      }
    x.sync();
    for (int e = l0; e < 2 * kMoKl; e += NL) {
      const int s = e / kMoKl, i = k + 1 + (e - s * kMoKl);
      if (i > ilast) continue;
      double *b = s ? b1 : b0;
      const double prod = a[mo_band_at(i, k)] * b[k];
      b[i] = b[i] - prod;
    }
    x.sync();
  }
  for (int c = n - 1; c >= 0; c--) {
    const double ucc = a[mo_band_at(c, c)];
    const double y0 = b0[c] / ucc, y1 = b1[c] / ucc;
    x.sync();                                                  // every lane has read b[c] before lane 0 overwrites it
    if (l0 == 0) { b0[c] = y0; b1[c] = y1; }
    for (int e = l0; e < kMoKuu; e += NL) {
      const int i = c - 1 - e;
      if (i < 0) continue;
      const double u = a[mo_band_at(i, c)];
      const double p0 = u * y0, p1 = u * y1;
      b0[i] = b0[i] - p0;
      b1[i] = b1[i] - p1;
    }
    x.sync();
  }
}

// ---- the re-plan of one gait from the factor block fac into the work area W (mo_layout's work_words doubles) --------------------
// WG_OK, and the caller copies the image out (mo_image_word) as behind mo_solve; WG_MORISAWA_BAD_INPUT with W in an unspecified
// state (the pivots are looked at where they have been copied to).  The factor's rows go from the block's pitch nmax to the work area's nmax + 1 over consecutive words of the block.  fac is read
// only, and not through W: it must not overlap the block the caller writes.
template <class X>
WG_MO_HD inline int mo_resolve(const X x, const wg_morisawa_model_t &m, int smax, const double *fac, const wg_rel_step_t *steps,
                               const double *feet6, const double *com3, double *W, const MoLayout &L) {
  const int l0 = x.lane(), NL = x.lanes();
  if (!mo_replan_ok(m, smax, false, fac, L, steps, feet6, com3)) return WG_MORISAWA_BAD_INPUT;
  const int S = reinterpret_cast<const int *>(fac)[0], I = 2 * S + 1, n = 2 * I + 6, P = L.nmax + 1;

  for (int e = l0; e < L.work_words; e += NL) W[e] = 0.0;
  x.sync();
  // ---- what the timing fixes: header, dT, omega, tref; pivots and factor; lane 0: the feet chain ----
  for (int e = l0; e < L.o_zx; e += NL) W[e] = fac[e];
  for (int e = L.o_piv + l0; e < L.o_lu + L.nmax * L.nmax; e += NL) {
    const double v = fac[e];
    if (e < L.o_lu) { W[e] = v; continue; }
    const int q = e - L.o_lu, r = q / L.nmax;
    W[L.o_lu + r * P + (q - r * L.nmax)] = v;
  }
  if (l0 == 0) mo_feet_chain(m, steps, S, feet6, W, L);
  x.sync();
  if (!mo_piv_ok(reinterpret_cast<const int *>(W + L.o_piv), n, n)) return WG_MORISAWA_BAD_INPUT;
  // ---- what the plan decides: the feet's polynomials, the ZMP profile, the interior cubics, w ----
  const double *dT = W + L.o_dT;
  for (int e = l0; e < I * 12; e += NL) {
    const int j = e / 12, f = (e - 12 * j) / 6, ax = e - 12 * j - 6 * f;
    const double *sg = W + L.o_seg + 24 * j + 12 * f;
    mo_foot_axis(ax, dT[j], sg[6 + ax], sg[ax], 0.0, W + (f ? L.o_right : L.o_left) + 36 * j + 6 * ax);
  }
  mo_plan_w(x, S, com3, W, L);
  double *rhs = W + L.o_rhs;
  mo_lu_resolve(x, n, W + L.o_lu, P, reinterpret_cast<const int *>(W + L.o_piv), rhs + 2 * L.nmax, rhs + 3 * L.nmax);
  mo_transfer(x, S, com3[2], W, L);
  return WG_OK;
}

// ---- the long re-plan: work area W (mo_layout_long's work_words doubles), block blk -----------------------------------------------
// mo_solve_long's order turned round, since nothing can refuse behind the first test: the feet first -- the chain's records in
// the words the band will take, each polynomial from its lane to the block --, then the band from the factor block over those
// words, w, the substitution, and the image to the block as mo_solve_long writes it.
template <class X>
WG_MO_HD inline int mo_resolve_long(const X x, const wg_morisawa_model_t &m, int smax, const double *fac, const wg_rel_step_t *steps,
                                    const double *feet6, const double *com3, double *W, const MoLayout &L, double *blk) {
  const int l0 = x.lane(), NL = x.lanes();
  if (!mo_replan_ok(m, smax, true, fac, L, steps, feet6, com3)) return WG_MORISAWA_BAD_INPUT;
  const MoLayout Lw = mo_work_long(L);
  const int S = reinterpret_cast<const int *>(fac)[0], I = 2 * S + 1, n = 2 * I + 6;

  for (int e = l0; e < L.work_words; e += NL) W[e] = 0.0;
  x.sync();
  for (int e = l0; e < L.o_zx; e += NL) W[e] = fac[e];         // header, dT, omega, tref: the long layout's are the work area's
  for (int e = L.o_piv + l0; e < L.o_lu; e += NL) W[e - 72 * L.imax] = fac[e];
  if (l0 == 0) mo_feet_chain(m, steps, S, feet6, W, Lw);
  x.sync();
  if (!mo_piv_ok(reinterpret_cast<const int *>(W + Lw.o_piv), n, kMoKl)) return WG_MORISAWA_BAD_INPUT;   // blk is still untouched
  const double *dT = W + Lw.o_dT;
  for (int e = l0; e < L.imax * 12; e += NL) {
    const int j = e / 12, f = (e - 12 * j) / 6, ax = e - 12 * j - 6 * f;
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < I) {
      const double *sg = W + Lw.o_seg + 24 * j + 12 * f;
      mo_foot_axis(ax, dT[j], sg[6 + ax], sg[ax], 0.0, c);
    }
    double *out = blk + (f ? L.o_right : L.o_left) + 36 * j + 6 * ax;
    for (int k = 0; k < 6; k++) out[k] = c[k];
  }
  x.sync();
  // ---- the band, consecutive words of the factor block, over the chain's foot records ----
  for (int e = L.o_lu + l0; e < L.o_lu + L.nmax * kMoBand; e += NL) W[e - 72 * L.imax] = fac[e];
  mo_plan_w(x, S, com3, W, Lw);
  double *rhs = W + Lw.o_rhs;
  mo_band_resolve(x, n, W + Lw.o_lu, reinterpret_cast<const int *>(W + Lw.o_piv), rhs + 2 * L.nmax, rhs + 3 * L.nmax);
  mo_transfer(x, S, com3[2], W, Lw);
  for (int e = l0; e < L.words; e += NL)
    if (e < L.o_left || e >= L.o_nat) blk[e] = mo_image_word_long(W, L, e);
  x.sync();
  return WG_OK;
}

}  // namespace wg
