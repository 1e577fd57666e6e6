// wg_audit_math.hpp -- the walk audit's per-sample arithmetic, once, for the host call (wg_audit.cpp) and the kernels
// (wg_audit_device.hpp): which queue entry holds a sample's time, the rows' values and distances, the sample's margin, the
// reference's violation test, and the fold of samples (or of per-chunk partial results) into a gait's wg_zmp_audit_t.
//
//   ZMPConstrainedQPFastFormulation::ValidationConstraints    ZMPConstrainedQPFastFormulation.cpp:248-381 (the test at :322)
//   ZMPConstrainedQPFastFormulation::BuildConstraintMatrices  :785-796 (the entry search)
//
// Plain C++ that a HIP translation unit compiles for both sides (WG_AU_HD is `__host__ __device__` there and nothing elsewhere);
// nothing here names a kernel, LDS or a block index.  The library is built with -ffp-contract=off, / and sqrt are IEEE on both
// sides: the same bytes from both.
//
// The entry search.  The rule is "the FIRST stored entry q with t_start[q] <= t <= t_end[q]".  On a queue as the foot-constraints
// calls write it -- t_end non-decreasing, t_start[q] <= t_end[q] <= t_start[q + 1] -- that entry is the first q with
// t_end[q] >= t (every earlier entry ends before t), provided t_start[q] <= t (if not, every later entry starts behind t too).
// That lower bound is a function of the queue and t alone, so it does not matter where a walk over the samples starts or how it
// is cut: au_seek keeps the bound of the previous sample and steps forward from it, and bisects when the time went backwards.
// On a queue that is not ordered like that the entry found is unspecified (never out of range).
#pragma once
#include <cmath>

#include "../../include/wg_mpc.h"
#ifdef __HIP__
#define WG_AU_HD __host__ __device__
#else
#define WG_AU_HD
#endif
#define WG_AU_INLINE WG_AU_HD inline __attribute__((always_inline))

namespace wg {

constexpr double kAuInf = __builtin_huge_val();
constexpr double kAuSlack = -1e-8;       // a row value below it is a violation (:322)

WG_AU_INLINE bool au_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// a gait (or a chunk of one) none of whose samples was audited
WG_AU_INLINE wg_zmp_audit_t au_empty() { return wg_zmp_audit_t{kAuInf, -1, -1, 0, 0, 0, WG_OK}; }

// what has been audited later (samples or chunks in ascending order) into what was audited before: the least margin, and on a
// tie the earlier sample keeps it; the counts add
WG_AU_INLINE void au_fold(wg_zmp_audit_t &A, const wg_zmp_audit_t &P) {
  if (P.margin < A.margin) {
    A.margin = P.margin;
    A.worst_sample = P.worst_sample;
    A.worst_row = P.worst_row;
  }
  A.n_violated += P.n_violated;
  A.n_uncovered += P.n_uncovered;
  A.n_nonfinite += P.n_nonfinite;
}

// the first q of te[0 .. K) with te[q] >= t, or K (a NaN t: K)
WG_AU_INLINE int au_lower_bound(const double *te, int K, double t) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (te[mid] >= t) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// where a walk over the samples stands in its gait's queue: q is the lower bound of the last time sought, with the three
// numbers that decide whether it still is the next one's
struct AuCursor {
  int q;
  double te_prev, te_cur, ts_cur;        // t_end[q - 1] (-inf at q = 0), t_end[q] and t_start[q] (+inf at q = K)
};
WG_AU_INLINE void au_place(const double *ts, const double *te, int K, int q, AuCursor &c) {
  c.q = q;
  c.te_prev = q > 0 ? te[q - 1] : -kAuInf;
  c.te_cur = q < K ? te[q] : kAuInf;
  c.ts_cur = q < K ? ts[q] : kAuInf;
}
// moves c to the lower bound of t; true when that entry holds t
WG_AU_INLINE bool au_seek(const double *ts, const double *te, int K, double t, AuCursor &c) {
  if (!(t > c.te_prev && t <= c.te_cur)) {
    int q;
    if (t > c.te_cur) {
      q = c.q + 1;                                        // c.q < K here: te_cur is +inf at K
      while (q < K && te[q] < t) q++;
    } else {
      q = au_lower_bound(te, K, t);
    }
    au_place(ts, te, K, q, c);
  }
  return c.q < K && c.ts_cur <= t && t <= c.te_cur;
}

// the rows of one entry as a walk keeps them; nrows = 0 stands for an entry whose nrows is outside 1 .. WG_POLY_MAX_ROWS
struct AuRows {
  int nrows;
  double a0[WG_POLY_MAX_ROWS], a1[WG_POLY_MAX_ROWS], b[WG_POLY_MAX_ROWS], norm[WG_POLY_MAX_ROWS];
};
WG_AU_INLINE void au_load(const wg_zmp_polytope_t *p, AuRows &R) {
  const int n = p->nrows;
  R.nrows = n >= 1 && n <= WG_POLY_MAX_ROWS ? n : 0;
#pragma unroll
  for (int j = 0; j < WG_POLY_MAX_ROWS; j++) {
    R.a0[j] = p->A[j][0];
    R.a1[j] = p->A[j][1];
    R.b[j] = p->B[j];
    R.norm[j] = sqrt(R.a0[j] * R.a0[j] + R.a1[j] * R.a1[j]);
  }
}

// sample k at (x, y): its margin (returned), folded into A.  covered: an entry holds the sample's time and R is that entry.
WG_AU_INLINE double au_sample(const AuRows &R, bool covered, double x, double y, int k, wg_zmp_audit_t &A) {
  const bool nonfinite = !(au_finite(x) && au_finite(y));
  const bool uncovered = !covered || R.nrows == 0;
  bool violated = nonfinite || uncovered;
  double m = -kAuInf;
  int row = -1;
  if (!violated) {
#pragma unroll
    for (int j = 0; j < WG_POLY_MAX_ROWS; j++) {
      if (j < R.nrows) {
        const double v = (R.a0[j] * x + R.a1[j] * y) + R.b[j];
        double d = v / R.norm[j];
        if (!au_finite(d)) d = -kAuInf;
        if (j == 0 || d < m) {
          m = d;
          row = j;
        }
        if (v < kAuSlack) violated = true;
      }
    }
  }
  wg_zmp_audit_t P{m, k, row, violated ? 1 : 0, uncovered ? 1 : 0, nonfinite ? 1 : 0, WG_OK};
  au_fold(A, P);
  return m;
}

}  // namespace wg
