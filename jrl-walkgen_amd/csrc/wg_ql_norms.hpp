// wg_ql_norms.hpp -- the chain of rotation norms of a Givens sweep (qld.cpp:1992-2030; sweep_flat's phase 1) from seeds made
// ahead of it, lane-parallel, and checked once.  One text for host and device: plain C++ without a header of its own
// but <cmath>; the host test compiles it with g++ (tests/test_seeded_norms_host.py), the solver includes it with WG_NORMS_FN,
// WG_NORMS_RSQ and WG_NORMS_EXACT set for the device (wg_ql_phases.hpp).  Compile with -ffp-contract=off: every operation below is
// the one written.
//
// The chain.  A sweep over s[lo .. hi) runs rotations c = hi-1, hi-2, .. lo+1.  Rotation c takes p = s[c-1] and cur (s[hi-1] for the
// first one, the previous rotation's result afterwards) to
//       cur' = t * sqrt(1 + (a / t)^2),     t = max(|p|, |cur|),  a = min(|p|, |cur|),
// with the reference's correctly rounded division and square root.  The exact form on the device (givens_norm_fast) spends about
// 23 dependent instructions on it, most of them refining 1/t and 1/sqrt(x), x = 1 + (a/t)^2, from the hardware's seeds.
//
// The seeds.  Entering rotation c, cur is the norm of s[c .. hi) up to a few ulps of accumulated rounding.  So before the chain
// starts every rotation can know t and x to about 1e-15:  with S_c = sum of s[j]^2 over c <= j < hi (a scan over the lanes, any
// order of addition: at most 36 terms, all >= 0) and P = s[c-1]^2,
//       T = max(P, S_c),  A = min(P, S_c),      r = 1/sqrt(T)  ~  1/t,       X = 1 + A r^2  ~  x,       y = 1/sqrt(X).
// The seeds work on SQUARES: no square root is needed for t, and the order of P and S_c may differ from that of |p| and |cur| only
// where the two are equal to 1e-15, where either choice is as good a seed.  Both reciprocal square roots start from the
// hardware's estimate (WG_NORMS_RSQ) and take TWO coupled Newton steps (an error e becomes 1.5 e^2): any estimate good to 2^-13
// ends below 2^-50, and then the roundings of the steps themselves decide -- r and y are good to about 4e-16, t and x as predicted
// to about 1e-15.  One step would do for an estimate good to 2^-26; the steps are lane-parallel, once per sweep, and the second
// costs four instructions, so the header does not lean on the estimate's accuracy.  (The host's stand-in, 1.0 / std::sqrt(x), is
// good to 1 ulp before the steps and stays there.)
//
// The step on the chain (norms_step), 11 dependent instructions with max and min, none of them transcendental:
//       q0 = a r;   rem = fma(-t, q0, a);   d = fma(rem, r, q0)                    the quotient a / t
//       x = 1 + d d
//       g0 = x y;   e = fma(-g0, g0, x);    g = fma(e, y / 2, g0)                  the root of x       (y / 2 off the chain)
//       cur' = t g
// One residual correction takes a quotient or a root that is good to 1e-13 to within 1e-26 (relative) of the true value before its
// last rounding, which therefore gives the correctly rounded one unless the true value lies that close to a rounding boundary.
// Measured on the host (tests/test_seeded_norms_host.py): no mismatch in 1 200 000 sweeps of six families with the seeds as made
// here, none with seeds perturbed by 1e-13, one or two at 1e-11, 4 % of the sweeps at 1e-9.
//
// No certificate: the check.  After the chain every rotation's operands are known exactly -- p = s[c-1], q = the value that entered
// (s[hi-1] or the recorded result of rotation c+1), and the recorded result.  Lane c recomputes ITS norm in the exact form from
// them and compares bit patterns (norms_rotation_ok); one ballot.  Induction over the chain: the first rotation's input is exact;
// if every rotation's recorded output equals the exact form applied to the input it actually had, then every input was the exact
// chain's, and so is every output.  On any mismatch -- whatever the seeds were: zero, infinite, NaN, stale -- phase 1 runs again in
// the exact form; it only writes the record, so the second run leaves nothing of the first behind.
//
// Zeros at the end of s.  While cur is zero the reference skips the rotation and hands p on: with s[h] the last non-zero entry
// (structural zeros of Z: three sweeps in ten of tests/test_seeded_norms_gpu.py's sample end in one), rotations c > h leave copies of s behind -- the caller
// writes them lane-parallel -- and the chain proper is the one above over s[lo .. h].  The check covers them by the same rule.
//
// Range.  The caller enters only when every entry of s[lo, hi) is zero or has its magnitude in [2^-400, 2^400] (sweep_range_ok),
// and runs the chain from the last non-zero entry, called s[hi-1] here.  Then squares lie in [2^-800, 2^800] or are zero, their sums below 2^806 and at least s[hi-1]^2 > 0: T is an
// ordinary number, r lies in [2^-403, 2^400], A r^2 <= 1 + 1e-15, X in [1, 2 + 1e-15].  cur never becomes zero (a norm is at least
// its larger operand), an exact-zero p gives q0 = rem = d = 0, x = 1, g = 1 and cur' = t; a quotient below 2^-27 may differ from
// the exact form's in its last bits and x = 1 + d d is 1 either way.
#pragma once
#include <cmath>

#ifndef WG_NORMS_FN
#define WG_NORMS_FN inline
#endif
#ifndef WG_NORMS_RSQ
#define WG_NORMS_RSQ(x) (1.0 / std::sqrt(x))        // the device: v_rsq_f64
#endif

namespace wg {

struct NormSeed { double r, y; };                   // r ~ 1 / t,  y ~ 1 / sqrt(x)

// 1 / sqrt(v) for an ordinary v > 0: the estimate and two coupled Newton steps
WG_NORMS_FN double norms_rsqrt(double v) {
  double y = WG_NORMS_RSQ(v);
  {
    const double g = v * y, h = 0.5 * y;
    const double e = __builtin_fma(-h, g, 0.5);
    y = __builtin_fma(y, e, y);
  }
  {
    const double g = v * y, h = 0.5 * y;
    const double e = __builtin_fma(-h, g, 0.5);
    y = __builtin_fma(y, e, y);
  }
  return y;
}

// the seeds of one rotation from p2 = s[c-1]^2 and s2 = the sum of the squares behind it (> 0)
WG_NORMS_FN NormSeed norms_seed(double p2, double s2) {
  const bool pbig = p2 >= s2;
  const double t2 = pbig ? p2 : s2, a2 = pbig ? s2 : p2;
  NormSeed o;
  o.r = norms_rsqrt(t2);
  const double x = 1.0 + a2 * (o.r * o.r);
  o.y = norms_rsqrt(x);
  return o;
}

// one rotation on the chain: t = max(|p|, |cur|) and a = min(|p|, |cur|) are the caller's (one instruction each on the device)
WG_NORMS_FN double norms_step(double t, double a, double r, double y) {
  const double q0 = a * r;
  const double rem = __builtin_fma(-t, q0, a);
  const double d = __builtin_fma(rem, r, q0);
  const double x = 1.0 + d * d;
  const double yh = 0.5 * y;
  const double g0 = x * y;
  const double e = __builtin_fma(-g0, g0, x);
  const double g = __builtin_fma(e, yh, g0);
  return t * g;
}

// the exact form: the reference's t * sqrt((p/t)^2 + (q/t)^2), of which one quotient is exactly +-1 (wg_ql_phases.hpp)
#ifndef WG_NORMS_EXACT
inline double norms_exact(double p, double q) {
  const double ap = std::fabs(p), aq = std::fabs(q);
  const double t = ap >= aq ? ap : aq, a = ap >= aq ? aq : ap;
  const double d = a / t;
  return t * std::sqrt(1.0 + d * d);
}
#define WG_NORMS_EXACT(p, q) ::wg::norms_exact(p, q)
#endif

WG_NORMS_FN bool norms_same_bits(double a, double b) {
  unsigned long long x, y;
  __builtin_memcpy(&x, &a, sizeof x);
  __builtin_memcpy(&y, &b, sizeof y);
  return x == y;
}
// the check of one rotation: (p, q) as they entered it, `recorded` as it left it.  A rotation whose q is zero is skipped by the
// reference and hands its p on (zeros at the end of s: the chain proper starts at the last non-zero entry)
WG_NORMS_FN bool norms_rotation_ok(double p, double q, double recorded) {
  const double want = (q == 0.0) ? p : WG_NORMS_EXACT(p, q);
  return norms_same_bits(want, recorded);
}

// The order the device scans in (wave_prefix_sum, wg_wave.hpp), for the host test: 64 lanes, inclusive prefix sums inside each row
// of 16 by doubling distances, then row 0's total into row 1 and row 2's into row 3, then the lower half's total into the upper.
inline void norms_prefix_scan(double *v /* 64 */) {
  for (int w = 1; w < 16; w *= 2)
    for (int i = 63; i >= 0; --i) if ((i & 15) >= w) v[i] = v[i] + v[i - w];
  for (int i = 16; i < 32; ++i) v[i] = v[i] + v[15];
  for (int i = 48; i < 64; ++i) v[i] = v[i] + v[47];
  for (int i = 32; i < 64; ++i) v[i] = v[i] + v[31];
}

}  // namespace wg
