// wg_ql_guard.hpp -- certificates for the decision-only sums of ql0002's active-set iteration: when a sum formed in
// ANOTHER order than the reference's may decide a branch for it.  One text for host and device: plain C++ without a header of its
// own but <cmath>; the host tests compile it with g++ (tests/test_guarded_sums_host.py), the solver includes it with WG_GUARD_FN and
// WG_GUARD_K set for the device (wg_ql_device.hpp).
//
// The sums.  Two places of an iteration form a sum whose VALUE is never used, only compared:
//   * the linear-dependence test, qld.cpp:1491-1532:  suma = sum w_i z_i,  sumb = sum |w_i z_i|,  sumc = sum z_i^2  (i < n) feed
//         significant(sumb, |suma|),  sumb > vsmall,  significant(sqrt(sumc) [/ wa], |suma|)
//     and all three holding means "take a step" (route 0);
//   * lql's magnitude test, :2039-2058 and :1776-1786:  S = sum |x_i| vfact (|d_i| + |G_ii x_i|) feeds
//         xmag = max(xmag, S),  S < 0.01 xmag  ("reset").
// significant(base, delta) is  base + 0.1 delta > base  and  base + 0.2 delta > base + 0.1 delta  in doubles.
//
// The bound.  n <= 36 terms t_i (the compact view; 64 would do), u = 2^-53, every order of addition starting from 0.0.  A sum of
// k <= 36 additions carries a relative error of at most gamma_36 = 36 u / (1 - 36 u) in every partial sum (additions have no
// underflow error), so two orders of the same terms differ by at most 2 gamma_36 sum |t_i| < 2^-46 sum |t_i|  (72 u = 2^-46.83).
// The slack between 2^-46.83 and 2^-46 absorbs the roundings of the certificates' own arithmetic and the difference between
// sum |t_i| and either computed sumb.  For sumb, sumc and S the terms are >= 0: the bound is RELATIVE,
//       exact-order value  in  tree value x (1 +- 2^-46);
// for suma it is ABSOLUTE:  | suma - suma' | <= 2^-46 sumb'.   (primes: the sums in the other order)
// The same holds for xmag' = max of the S' since the last reset against xmag = max of the S: max is monotone.
//
// Why 2^-40.  significant(base, delta) certainly holds when base >= 0 is an ordinary number and delta >= 2^-40 base: then
// fl(0.1 delta) >= 2^-43.4 base >= 2^8.6 ulp(base), so temp = base + 0.1 delta lies hundreds of ulps above base, and the step from
// temp to tempa = base + 0.2 delta is another 0.1 delta >= 2^8 ulp(temp).  The certificates ask for delta' - 2^-46 sumb' >=
// 2^-40 (1 + 2^-40) base': the factor (1 + 2^-40) covers base <= base' (1 + 2^-45) (sumc's relative bound through sqrt and the
// division by the same wa) and the handful of roundings in forming both sides.  Likewise S' >= 0.01 xmag' (1 + 2^-40) implies
// S >= S' (1 - 2^-46) > fl(0.01 xmag) for every xmag within 2^-46 of xmag', and S' <= 0.01 xmag' (1 - 2^-40) implies S < fl(0.01 xmag).
// The second base, c = sqrt(sumc) / wa, is never formed: with d = |suma'| - 2^-46 sumb' >= 0, wa > 0 and k = 2^-40 (1 + 2^-40),
// d >= k c is (d wa)^2 >= k^2 sumc' -- three multiplications instead of a square root and a division on the iteration's path.  The
// roundings of both sides (four, 2^-51 in all on the squares) disappear in k's margin; d wa must be at least 2^-400, so that its
// square does not underflow (a right-hand side that underflows is below every such square: the inequality then holds in exact
// arithmetic too); a product or a square that overflows to infinity is in truth above k^2 sumc' < 2^421.
// No overflow: every value must lie below 2^500, so neither the other order's partial sums (<= sumb' (1 + 2^-46)) nor
// base + 0.2 delta reach infinity (c <= d / k < 2^541).  A NaN fails every comparison below, which are all written so that failing
// means doubt.
//
// What is certified -- and nothing else: "route 0" at the dependence test; "no reset" and "reset" at the magnitude test.  Every
// other outcome (a dependent normal, the coordinate check, NaN or infinite sums, zero sums, values beyond 2^500, a margin inside
// the bands) is DOUBT: the caller forms the sums in the reference's order and lets the reference's own tests decide.
// Tighten or loosen a constant only together with this argument (tests/test_guarded_sums_host.py holds the certificates to the
// reference's tests over adversarial inputs, in four orders of addition).
#pragma once
#include <cmath>

#ifndef WG_GUARD_FN
#define WG_GUARD_FN inline
#endif
#ifndef WG_GUARD_K
#define WG_GUARD_K(c) (c)          // the device materialises double constants where they are used (wg_kconst)
#endif

namespace wg {

enum GuardVerdict : int { kGuardDoubt = -1, kGuardNoReset = 0, kGuardReset = 1 };

// true: the reference's three tests on the index-order sums certainly send this iteration to route 0 (take a step).
// suma, sumb, sumc: the sums in any order; by_wa / wa: the normal is a general row and its reciprocal length as the scan read it
// (qld.cpp divides sqrt(sumc) by it); vsmall: the solver's eps.
WG_GUARD_FN bool guard_route0(double suma, double sumb, double sumc, bool by_wa, double wa, double vsmall) {
  const double big = WG_GUARD_K(0x1p500);
  const double as = std::fabs(suma);
  if (!(as < big) || !(sumb < big) || !(sumc < big)) return false;                   // NaN, infinity, beyond 2^500
  if (!(sumb * WG_GUARD_K(1.0 - 0x1p-46) > vsmall)) return false;                      // sumb > vsmall in the other order too
  const double d = as - WG_GUARD_K(0x1p-46) * sumb;                                    // a lower bound of |suma| in any order
  if (!(d >= WG_GUARD_K(0x1p-40 * (1.0 + 0x1p-40)) * sumb)) return false;              // against the first base, sumb
  // against the second base, c = sqrt(sumc) / wa, without the square root and the division:  d >= k c  <=>  (d wa)^2 >= k^2 sumc
  double p = d;
  if (by_wa) {
    if (!(wa > 0.0)) return false;
    p = d * wa;
  }
  if (!(p >= WG_GUARD_K(0x1p-400))) return false;                                      // p * p does not underflow
  return p * p >= WG_GUARD_K(0x1p-80 * (1.0 + 0x1p-39 + 0x1p-52)) * sumc;              // the constant: k^2 rounded up
}

// s: the magnitude sum in any order; xmag: the running maximum of such sums since the last reset, s included.
WG_GUARD_FN int guard_xmag(double s, double xmag) {
  const double big = WG_GUARD_K(0x1p500);
  if (!(s > 0.0) || !(s < big) || !(xmag < big)) return kGuardDoubt;                   // zero sums, NaN, infinity
  const double t = WG_GUARD_K(.01) * xmag;
  if (s >= t * WG_GUARD_K(1.0 + 0x1p-40)) return kGuardNoReset;
  if (s <= t * WG_GUARD_K(1.0 - 0x1p-40)) return kGuardReset;
  return kGuardDoubt;
}

// the running maximum may be taken over sums in another order while they are ordinary numbers (max is monotone and f2c's
// max(a, b) = a >= b ? a : b treats a NaN by position): false means doubt
WG_GUARD_FN bool guard_xmag_update(double s) { return s < WG_GUARD_K(0x1p500); }

// The orders the device adds in; the host tests form their "device order" sums with these two functions.
// The magnitude sum (wave_sum_tree, wg_wave.hpp): lane i holds term i (zero from n on), 64 lanes, a balanced binary tree: pairs
// of neighbours, pairs of pairs ...
inline double guard_tree_sum(const double *t, int n) {
  double v[64];
  for (int i = 0; i < 64; ++i) v[i] = i < n ? t[i] : 0.0;
  for (int w = 1; w < 64; w *= 2)
    for (int i = 0; i < 64; i += 2 * w) v[i] = v[i + w] + v[i];
  return v[0];
}
// The three sums of the dependence test (ql_solve, n <= 48): each in a row of 16 lanes, lane j starts from
// (t_j + t_{j+16}) + t_{j+32} (zeros from n on), then the balanced tree over the row.
inline double guard_rows_sum(const double *t, int n) {
  double v[16];
  for (int j = 0; j < 16; ++j) v[j] = ((j < n ? t[j] : 0.0) + (j + 16 < n ? t[j + 16] : 0.0)) + (j + 32 < n ? t[j + 32] : 0.0);
  for (int w = 1; w < 16; w *= 2)
    for (int i = 0; i < 16; i += 2 * w) v[i] = v[i + w] + v[i];
  return v[0];
}

}  // namespace wg
