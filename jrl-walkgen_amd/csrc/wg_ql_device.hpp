// wg_ql_device.hpp -- one dense convex QP per wavefront, all factors in LDS.
//
// Device-side replacement for the solver on the reference's Herdt-2010 path:
//   ql0001_ / ql0002_   src/Mathematics/qld.cpp:378-612, 621-2091
// (Powell / Schittkowski dual active-set method; called from
//  QPProblem::solve, src/ZMPRefTrajectoryGeneration/qp-problem.cpp:245-294.)
//
// The solver in five headers, included here in order (include this one):
//   wg_wave.hpp        the one-wave rules (no barrier, lanes over independent outputs only, sums in the reference's order)
//                      and the wave tools: WG_WSYNC, wg_lane, uni, rl, wg_kconst, the DPP reductions
//   wg_ql_view.hpp     QlDims, QlView and its layouts, the Z / G / A / R accessors, the dense problem policies, QlResult,
//                      QlResume, the WG_REP / WG_SINK macros of the attribution builds
//   wg_prof.hpp        (included by wg_ql_view.hpp) the profile build's g_prof slots by name and its timer marks: PT_* for the
//                      solver, TK_* for the tick, PT_LOCAL_* for a phase that times itself; nothing without WG_PROFILE
//   wg_ql_phases.hpp   the phases of one active-set iteration (products with Z, back substitution, sweeps, scans, deletion)
//   wg_ql_guard.hpp    the certificates of the compact view's decision-only sums, one text for host and device
//   this file          the dispatch of the back substitution and the sweep by problem view, and ql_solve itself (ISA-sensitive: compare
//                      every kernel before moving one of its blocks)
// Compile with -ffp-contract=off: the reference build has no FMA contraction.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wg_wave.hpp"
#include "wg_ql_view.hpp"
#include "wg_ql_phases.hpp"
// the certificates of the guarded sums, the host's text compiled for the device: constants materialised where they are used
#define WG_GUARD_FN __device__ __forceinline__
#define WG_GUARD_K(c) ::wg::wg_kconst(c)
#include "wg_ql_guard.hpp"

namespace wg {

// The solver.  Problem data must already be in LDS: G (copy of C, patched per
// qld.cpp:442-444), A, d, b (INNER sign: b = -b_user, qld.cpp:469-475), xl, xu.
// hist: optional global add(+code)/drop(-code) log written by lane 0.
// compact view (n <= 36): the LDS-pipelined form with two 48-entry buffers, its bottom rows at their own lengths; other views whose four scratch vectors hold two
// 96-entry buffers (n >= 48) take it too while every multiplier has a lane of its own (nact <= 60), the generic forms otherwise
#define WG_BACKSUB(q, s, nact, lane)                                                                   \
  do {                                                                                                 \
    if constexpr (P::kNM > 0 && P::kNM + 12 <= 48) backsub_lds<48, ExactBacksubOf<P>::value>(q, s, nact, lane, q.sc0); \
    else if (P::kNM == 0 && (P::kWideN || q.n >= 48) && (nact) <= 60) backsub_lds<96>(q, s, nact, lane, q.sc0);     \
    else if (P::kNM == 0 && !P::kRowOps && q.n >= 24 && (nact) <= 36) backsub_lds<48>(q, s, nact, lane, q.sc0); \
    else backsub(q, s, nact, lane);                                                                    \
  } while (0)
// one row of Z per lane (n <= 64): the branch-free, prefetching form -- the compact view always, the dense view by size (the
// element view is built for n > 64: it keeps the one form it needs, its kernel is large enough as it is)
#define WG_SWEEP(q, s, nu, nact, lane) \
  do { if (P::kNM > 0 || (!P::kRowOps && q.n <= 64)) sweep_flat<P::kFixedLdz, SeededNormsOf<P>::value>(q, s, nu, nact, lane, nmode PT_SW_ARG); else sweep<(P::kRowOps ? WG_ELEM_GRP : 8), P::kWideN>(q, s, nu, nact, lane); } while (0)

// the reference's tests of one candidate row k in its order, :1256-1282 (cvmax starts at 0); reads wak, sum, temp of the scan body
// it sits in and skips to its next row with `continue`.  A macro: as a function it changed the tick kernels' code
#define QL_SCAN_ACCEPT                                                                        \
  if (wak <= 0.0) continue;                                                                   \
  double sumx = -sum * wak;                                                                   \
  if (k + 1 <= me) sumx = fabs(sumx);                                                         \
  if (sumx <= 0.0) continue;                                                                  \
  if (bidx >= 0 && sumx <= bestv) continue;                                                   \
  double tempa = temp + fabs(sum);                                                            \
  if (tempa <= temp) continue;                                                                \
  temp += onha * fabs(sum);                                                                   \
  if (temp <= tempa) continue;                                                                \
  bestv = sumx; bestres = sum; bestw = wak; bidx = k + 1
template <class P>
__device__ __forceinline__ QlResult ql_solve(const QlView &q, P &prob, double vsmall, int *hist, int hist_cap, QlResume *rs = nullptr) {
  // NaN iterates followed exactly (every policy of the shipped kernels; a policy may opt out for an A/B of what that costs)
  constexpr bool kNan = P::kNanExact && (WG_NAN_REGIME != 0);
  // Guarded sums (the compact view; wg_ql_guard.hpp): the sums that only decide a branch -- the three of the
  // linear-dependence test, lql's magnitude sum -- are added as a tree over the lanes while a certificate can vouch for the
  // decision.  A doubt at the dependence test forms that iteration's sums in the reference's order on the spot (the test keeps no
  // state); a doubt at the magnitude test cannot be settled there (the exact running maximum is not known), so the solve leaves
  // with kQlDoubt -- a code no caller of the tick ever sees -- and ql_solve_guarded starts it again from its set-up with every sum
  // in the reference's order (sums_mode = kSumsOrdered: one mode word, wave-uniform).
  // kSumsDoubt (tests): the dependence certificate always doubts, and the finished solve is doubted as a whole -- the second pass
  // starts from the dirtiest state a first pass can leave.
  constexpr bool kGuard = GuardedSumsOf<P>::value;
  [[maybe_unused]] int gmode = kSumsOrdered;
  if constexpr (kGuard) gmode = uni(prob.sums_mode) & kSumsMask;
  // the sweep's norm chain (the compact view; wg_ql_norms.hpp): seeded and checked, exact throughout, or doubted in every sweep
  [[maybe_unused]] int nmode = kNormsExact;
  if constexpr (SeededNormsOf<P>::value) nmode = uni(prob.sums_mode) & kNormsMask;
  int lane = wg_lane();
  const int n = q.n, m = q.m, me = q.me, mn = q.mn;
  QlResult out;
  out.hist_len = 0;
  const bool resuming = rs != nullptr && rs->valid != 0;     // wave-uniform; a compile-time constant where rs is
  int nact = 0, info = 0, iterc = 1, itref = 0, iflag = 0;
  const int maxit = (m + n) * 40;                       // :459
  const double onha = 1.5, xmagr = .01, diagr = 2.0;
  const int ifinc = 3, kfinc = n > 10 ? n : 10;
  int jfinc = -kfinc;
  double xmag = 0.0, vfact = 1.0, res = 0.0, ratio = 0.0, diag = 0.0;
  double wsel = 1.0;                                        // wa[.] of the constraint knext, as the scan read it (positive)
  int knext = 0;
  const int s_tail = q.r_tail;                              // n (n + 1) / 2, or the working column of the last allowed nact
  double *s = q.R + s_tail;
  bool early_exit = false;
  bool cap_hit = false;
  // Has the iterate left the ordinary numbers (wave-uniform, sticky)?  x only changes in the residual refresh (once or twice per
  // solve: tested there with one compare per lane) and by `x += step z` (tested on the scalar step: free).  From then on the
  // violation scan is scan_nan_exact's -- the reference's dense row sums and its treatment of NaN values, exact for any x
  bool x_suspect = false;
  auto x_has_non_numbers = [&]() {
    bool b = false;
    for (int i = lane; i < n; i += 64) { const bool bi = !wg_sane(q.x[i]); b = b || bi; }
    return __ballot(b) != 0ull;
  };
  PT_DECL
  if (resuming) {
    nact = rs->nact; info = rs->info; iterc = rs->iterc; itref = rs->itref; iflag = rs->iflag; jfinc = rs->jfinc; knext = rs->knext;
    out.hist_len = rs->hist_len;
    xmag = rs->xmag; vfact = rs->vfact; res = rs->res; ratio = rs->ratio; diag = rs->diag;
    if constexpr (kNan) x_suspect = x_has_non_numbers();
  }

#define LOG_EVENT(code)                                                   \
  do {                                                                    \
    if (lane == 0 && hist && out.hist_len < hist_cap) hist[out.hist_len] = (code); \
    out.hist_len++;                                                       \
  } while (0)
  // guarded sums only: leave with kQlDoubt, the caller (ql_solve_guarded) runs the solve again from its set-up with every sum in
  // the reference's order.  What this pass changed and the set-up does not rewrite is put back here: a shifted Hessian diagonal (wd
  // still holds the caller's); wa, R, Z, the iterate, the multipliers and the history are rewritten from their first entry on
#define QL_RERUN_ORDERED                                                              \
  do {                                                                                \
    PT_COUNT2(PS_N_RERUN);                                                            \
    for (int i = lane; i < n; i += 64) prob.setGd(q, i, q.wd[i]);                     \
    WG_WSYNC();                                                                       \
    PT_FLUSH;                                                                         \
    out.ifail = kQlDoubt; out.n_iter = iterc; out.nact = nact;                        \
    return out;                                                                       \
  } while (0)

  // ---- reciprocal lengths of the constraint normals, :769-807 ----
  if (!resuming) {
    int fatal = 0x7fffffff;
    if constexpr (P::kCompact) {
      fatal = prob.norms(q, lane);
    } else {
      for (int k = lane; k < m; k += 64) {
        double sum = 0.0;
        if constexpr (P::kRowOps) sum = prob.row_sqnorm(q, k);
        else {
          WG_UNROLL
          for (int i = 0; i < n; ++i) { double a = Am(k, i); sum += a * a; }
        }
        if (sum > 0.0) sum = 1.0 / sqrt(sum);
        else if (q.b[k] == 0.0) {}
        else if (k + 1 <= me || !(q.b[k] <= 0.0)) fatal = k + 1 < fatal ? k + 1 : fatal;   // :789, a NaN fails
        q.wa[k] = sum;
      }
    }
    for (int k = lane; k < n; k += 64) q.wa[m + k] = 1.0;
    fatal = uni(wave_min_int(fatal));
    if (fatal != 0x7fffffff) { info = -fatal; early_exit = true; }
  }
  PT(PS_NORMS);

  if (!early_exit && !resuming) {
    // ---- make the Hessian numerically positive definite, :814-854 ----
    for (int i = lane; i < n; i += 64) q.wd[i] = prob.Gd(q, i);
    WG_WSYNC();
    if constexpr (P::kCompact) {
      diag = prob.diag_check(q, vsmall, lane);
    } else {
      double dl = 0.0;
      for (int i = lane; i < n; i += 64) {
        double wdi = q.wd[i];
        dl = maxd(dl, vsmall - wdi);
        WG_UNROLL
        for (int j = i + 1; j < n; ++j) {
          double gjj = q.wd[j], gij = Gm(i, j);
          double ga = -mind(wdi, gjj);
          double gb = fabs(wdi - gjj) + fabs(gij);
          if (gb > 0.0) ga += gij * gij / gb;
          dl = maxd(dl, ga);
        }
      }
      diag = wave_max(dl);
    }
    diag = uni(diag);
    bool need_shift = !(diag <= 0.0);                       // :844 `if (diag <= 0) goto L90`: a NaN shifts
    PT(PS_DIAGCHK);
    bool factored = false;
    if constexpr (P::kHasFactor) {
      WG_REP(8)
      if (!need_shift && prob.blocks_ok) factored = WG_UBOOL(prob.factor(q, vsmall, lane));
    }
    if constexpr (P::kNM > 0 && P::kNM <= 64 && !P::kHasFactor) {
      // compile-time-bounded views without a structured factor of their own (the dense boundary at a known size, the Dimitrov
      // tick's QL back-end): R and Z through registers.  The compact view keeps the generic loops for the rare tick whose blocks
      // do not apply: unrolled into the tick kernels this body doubled their spilled SGPRs (260 -> 552) for a path they almost never take
      if (!factored && !need_shift) factored = chol_inverse_regs<P::kNM>(q, prob, vsmall, lane);
    }
    if (!factored) {
    for (;;) {
      if (need_shift) {
        diag = diagr * diag;
        for (int i = lane; i < n; i += 64) prob.setGd(q, i, diag + q.wd[i]);
        WG_WSYNC();
      }
      // ---- Cholesky, row by row (same sums as the column order of :859-890) ----
      int jfail = -1;
      double tfail = 0.0;
      for (int i = 0; i < n; ++i) {
        for (int j = i + lane; j < n; j += 64) {
          double temp = Gm(i, j);
          WG_UNROLL
          for (int k = 0; k < i; ++k) temp -= Rf(k, j) * Rf(k, i);
          if (j == i) {
            if (temp < vsmall) { q.slot[0] = 1.0; q.slot[1] = temp; }
            else { q.slot[0] = 0.0; Rf(i, i) = sqrt(temp); }
          } else q.sc0[j] = temp;
        }
        WG_WSYNC();
        if (WG_UBOOL(q.slot[0] != 0.0)) { jfail = i; tfail = q.slot[1]; break; }
        double rii = Rf(i, i);
        for (int j = i + 1 + lane; j < n; j += 64) Rf(i, j) = q.sc0[j] / rii;
        WG_WSYNC();
      }
      jfail = uni(jfail);
      if (jfail < 0) break;
      // ---- :895-918 further diagonal shift (rare; lane 0, serial) ----
      if (lane == 0) {
        double dnew;
        if (jfail == 0) dnew = diag + vsmall - tfail;
        else {
          double *v = q.lam;
          double sumx = 1.0;
          v[jfail] = 1.0;
          for (int k = jfail; k >= 1; --k) {
            double sum = 0.0;
            WG_UNROLL
            for (int i = k; i <= jfail; ++i) sum -= Rf(k - 1, i) * v[i];
            v[k - 1] = sum / Rf(k - 1, k - 1);
            sumx += v[k - 1] * v[k - 1];
          }
          dnew = diag + vsmall - tfail / sumx;
        }
        q.slot[2] = dnew;
      }
      WG_WSYNC();
      diag = uni(q.slot[2]);
      need_shift = true;
    }

    PT(PS_CHOL);
    // ---- Z = R^-1, :937-975 ----
    for (int i = lane; i < n; i += 64) {
      WG_UNROLL
      for (int j = 0; j < i; ++j) Zm(i, j) = 0.0;
      Zm(i, i) = 1.0 / Rf(i, i);
    }
    {
      // aligned form: all lanes walk (c, k) together so R(k,c) is a broadcast
      const int i0 = lane, i1 = lane + 64;
      double sum0, sum1;
      for (int c = 1; c < n; ++c) {
        sum0 = 0.0; sum1 = 0.0;
        WG_UNROLL
        for (int k = 0; k < c; ++k) {
          double rkc = Rf(k, c);
          if (i0 <= k) sum0 += Zm(i0, k) * rkc;
          if (i1 <= k) sum1 += Zm(i1, k) * rkc;
        }
        double rcc = Rf(c, c);
        if (i0 < c) Zm(i0, c) = -sum0 / rcc;
        if (i1 < c) Zm(i1, c) = -sum1 / rcc;
      }
    }
    WG_WSYNC();
    }   // !factored
  }

  PT(PS_INVERSE);
  // register rows of A (DenseRegProb) are loaded here, after the factorisation has given its registers back
  if constexpr (HasRegRows<P>::value) { if (!early_exit && !resuming) prob.load_rows(q, lane); }
  enum { ST_RESET, ST_RESID, ST_SCAN, ST_CONVERGED, ST_FINISH };
  int st = early_exit ? ST_FINISH : ST_RESET;
  if (resuming) st = rs->st;
  while (st != ST_FINISH) {
    // the lane index is made opaque once per iteration: otherwise everything derived from it alone (clamped indices, LDS
    // addresses of the lane's entries) is computed in front of the loop and kept alive -- in the 256-register kernel: spilled
    // there and reloaded from scratch memory in every iteration
    asm volatile("" : "+v"(lane));
    if (st == ST_RESET || st == ST_RESID) {
      s = q.R + s_tail;
      if (st == ST_RESET) {                                 // :989-1027
        iflag = 1;
        for (int i = lane; i < n; i += 64) {
          q.x[i] = 0.0;
          q.ww[i] = q.d[i];
          if (i >= nact) continue;
          q.lam[i] = 0.0;
          int k = q.iact[i];
          if (k <= m) s[i] = q.b[k - 1];
          else if (k > mn) s[i] = -prob.xu(q, k - mn - 1);
          else s[i] = prob.xl(q, k - m - 1);
        }
        xmag = 0.0;
        vfact = 1.0;
        WG_WSYNC();
        PT(PS_RESET_BODY);
      } else {                                              // :1031-1099
        iflag = 2;
        WG_REP(11) {                                        // gradient and residuals of the refresh: reads x, lam; writes ww, s
        typename ActiveParamsOf<P>::type ap;
        if constexpr (P::kCompact) ap = prob.active_params(q, nact, lane);
        for (int i = lane; i < n; i += 64) {
          double acc = q.d[i];
          if constexpr (P::kCompact) acc = prob.gdot_acc(q, i, q.x, acc);
          else {
            WG_UNROLL
            for (int j = 0; j < n; ++j) acc += Gm(i, j) * q.x[j];
          }
          PT_VIA(PS_RESID_GX, q.ww[i], acc);
          if constexpr (P::kCompact) acc = prob.grad_minus_active(q, ap, nact, i, acc);
          else {
            WG_UNROLL
            for (int k = 0; k < nact; ++k) {
              int kk = q.iact[k];
              if (kk <= m) acc -= q.lam[k] * Am(kk - 1, i);
              else if (kk <= mn) { if (kk - m - 1 == i) acc -= q.lam[k]; }
              else { if (kk - mn - 1 == i) acc += q.lam[k]; }
            }
          }
          q.ww[i] = acc;
        }
        if constexpr (P::kCompact) { prob.row_residuals(q, q.sc0, lane); WG_WSYNC(); }
        for (int k = lane; k < nact; k += 64) {
          int kk = q.iact[k];
          double sk;
          if (kk <= m) {
            if constexpr (P::kCompact) sk = q.sc0[kk - 1];
            else {
              sk = q.b[kk - 1];
              WG_UNROLL
              for (int i = 0; i < n; ++i) sk -= q.x[i] * Am(kk - 1, i);
            }
          } else if (kk <= mn) { int k1 = kk - m - 1; sk = prob.xl(q, k1) - q.x[k1]; }
          else { int k1 = kk - mn - 1; sk = -prob.xu(q, k1) + q.x[k1]; }
          s[k] = sk;
        }
        WG_WSYNC();
        }   // WG_REP(11)
        PT(PS_RESID_GRAD);
      }
      if (nact > 0) {                                       // :1104-1170
        // forward substitution with R^T, column oriented (sums ascend in j)
        {
          double sum0 = 0.0, sum1 = 0.0;
          const int i0 = lane, i1 = lane + 64;
          for (int j = 0; j < nact; ++j) {
            if (i0 == j) s[j] = (s[j] - sum0) / Rp(j, j);
            if (i1 == j) s[j] = (s[j] - sum1) / Rp(j, j);
            WG_WSYNC();
            double sj = s[j];
            if (i0 > j && i0 < nact) sum0 += Rp(j, i0) * sj;
            if (i1 > j && i1 < nact) sum1 += Rp(j, i1) * sj;
          }
        }
        PT(PS_RESID_FWD);
        if (P::kWideN || (P::kNM == 0 && n > 64 && n <= 128)) {
          double r0, r1;
          z_rows_times<(P::kRowOps ? WG_ELEM_GRP : 8)>(q, s, 0, nact, lane, r0, r1);
          q.x[lane] += r0; q.sc0[lane] = r0;
          if (lane + 64 < n) { q.x[lane + 64] += r1; q.sc0[lane + 64] = r1; }
        } else
        for (int i = lane; i < n; i += 64) {
          double sum = 0.0;
          WG_UNROLL
          for (int j = 0; j < nact; ++j) sum += s[j] * Zm(i, j);
          q.x[i] += sum;
          q.sc0[i] = sum;
        }
        WG_WSYNC();
        for (int j = lane; j < n; j += 64) {
          double acc = q.ww[j];
          if constexpr (P::kCompact) acc = prob.gdot_acc(q, j, q.sc0, acc);
          else {
            WG_UNROLL
            for (int i = 0; i < n; ++i) acc += q.sc0[i] * Gm(i, j);
          }
          q.ww[j] = acc;
        }
        WG_WSYNC();
      }
      PT(PS_RESID);
      zt_times_ww<P::kNM, (P::kRowOps ? WG_ELEM_GRP : 8), P::kWideN>(q, s, lane);                           // :1175-1177
      PT(PS_ZTWW_RESID);
      if (nact != n) {                                      // :1186-1201
        if (P::kWideN || (P::kNM == 0 && n > 64 && n <= 128)) {
          double r0, r1;
          z_rows_times<(P::kRowOps ? WG_ELEM_GRP : 8)>(q, s, nact, n, lane, r0, r1);
          q.x[lane] -= r0;
          if (lane + 64 < n) q.x[lane + 64] -= r1;
        } else
        for (int i = lane; i < n; i += 64) {
          double sum = 0.0;
          WG_UNROLL
          for (int j = nact; j < n; ++j) sum += Zm(i, j) * s[j];
          q.x[i] -= sum;
        }
        info = 0;
        WG_WSYNC();
      }
      PT(PS_XSHIFT);
      if (nact != 0) {                                      // :1208-1217
        WG_BACKSUB(q, s, nact, lane);
        for (int k = lane; k < nact; k += 64) q.lam[k] += q.ww[k];
        WG_WSYNC();
      }
      PT(PS_BACKSUB_RESID);
      if constexpr (kGuard) {
        // nothing is decided here: the running maximum follows the tree sums while they are ordinary numbers
        double sm = 0.0;
        WG_REP(6) { sm = uni(xmag_sum_guarded(q, prob, vfact, lane, gmode == kSumsOrdered)); WG_SINK(sm); }
        if (gmode != kSumsOrdered && WG_UBOOL(x_suspect || !guard_xmag_update(sm))) QL_RERUN_ORDERED;
        xmag = maxd(xmag, sm);
      } else
      { double sm = 0.0; WG_REP(6) { sm = uni(xmag_sum(q, prob, vfact, lane)); WG_SINK(sm); } xmag = maxd(xmag, sm); }
      PT(PS_XMAG_RESID);
      if (iflag == itref) { st = ST_RESID; continue; }      // :1226
      // first inequality with a negative multiplier, :1233-1249 (`if (w[kdrop] >= zero) goto next`: a NaN multiplier IS dropped)
      int kd = 0x7fffffff;
      for (int k = lane; k < nact; k += 64)
        if (!(q.lam[k] >= 0.0) && q.iact[k] > me) { kd = k < kd ? k : kd; }
      kd = uni(wave_min_int(kd));
      if (kd != 0x7fffffff) {
        LOG_EVENT(-q.iact[kd]);
        nact = drop_constraint(q, kd, nact, nact, lane);
        st = ST_RESID;
        continue;
      }
      if constexpr (kNan) x_suspect = x_suspect || x_has_non_numbers();       // the refresh rewrote x
      st = ST_SCAN;
    }

    if (st == ST_SCAN) {
      // the common path -- an add that neither resets nor refreshes is followed by the next scan -- closes here with ONE taken
      // branch, without passing the dispatch on `st` at the head of the loop (the lane index is made opaque again, as there)
      next_scan: asm volatile("" : "+v"(lane));
      // ---- most violated normalised constraint, :1255-1331 ----
      // bestw: the weight wa[.] of the lane's candidate as the scan read it.  The winner's is kept (wsel): the linear-dependence
      // test divides by it and the activation stores its negative -- wa may live in global memory (L2), where reading it again on
      // the critical path is an exposed round trip per iteration (the same value: nothing writes wa between the scan and the add)
      double bestv = 0.0, bestres = 0.0, bestw = 0.0;
      int bidx = -1;
      if (kNan && x_suspect) {                              // the iterate may hold a NaN / an infinity: the NaN-exact form decides
        if constexpr (kNan) {
          double cv = 0.0;
          int kn = knext;
          scan_nan_exact(q, prob, onha, cv, res, wsel, kn, lane);
          knext = uni(kn);
          bestv = uni(cv); bidx = -1;                       // res / knext / wsel are already what the reference leaves
        }
      } else
      WG_REP(1) {
      bestv = 0.0; bestres = 0.0; bestw = 0.0; bidx = -1;
      if constexpr (P::kCompact) {
        constexpr int NH = sizeof(prob.ax) / sizeof(double);
        double xs[2 * NH];
#pragma unroll
        for (int c = 0; c < 2 * NH; ++c) xs[c] = q.x[c];
        // the foot-placement row's operands are requested here as well: they arrive while the CoP row is summed
        const bool has_foot = lane < 5 * prob.ns;
        const int kf = has_foot ? 1 + 4 * NH + lane : 0;
        const double wakf = q.wa[kf], bkf = q.b[kf];
        // ... and so is every other operand of what follows the CoP row's jerk terms: its two step-column terms, the four terms of
        // the foot-placement row and the bound pair of variable `lane`.  Requested one by one where they are used, each was an
        // exposed round trip per iteration (six to LDS, and one to L2 for the bound's weight: wa lives in global memory here).
        // A CoP row of the current support phase (fj < 0) has no step-column entry: its lanes take x[0] with a zero coefficient
        // instead of branching around the two terms.  Their products are +-0.0 (x holds ordinary numbers on this path): a non-zero
        // sum and asum >= +0.0 are unchanged, and a zero sum of either sign gives sumx = -(+-0) wak, which is not > 0: no
        // candidate either way, and only a candidate's sum is ever used
        const bool has_step = prob.fj >= 0;
        const double xsa = q.x[has_step ? 2 * NH + prob.fj : 0], xsb = q.x[has_step ? 2 * NH + prob.ns + prob.fj : 0];
        const auto fr = prob.foot_row();
        double xfr[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) xfr[e] = q.x[fr.c[e]];
        const bool bin = lane < n;
        const int bkc = bin ? lane : n - 1;
        const double bw = q.wa[m + bkc], bxk = q.x[bkc];
        {
          const int k = lane + 1;                     // the lane's CoP row
          const double wak = q.wa[k], bk = prob.bcop;
          double sum = -bk, asum = fabs(bk);
          prob.cop_row_dot(xs, sum, asum);
          {
            const double ca = has_step ? prob.fa() : 0.0, cb = has_step ? prob.fb() : 0.0;
            double t = xsa * ca; sum += t; asum += fabs(t);
            t = xsb * cb; sum += t; asum += fabs(t);
          }
          const double sumx = -sum * wak;
          {                                           // the reference's tests in its order, as one predicate and three selects
            const double tempa = asum + fabs(sum);
            const double temp2 = asum + onha * fabs(sum);
            const bool take = (wak > 0.0) & !(sumx <= 0.0) & !(tempa <= asum) & !(temp2 <= tempa);
            bestv = take ? sumx : bestv; bestres = take ? sum : bestres; bestw = take ? wak : bestw; bidx = take ? k + 1 : bidx;
          }
        }
        {
          // the lane's foot-placement row; lanes without one walk the all-zero dummy row 0 (weight 0: never a candidate) on
          // valid columns with zero coefficients
          const int k = kf;
          const double wak = wakf, bk = bkf;
          double sum = -bk, asum = fabs(bk);
#pragma unroll
          for (int e = 0; e < 4; ++e) { const double t = xfr[e] * fr.v[e]; sum += t; asum += fabs(t); }
          const double sumx = -sum * wak;
          const double tempa = asum + fabs(sum);
          const double temp2 = asum + onha * fabs(sum);
          const bool take = has_foot & (wak > 0.0) & !(sumx <= 0.0) & !((bidx >= 0) & (sumx <= bestv)) & !(tempa <= asum) & !(temp2 <= tempa);
          bestv = take ? sumx : bestv; bestres = take ? sum : bestres; bestw = take ? wak : bestw; bidx = take ? k + 1 : bidx;
        }
        {
          // the bound pair of variable `lane` (the n <= 64 form below, on the operands requested above); the code of an upper bound
          // is the lower one's plus n: an addend chosen by a select, not two assignments under exec masks
          const double s1 = prob.xl(q, bkc) - bxk;
          const bool upper = s1 < 0.0;
          const double sum = upper ? bxk - prob.xu(q, bkc) : s1;
          const bool take = bin & !(bw <= 0.0) & !(s1 == 0.0) & !(sum <= 0.0) & !((bidx >= 0) & (sum <= bestv));
          bestv = take ? sum : bestv; bestres = take ? -sum : bestres; bestw = take ? bw : bestw;
          bidx = take ? bkc + 1 + m + (upper ? n : 0) : bidx;
        }
      } else {
      if constexpr (P::kRowOps) {
        // structured rows: every lane of a pass walks its row the same number of steps, both sums at once (row_dot_both);
        // the tests below are the reference's, in its order
        // wa, b and the row tables may live in global memory (L2): the operands of every pass are requested before the first
        // pass starts (m <= 1 + 64 kScanPasses rows, checked where the view is chosen)
        constexpr int kScanPasses = 3;
        double wak_p[kScanPasses], bk_p[kScanPasses], ra_p[kScanPasses], rb_p[kScanPasses];
        int rk_p[kScanPasses];
#pragma unroll
        for (int pp = 0; pp < kScanPasses; ++pp) {
          const int k = 1 + 64 * pp + lane;
          const bool in = k < m;
          const int kc = in ? k : 0;                          // surplus lanes walk the all-zero dummy row
          wak_p[pp] = in ? q.wa[kc] : 0.0; bk_p[pp] = q.b[kc];
          ra_p[pp] = prob.rowA[kc]; rb_p[pp] = prob.rowB[kc]; rk_p[pp] = prob.rowK[kc];
        }
#pragma unroll
        for (int pp = 0; pp < kScanPasses; ++pp) {            // row 0 is the all-zero dummy row: never a candidate, not walked
          const int k0 = 1 + 64 * pp;
          if (k0 >= m) break;
          const int k = k0 + lane;
          const int kc = k < m ? k : 0;
          const double wak = wak_p[pp], bk = bk_p[pp];
          double sum = -bk, temp = fabs(bk);
          prob.row_dot_both(q, kc, k0, ra_p[pp], rb_p[pp], rk_p[pp], q.x, sum, temp);
          QL_SCAN_ACCEPT;
        }
      } else if constexpr (HasRegRows<P>::value) {
        // dense rows in registers: no memory access but x (LDS broadcasts, eight at a time); both of the lane's rows (lane,
        // 64 + lane) are walked together, then the reference's tests in its order -- row lane first, row 64 + lane second
        constexpr int NMr = P::kNM;
        const int ka = lane, kb = lane + 64;
        const bool ina = ka < m, inb = kb < m;
        const int mc = m > 0 ? m - 1 : 0;      // m == 0: entry 0 of b exists (mmax >= 1), its value is masked below
        const int kca = ina ? ka : mc, kcb = inb ? kb : mc;
        const double waka = ina ? q.wa[kca] : 0.0, bka = q.b[kca], wakb = inb ? q.wa[kcb] : 0.0, bkb = q.b[kcb];
        double suma = -bka, tempa_ = fabs(bka), sumb = -bkb, tempb_ = fabs(bkb);
#pragma unroll
        for (int i0 = 0; i0 < NMr; i0 += 8) {
          double xs[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) xs[e] = q.x[(i0 + e < n) ? i0 + e : n - 1];
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (i0 + e < NMr && i0 + e < n) {
              const double ta = xs[e] * prob.ar0[i0 + e]; suma += ta; tempa_ += fabs(ta);
              const double tb = xs[e] * prob.ar1[i0 + e]; sumb += tb; tempb_ += fabs(tb);
            }
        }
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          const int k = pp == 0 ? ka : kb;
          const double wak = pp == 0 ? waka : wakb, sum = pp == 0 ? suma : sumb;
          double temp = pp == 0 ? tempa_ : tempb_;
          QL_SCAN_ACCEPT;
        }
      } else
      // dense rows: ONE walk of the row for both sums (sum += x_i a_ki, temp += |x_i a_ki|, i ascending: the same values the
      // serial code forms in two walks, the second only for candidates), the row's entries of eight columns requested while the
      // previous eight are added -- with A read in place (L2) the 4-at-a-time walk exposed a round trip every four terms.
      // Every lane of a pass walks (surplus lanes a valid row); the tests below are the reference's, in its order.
      for (int k0 = 0; k0 < m; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < m;
        const int kc = in ? k : m - 1;
        const double wak = in ? q.wa[kc] : 0.0, bk = q.b[kc];
        double sum = -bk, temp = fabs(bk);
        {
          constexpr int kG = 8;
          double ua[kG], ub[kG];
          auto fetch = [&](double (&u)[kG], int i) {
#pragma unroll
            for (int e = 0; e < kG; ++e) u[e] = Am(kc, i + e < n ? i + e : n - 1);   // past the end: clamped (loaded, unused)
          };
          auto add = [&](const double (&u)[kG], int i) {
            double xs[kG];
#pragma unroll
            for (int e = 0; e < kG; ++e) xs[e] = q.x[i + e];
#pragma unroll
            for (int e = 0; e < kG; ++e) { const double t = xs[e] * u[e]; sum += t; temp += fabs(t); }
          };
          int i = 0;
          const int whole = n / kG * kG;
          if (whole > 0) {
            fetch(ua, 0);
            for (;;) {
              fetch(ub, i + kG);
              add(ua, i); i += kG;
              if (i >= whole) break;
              fetch(ua, i + kG);
              add(ub, i); i += kG;
              if (i >= whole) { 
#pragma unroll
                for (int e = 0; e < kG; ++e) ub[e] = ua[e];
                break;
              }
            }
            // ub holds columns i .. i + kG - 1 (clamped): the odd ones
#pragma unroll
            for (int e = 0; e < kG - 1; ++e)
              if (i + e < n) { const double t = q.x[i + e] * ub[e]; sum += t; temp += fabs(t); }
          } else {
            for (; i < n; ++i) { const double t = q.x[i] * Am(kc, i); sum += t; temp += fabs(t); }
          }
        }
        QL_SCAN_ACCEPT;
      }
      }
      if constexpr (P::kCompact) {                           // done above, with the rows
      } else if constexpr (P::kNM > 0) {                     // n <= 64: one bound pair per lane, selects instead of continues
        const bool in = lane < n;
        const int kc = in ? lane : n - 1;
        const double w = q.wa[m + kc], xk = q.x[kc];
        const double s1 = prob.xl(q, kc) - xk;
        const bool upper = s1 < 0.0;
        const double sum = upper ? xk - prob.xu(q, kc) : s1;
        const bool take = in && !(w <= 0.0) && !(s1 == 0.0) && !(sum <= 0.0) && !(bidx >= 0 && sum <= bestv);
        bestv = take ? sum : bestv; bestres = take ? -sum : bestres; bestw = take ? w : bestw; bidx = take ? (upper ? kc + 1 + mn : kc + 1 + m) : bidx;
      } else
      for (int k = lane; k < n; k += 64) {
        const double w = q.wa[m + k];
        if (w <= 0.0) continue;
        bool lower = true;
        double sum = prob.xl(q, k) - q.x[k];
        if (sum == 0.0) continue;
        if (sum < 0.0) { sum = q.x[k] - prob.xu(q, k); lower = false; }
        if (sum <= 0.0) continue;               // cvmax starts at 0
        if (bidx >= 0 && sum <= bestv) continue;
        bestv = sum; bestres = -sum; bestw = w; bidx = lower ? k + 1 + m : k + 1 + mn;
      }
      {
        // order key: general rows 1..m, then bounds by variable; lower/upper of one
        // variable never compete.  knext codes > mn (upper) must sort by variable.
        int key = bidx < 0 ? -1 : (bidx > mn ? bidx - n : bidx);
        if constexpr (P::kCompact) {
          // the compact view's selection on the bit patterns of the (positive) candidate values: scan_select_lane
          const int src = scan_select_lane(bestv, key);
          if (src < 0) { bestv = 0.0; bidx = -1; }
          else {
            bestv = rl(bestv, src);
            bestres = rl(bestres, src);
            bestw = rl(bestw, src);
            bidx = __builtin_amdgcn_readlane(bidx, src);
          }
        } else {
        double v = bestv;
        int kk = key;
        wave_argmax_first(v, kk);
        kk = uni(kk);
        if (kk < 0) { bestv = 0.0; bidx = -1; }
        else {
          int src = -1;
          // the lane that owns the winning key
          unsigned long long mask = __ballot(key == kk);
          src = __ffsll((long long)mask) - 1;
          bestv = rl(bestv, src);
          bestres = rl(bestres, src);
          bestw = rl(bestw, src);
          bidx = __builtin_amdgcn_readlane(bidx, src);
        }
        }
      }
      WG_SINK(bestv); WG_SINK(bestres); WG_SINK(bestw); WG_SINK(bidx);
      }   // WG_REP(1)
      double cvmax = bestv;
      if (bidx >= 0) { res = bestres; knext = bidx; wsel = bestw; }
      PT(PS_SCAN);
      info = 0;
      if (WG_UBOOL(cvmax <= wg_kconst(vsmall))) { st = ST_CONVERGED; continue; }  // :1336

      // ---- has the objective stopped increasing?  :1343-1408 ----
      ++jfinc;
      if (jfinc == 0 || jfinc == ifinc) {
        if (jfinc == ifinc) {
          for (int i = lane; i < n; i += 64) {
            double sum = 2.0 * q.d[i];
            double sumx = fabs(sum);
            WG_UNROLL
            for (int j = 0; j < n; ++j) {
              double temp = Gm(i, j) * (q.wx[j] + q.x[j]);
              sum += temp;
              sumx += fabs(temp);
            }
            double dx = q.x[i] - q.wx[i];
            q.sc0[i] = sum * dx;
            q.sc1[i] = sumx * fabs(dx);
          }
          WG_WSYNC();
          double fdiff = 0.0, fdiffa = 0.0;
          WG_UNROLL
          for (int i = 0; i < n; ++i) { fdiff += q.sc0[i]; fdiffa += q.sc1[i]; }
          info = 2;
          double sum = fdiffa + fdiff;
          if (WG_UBOOL(sum <= fdiffa)) { st = ST_CONVERGED; continue; }
          double temp = fdiffa + onha * fdiff;
          if (WG_UBOOL(temp <= sum)) { st = ST_CONVERGED; continue; }
          jfinc = 0;
          info = 0;
        }
        for (int i = lane; i < n; i += 64) q.wx[i] = q.x[i];
        WG_WSYNC();
      }
      PT(PS_FDIFF);
      ++iterc;                                              // :1415-1420
      if (iterc > maxit) { info = 1; st = ST_FINISH; continue; }

      // ---- new normal and its products with the columns of Z, :1422-1470 ----
      s = q.R + nact * (nact + 1) / 2;
      WG_REP(2)
      if (knext <= m) {
        if constexpr (P::kCompact) prob.fill_row(q, knext - 1, q.ww, lane);
        else if constexpr (HasRegRows<P>::value) prob.row_to(q, knext - 1, q.ww, lane);
        else for (int i = lane; i < n; i += 64) q.ww[i] = Am(knext - 1, i);
        WG_WSYNC();
        if constexpr (P::kCompact) prob.zt_row(q, s, knext - 1, lane);
        else if constexpr (P::kWideN && P::kRowOps) {
          // the Herdt QP at a horizon known at compile time: a CoP row of instant r has no entry in rows (r, N) and (N + r, 2N)
          constexpr int kNHc = P::kHorizon;
          const int k = knext - 1;
          const bool cop = k >= 1 && k <= 4 * kNHc;
          const int rr = cop ? ((k - 1) >> 2) : -1;
          const int si = cop ? prob.stepidx[rr] : 1;         // the previewed step the instant belongs to (0: the current support phase)
          zt_times_ww_cop_tiled<kNHc>(q, s, lane, rr, !cop || (si >= 1 && si <= prob.ns));
        }
        else zt_times_ww<P::kNM, (P::kRowOps ? WG_ELEM_GRP : 8), P::kWideN>(q, s, lane);
      } else {
        int k1 = knext - m;
        double sg = 1.0;
        if (k1 > n) { k1 = knext - mn; sg = -1.0; }
        for (int i = lane; i < n; i += 64) {
          q.ww[i] = (i == k1 - 1) ? sg : 0.0;
          double z = Zm(k1 - 1, i);
          s[i] = (sg > 0.0) ? z : -z;
        }
        WG_WSYNC();
      }
      PT(PS_NEWNORMAL);
      double parnew = 0.0, parinc = 0.0, step = 0.0, sumy;
      int kdrop = -1;
      int route;   // 0 step, 1 dependent (multipliers needed), 2 dependent (multipliers in ww)
      if (nact == n) route = 1;                             // :1477
      else {
        WG_SWEEP(q, s, n, nact, lane);                         // :1480-1482
        PT(PS_SWEEP);
        if (nact == 0) route = 0;                           // :1488
        else {                                              // :1491-1532
          double suma = 0.0, sumb = 0.0, sumc = 0.0;
          bool step_certain = false;                         // guarded sums: the certificate has decided route 0
          WG_REP(5) {
          if constexpr (kGuard) {
            constexpr int NM = P::kNM;
            static_assert(NM > 32 && NM <= 48, "three entries per lane of a 16-lane row");
            {
              // the three product vectors, written as before (lanes past NM shadow lane NM - 1, entries from n on are zeros)
              const int il = lane < NM ? lane : NM - 1;
              const bool in = il < n;
              const int ic = in ? il : n - 1;
              const double zv = Zm(ic, nact), wv = q.ww[ic];
              const double zi = in ? zv : 0.0, wi = in ? wv : 0.0;
              q.sc0[il] = wi * zi; q.sc1[il] = fabs(wi * zi); q.sc2[il] = zi * zi;
            }
            WG_WSYNC();
            if (gmode == kSumsGuarded && !x_suspect) {
              // the three sums side by side, one per row of 16 lanes (row 3 shadows row 2): lane j of row s adds entries j, j + 16
              // and j + 32 of vector s, then the row is folded as a balanced tree on the DPP path (guard_rows_sum is this order on
              // the host).  The values may differ from the reference's in their last bits -- they are handed to the certificate
              // and to nothing else
              const int row = (lane >> 4) < 3 ? (lane >> 4) : 2, j = lane & 15;
              const int j2 = j + 32 < NM ? j + 32 : NM - 1;      // in bounds for every lane; past NM the value is dropped
              const double *vec = q.sc0 + row * (int)(q.sc1 - q.sc0);
              const double t0 = vec[j], t1 = vec[j + 16], t2 = vec[j2];
              double v = (t0 + t1) + (j + 32 < NM ? t2 : 0.0);
              v += dpp_zero<0x111, 0xf>(v);                       // row_shr:1, 2, 4, 8: lane 15 of a row holds its sum
              v += dpp_zero<0x112, 0xf>(v);
              v += dpp_zero<0x114, 0xf>(v);
              v += dpp_zero<0x118, 0xf>(v);
              suma = rl(v, 15); sumb = rl(v, 31); sumc = rl(v, 47);
              step_certain = WG_UBOOL(guard_route0(suma, sumb, sumc, knext <= m, wsel, wg_kconst(vsmall)));
            }
            if (!step_certain) {
              // doubt (or the reference's order asked for): the parent's three chains as rolled loops, lanes 0 .. 2
              if (gmode != kSumsOrdered) PT_COUNT2(PS_N_FALLBACK);
              const double *src = q.sc0 + (lane < 3 ? lane : 0) * (int)(q.sc1 - q.sc0);
              double acc = 0.0;
#pragma nounroll
              for (int i = 0; i < NM; ++i) acc += src[i];
              suma = rl(acc, 0); sumb = rl(acc, 1); sumc = rl(acc, 2);
            }
            WG_WSYNC();
          } else if constexpr (P::kNM > 0) {
            constexpr int NM = P::kNM;
            {
              // lanes past NM shadow lane NM - 1 (same value to the same address); loads from clamped addresses, selected values:
              // a load or a store under a lane-dependent condition is an exec-mask save / restore, here in every iteration
              const int il = lane < NM ? lane : NM - 1;
              const bool in = il < n;
              const int ic = in ? il : n - 1;
              const double zv = Zm(ic, nact), wv = q.ww[ic];
              const double zi = in ? zv : 0.0, wi = in ? wv : 0.0;
              q.sc0[il] = wi * zi; q.sc1[il] = fabs(wi * zi); q.sc2[il] = zi * zi;
            }
            WG_WSYNC();
            // three ordered sums of NM terms: lane 0 adds the first vector, lane 1 the second, lane 2 the third (the
            // scratch vectors are contiguous) -- one 8-cycle add chain per lane instead of three interleaved ones in all
            // the lane's vector through ONE typed address register with constant offsets (as in sweep_flat): as a plain pointer
            // every pair of loads got an address of its own, a v_add each, because the scratch vectors lie beyond the reach
            // of a two-entry load's offsets
            typedef __attribute__((address_space(3))) double lds_f64;
            const lds_f64 *src = (const lds_f64 *)(q.sc0 + (lane < 3 ? lane : 0) * (int)(q.sc1 - q.sc0));
            asm volatile("" : "+v"(src));
            double acc = 0.0;
#pragma unroll
            for (int i0 = 0; i0 < NM; i0 += kOsChunk) {
              double t[kOsChunk];
#pragma unroll
              for (int i = 0; i < kOsChunk; ++i) if (i0 + i < NM) t[i] = src[i0 + i];
#pragma unroll
              for (int i = 0; i < kOsChunk; ++i) if (i0 + i < NM) acc += t[i];
            }
            suma = rl(acc, 0); sumb = rl(acc, 1); sumc = rl(acc, 2);
            WG_WSYNC();
          } else {
            // column nact of Z is read once, lane-parallel (with Z in global memory: two coalesced loads instead of n
            // broadcast ones in a row); the three ordered sums then run from LDS, one per lane, as in the compact view
            for (int i = lane; i < n; i += 64) {
              const double zi = Zm(i, nact), wi = q.ww[i];
              q.sc0[i] = wi * zi; q.sc1[i] = fabs(wi * zi); q.sc2[i] = zi * zi;
            }
            WG_WSYNC();
            const double *src = q.sc0 + (lane < 3 ? lane : 0) * (int)(q.sc1 - q.sc0);
            double acc = 0.0;
            int i = 0;
            for (; i + 8 <= n; i += 8) {
              double t[8];
#pragma unroll
              for (int e = 0; e < 8; ++e) t[e] = src[i + e];
#pragma unroll
              for (int e = 0; e < 8; ++e) acc += t[e];
            }
            for (; i < n; ++i) acc += src[i];
            suma = rl(acc, 0); sumb = rl(acc, 1); sumc = rl(acc, 2);
            WG_WSYNC();
          }
          WG_SINK(suma); WG_SINK(sumb); WG_SINK(sumc);
          }   // WG_REP(5)
          if (kGuard && step_certain) route = 0;
          else if (WG_UBOOL(!significant(sumb, fabs(suma)) || !(sumb > wg_kconst(vsmall)))) route = 1;
          else {
            sumc = sqrt(sumc);
            if (knext <= m) sumc /= wsel;                    // wa[knext - 1]: the value the scan read
            if (WG_UBOOL(significant(sumc, fabs(suma)))) route = 0;
            else {                                          // :1538-1540
              PT_COUNT(PS_N_COORD);
              WG_BACKSUB(q, s, nact, lane);
              route = independent_coordinate(q, prob, knext, nact, vsmall, lane) ? 0 : 2;
            }
          }
        }
      }
      route = uni(route);
      PT(PS_ROUTE);
      PT_COUNT(PS_N_ROUTE);
      if (route != 0) PT_COUNT(PS_N_DEPENDENT);
      if (route != 0) {
        if (route == 1) WG_BACKSUB(q, s, nact, lane);
        kdrop = pick_drop<(P::kNM > 0), kNan>(q, nact, res, ratio, lane);
        info = -knext;                                      // :1663
        if (kdrop < 0) { st = ST_CONVERGED; continue; }
        parinc = ratio;
        parnew = parinc;
      }

      // ---- partial steps, each ending in a deletion, :1673-1759 ----
      bool dual_only = (route != 0);
      for (;;) {
        if (!dual_only) {
          sumy = s[nact];                                   // :1718-1720
          step = -res / sumy;
          parinc = step / sumy;
          kdrop = -1;
          if (nact > 0) {
            PT(PS_STEP_PRE);
            WG_REP(4) WG_BACKSUB(q, s, nact, lane);
            PT(PS_BACKSUB_STEP);
            WG_REP(7) { kdrop = pick_drop<(P::kNM > 0), kNan>(q, nact, res, ratio, lane); WG_SINK(kdrop); WG_SINK(ratio); }
            PT(PS_PICKDROP);
            if (kdrop >= 0) {                               // :1734-1743
              double temp = 1.0 - ratio / parinc;
              if (WG_UBOOL(temp <= 0.0)) kdrop = -1;
              else { step = ratio * sumy; parinc = ratio; res = temp * res; }
            }
          }
          if constexpr (P::kNM > 0) {                       // :1749-1755; surplus lanes shadow lane n - 1 (same address, same value)
            const int il = lane < n ? lane : n - 1;
            q.x[il] = q.x[il] + step * Zm(il, nact);
          } else
          for (int i = lane; i < n; i += 64) q.x[i] += step * Zm(i, nact);
          parnew += parinc;
          if constexpr (kNan) x_suspect = x_suspect || WG_UBOOL(!wg_sane(step) || !wg_sane(parinc));
          WG_WSYNC();
          if (nact < 1) break;
        }
        dual_only = false;
        if constexpr (P::kNM > 0) {                         // :1677-1687; surplus lanes shadow lane nact - 1
          if (nact > 0) {
            const int kl = lane < nact ? lane : nact - 1;
            const double l0 = q.lam[kl] - parinc * q.ww[kl];
            const int ia = q.iact[kl];
            q.lam[kl] = (ia > me) ? maxd(0.0, l0) : l0;
          }
        } else
        for (int k = lane; k < nact; k += 64) {             // :1677-1687
          double l = q.lam[k] - parinc * q.ww[k];
          if (q.iact[k] > me) l = maxd(0.0, l);
          q.lam[k] = l;
        }
        WG_WSYNC();
        if (kdrop < 0) break;
        {                                                   // :1697-1711
          int nu = nact + 1;
          LOG_EVENT(-q.iact[kdrop]);
          nact = drop_constraint(q, kdrop, nu, nact, lane);
          double *snew = s - (nact + 1);
          if (nu > n) nu = n;
          // ascending copy, source ahead of destination: lanes in index order
          for (int i0 = 0; i0 < nu; i0 += 64) {
            int i = i0 + lane;
            double v = (i < nu) ? s[i] : 0.0;
            WG_WSYNC();
            if (i < nu) snew[i] = v;
            WG_WSYNC();
          }
          s = snew;
          WG_SWEEP(q, s, nu, nact, lane);
        }
      }

      PT(PS_STEP);
      // ---- add the new constraint, :1764-1771 ----
      ql_activate(q, nact, knext, parnew, wsel, lane, n, mn);
      nact++;
      LOG_EVENT(knext);
      WG_WSYNC();
      PT(PS_ADD);
      double sm = 0.0;
      if constexpr (kGuard) {
        WG_REP(6) { sm = uni(xmag_sum_guarded(q, prob, vfact, lane, gmode == kSumsOrdered)); WG_SINK(sm); }   // :1776-1786
        xmag = maxd(xmag, sm);
        PT(PS_XMAG_ADD);
        bool reset;
        if (gmode == kSumsOrdered) reset = WG_UBOOL(sm < wg_kconst(xmagr) * xmag);
        else {
          const int verdict = x_suspect ? (int)kGuardDoubt : uni(guard_xmag(sm, xmag));
          if (verdict == kGuardDoubt) QL_RERUN_ORDERED;
          reset = verdict == kGuardReset;
        }
        if (reset) st = ST_RESET;
        else if (itref <= 0) st = ST_SCAN;
        else st = ST_RESID;
      } else {
      WG_REP(6) { sm = uni(xmag_sum(q, prob, vfact, lane)); WG_SINK(sm); }   // :1776-1786
      xmag = maxd(xmag, sm);
      PT(PS_XMAG_ADD);
      if (WG_UBOOL(sm < wg_kconst(xmagr) * xmag)) st = ST_RESET;
      else if (itref <= 0) st = ST_SCAN;
      else st = ST_RESID;
      }
      // R's LDS part is full (its columns and the working column hold nact finished columns): stop BETWEEN two iterations,
      // the loop's state goes to the caller, who moves R and resumes (or, without rs, repeats the solve from the start)
      if (q.nact_cap > 0 && nact > q.nact_cap) { cap_hit = true; break; }
      if (st == ST_SCAN) goto next_scan;
      continue;
    }

    if (st == ST_CONVERGED) {                               // :1791-1799
      ++itref;
      jfinc = -1;
      if (itref == 1) { st = ST_RESID; continue; }
      st = ST_FINISH;
    }
  }
  if constexpr (kGuard) { if (gmode == kSumsDoubt && !early_exit && !cap_hit) QL_RERUN_ORDERED; }   // tests: the whole solve doubted once
#undef QL_RERUN_ORDERED
#undef LOG_EVENT

  PT(PS_TAIL);
  PT_FLUSH;
  if (cap_hit) {
    if (rs) {
      rs->nact = nact; rs->info = info; rs->iterc = iterc; rs->itref = itref; rs->iflag = iflag; rs->jfinc = jfinc; rs->knext = knext;
      rs->st = st; rs->hist_len = out.hist_len;
      rs->xmag = xmag; rs->vfact = vfact; rs->res = res; rs->ratio = ratio; rs->diag = diag;
    }
    out.ifail = kQlCapHit; out.n_iter = iterc; out.nact = nact;
    return out;
  }
  out.ifail = ql_ifail_of(info);                          // ql0001 epilogue, :497-608
  out.n_iter = iterc;
  out.nact = nact;
  return out;
}

// ql_solve for a policy with guarded sums: a solve that leaves in doubt (kQlDoubt) is run again from its set-up in the reference's
// order -- once: the second pass has no certificate left to doubt.  One call site in a loop, so the solver is compiled once.
template <class P>
__device__ __forceinline__ QlResult ql_solve_guarded(const QlView &q, P &prob, double vsmall, int *hist, int hist_cap) {
  static_assert(GuardedSumsOf<P>::value, "for policies with kGuardedSums");
  QlResult r;
  for (;;) {
    r = ql_solve(q, prob, vsmall, hist, hist_cap);
    if (!WG_UBOOL(r.ifail == kQlDoubt)) break;
    prob.sums_mode = (prob.sums_mode & ~kSumsMask) | kSumsOrdered;   // the other bits of the word (the norms' mode) stay
  }
  return r;
}

}  // namespace wg
