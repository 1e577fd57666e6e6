"""The certificates of the guarded sums (jrl-walkgen_amd/csrc/wg_ql_guard.hpp) on the host, without a GPU.

The N = 16 solver forms four sums that only decide a branch -- suma, sumb, sumc of the linear-dependence test and lql's magnitude
sum -- as a tree over the lanes and lets a certificate say whether the decision is the reference's.  The header compiles for host and
device from one text; here g++ builds it into a small shared object (no FMA contraction, as everywhere).

1. Property check.  Random and adversarial terms (cancelling pairs, |suma| at the 2^-40 boundary, bases at powers of two, zeros,
   subnormals, 1e300, infinities, NaN), every sum formed in index order, reversed, pairwise and in the device's two orders (the
   64-lane tree of the magnitude sum, the 16-lane rows of the dependence sums): whenever
   a certificate decides from ANY of these orders, its decision must be what the reference's own tests (ql0002's `significant`,
   `sumb > vsmall`, `sum < 0.01 xmag` with f2c's max) give on the index-order sums.  A certificate that never decided would pass
   that vacuously, so plain well-conditioned inputs must be decided.
2. Sample check.  A throw-away build of oracle/ql_oracle.c with hooks at the dependence test and at both magnitude sites (the way
   tests/test_iteration_paths_gpu.py instruments it; the patched text lives in a temp dir) solves every QP of that module's sample
   (B = 64, T = 48, velocity references x 1, 3, 7) and applies the certificates to tree-order sums, following the device: after a
   doubt at the magnitude test the rest of that solve counts as run in the reference's order.  Scale 1: no doubt at either site.
   Scales 3 and 7: doubts at the dependence site and resets occur, and the doubts stay below 1 % of the decisions.  No certificate
   may contradict the oracle anywhere."""
import atexit
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jrl-walkgen_amd", "csrc")
CXXFLAGS = ["-O2", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra"]
NMAX = 36                                                         # the compact view: n <= 2 N + 4

_CHECK_CPP = r"""
#include "wg_ql_guard.hpp"
#include <cmath>
using namespace wg;
namespace {
// the reference's tests, as oracle/ql_oracle.c and qld.cpp state them
bool significant(double base, double delta_abs) {
  double temp = base + delta_abs * .1;
  double tempa = base + delta_abs * .2;
  if (temp <= base) return false;
  if (tempa <= temp) return false;
  return true;
}
double maxd(double a, double b) { return a >= b ? a : b; }
double pairwise(const double *t, int lo, int hi) {
  if (hi - lo == 1) return 0.0 + t[lo];
  if (hi <= lo) return 0.0;
  const int mid = lo + (hi - lo) / 2;
  return pairwise(t, lo, mid) + pairwise(t, mid, hi);
}
// order 0: index order from 0.0 (the reference), 1: reversed, 2: pairwise over n, 3: the device's tree over 64 zero-padded lanes
// (the magnitude sum), 4: the device's rows of 16 lanes (the dependence sums)
double sum_in(const double *t, int n, int order) {
  double s = 0.0;
  switch (order) {
    case 0: for (int i = 0; i < n; ++i) s += t[i]; return s;
    case 1: for (int i = n - 1; i >= 0; --i) s += t[i]; return s;
    case 2: return pairwise(t, 0, n);
    case 3: return guard_tree_sum(t, n);
    default: return guard_rows_sum(t, n);
  }
}
}
extern "C" {
// bit k of the result: the certificate decided route 0 from order k's sums; bit 8: the reference's tests say route 0
int gs_check_dep(const double *w, const double *z, int n, int by_wa, double wa, double vsmall) {
  double p[64], ap[64], zz[64];
  for (int i = 0; i < n; ++i) { p[i] = w[i] * z[i]; ap[i] = std::fabs(w[i] * z[i]); zz[i] = z[i] * z[i]; }
  int out = 0;
  {
    const double suma = sum_in(p, n, 0), sumb = sum_in(ap, n, 0);
    double sumc = sum_in(zz, n, 0);
    bool route0 = false;
    if (!significant(sumb, std::fabs(suma)) || !(sumb > vsmall)) route0 = false;
    else {
      sumc = std::sqrt(sumc);
      if (by_wa) sumc /= wa;
      route0 = significant(sumc, std::fabs(suma));
    }
    if (route0) out |= 256;
  }
  for (int k = 0; k < 5; ++k)
    if (guard_route0(sum_in(p, n, k), sum_in(ap, n, k), sum_in(zz, n, k), by_wa != 0, wa, vsmall)) out |= 1 << k;
  return out;
}
// terms: nsum vectors of n non-negative terms, the sums since the last reset; the decision is taken at the last one.
// verdict[k] for order k: -1 doubt (also: an earlier sum the running maximum may not follow), 0 no reset, 1 reset; returns the reference's
int gs_check_xmag(const double *terms, int nsum, int n, int *verdict) {
  int ref = 0;
  for (int k = 0; k < 5; ++k) {
    double xmag = 0.0, s = 0.0;
    bool doubt = false;
    for (int j = 0; j < nsum; ++j) {
      s = sum_in(terms + (long)j * n, n, k);
      if (k != 0 && j + 1 < nsum && !guard_xmag_update(s)) doubt = true;
      xmag = maxd(xmag, s);
    }
    if (k == 0) ref = s < .01 * xmag ? 1 : 0;
    verdict[k] = doubt ? -1 : guard_xmag(s, xmag);
  }
  return ref;
}
double gs_sum(const double *t, int n, int order) { return sum_in(t, n, order); }
}
"""

_HOOKS_CPP = r"""
#include "wg_ql_guard.hpp"
#include <cmath>
using namespace wg;
namespace {
bool significant(double base, double delta_abs) {
  double temp = base + delta_abs * .1, tempa = base + delta_abs * .2;
  return !(temp <= base) && !(tempa <= temp);
}
double xmag_tree = 0.0;
bool ordered = false;      // after a doubt at the magnitude test the device runs the solve again in the reference's order
}
extern "C" {
// 0 dependence tests, 1 of them doubted, 2 certified against the oracle, 3 not route 0 by the oracle's first two tests and its third,
// 4 magnitude decisions, 5 doubts at a magnitude site, 6 certified against the oracle, 7 resets by the oracle
__attribute__((visibility("default"))) long long wg_gs_count[8];
void wg_gs_solve_begin(void) { ordered = false; xmag_tree = 0.0; }
void wg_gs_xmag_reset(void) { xmag_tree = 0.0; }
void wg_gs_dep(const double *w, const double *z, int n, int by_wa, double wa, double vsmall) {
  double p[80], ap[80], zz[80], suma = 0.0, sumb = 0.0, sumc = 0.0;
  for (int i = 0; i < n; ++i) {
    p[i] = w[i] * z[i]; ap[i] = std::fabs(w[i] * z[i]); zz[i] = z[i] * z[i];
    suma += p[i]; sumb += ap[i]; sumc += zz[i];
  }
  bool route0 = false;
  if (significant(sumb, std::fabs(suma)) && sumb > vsmall) {
    double c = std::sqrt(sumc);
    if (by_wa) c /= wa;
    route0 = significant(c, std::fabs(suma));
  }
  ++wg_gs_count[0];
  if (!route0) ++wg_gs_count[3];
  if (ordered) return;
  if (!guard_route0(guard_rows_sum(p, n), guard_rows_sum(ap, n), guard_rows_sum(zz, n), by_wa != 0, wa, vsmall)) ++wg_gs_count[1];
  else if (!route0) ++wg_gs_count[2];
}
void wg_gs_xmag(const double *t, int n, int decide, int ref_reset) {
  if (decide) { ++wg_gs_count[4]; if (ref_reset) ++wg_gs_count[7]; }
  if (ordered) return;
  const double s = guard_tree_sum(t, n);
  if (!decide) {
    if (!guard_xmag_update(s)) { ++wg_gs_count[5]; ordered = true; return; }
    xmag_tree = xmag_tree >= s ? xmag_tree : s;
    return;
  }
  xmag_tree = xmag_tree >= s ? xmag_tree : s;
  const int v = guard_xmag(s, xmag_tree);
  if (v == kGuardDoubt) { ++wg_gs_count[5]; ordered = true; }
  else if (v != ref_reset) ++wg_gs_count[6];
}
}
"""

_HOOKS_H = """
void wg_gs_solve_begin(void);
void wg_gs_xmag_reset(void);
void wg_gs_dep(const double *w, const double *z, int n, int by_wa, double wa, double vsmall);
void wg_gs_xmag(const double *t, int n, int decide, int ref_reset);
#define WG_GS_XMAG(decide, ref) do { double t_[80]; for (int i_ = 0; i_ < q->n; ++i_) \\
    t_[i_] = fabs(q->x[i_]) * vfact * (fabs(q->grad[i_]) + fabs(G(i_, i_) * q->x[i_])); wg_gs_xmag(t_, q->n, decide, ref); } while (0)
#define WG_GS_DEP() do { double w_[80], z_[80]; for (int i_ = 0; i_ < n; ++i_) { w_[i_] = q->ww[i_]; z_[i_] = Z(i_, q->nact); } \\
    wg_gs_dep(w_, z_, n, knext <= m, knext <= m ? q->wa[knext - 1] : 1.0, q->vsmall); } while (0)
"""
_SITES = (                                                        # one line of oracle/ql_oracle.c each, and what it becomes
    (r"^(\s*double xmag = 0\.0, vfact = 1\.0;)\s*$", r"\1 wg_gs_solve_begin();"),
    (r"^(\s*xmag = 0\.0;)\s*$", r"\1 wg_gs_xmag_reset();"),
    (r"^(\s*)(\{ double sm = xmag_sum\(q, vfact\); xmag = MAXD\(xmag, sm\); \}.*)$", r"\1WG_GS_XMAG(0, 0); \2"),
    (r"^(\s*)(if \(!significant\(sumb, fabs\(suma\)\) \|\| !\(sumb > q->vsmall\)\) route = 1;)\s*$", r"\1WG_GS_DEP(); \2"),
    (r"^(\s*)(if \(sm < xmagr \* xmag\) st = ST_RESET;)\s*$", r"\1WG_GS_XMAG(1, sm < xmagr * xmag); \2"),
)


def _tmpdir(prefix):
    d = tempfile.mkdtemp(prefix=prefix)
    atexit.register(shutil.rmtree, d, True)
    return d


@functools.lru_cache(maxsize=None)
def _check_lib():
    d = _tmpdir("wg_guard_check_")
    open(os.path.join(d, "check.cpp"), "w").write(_CHECK_CPP)
    so = os.path.join(d, "libguard_check.so")
    subprocess.check_call(["g++"] + CXXFLAGS + ["-I", CSRC, "-shared", "-o", so, os.path.join(d, "check.cpp")])
    lib = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    lib.gs_check_dep.argtypes = [dp, dp, C.c_int, C.c_int, C.c_double, C.c_double]
    lib.gs_check_xmag.argtypes = [dp, C.c_int, C.c_int, C.POINTER(C.c_int)]
    lib.gs_sum.argtypes = [dp, C.c_int, C.c_int]
    lib.gs_sum.restype = C.c_double
    return lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


# ---------------------------------------------------------------------------------------------------------------- inputs
SPECIALS = (0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-300, 1e300, -1e300, 1.7e308, np.inf, -np.inf, np.nan)


def _dep_cases(rng):
    """(w, z, by_wa, wa) with terms w_i z_i.  z_i = 1 (or a power of two) wherever the terms themselves are to be controlled."""
    out = []
    for _ in range(4000):                                         # plain: well-conditioned products of normal numbers
        n = int(rng.integers(1, NMAX + 1))
        out.append((rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6), rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3),
                    int(rng.integers(0, 2)), 10.0 ** rng.uniform(-4, 4), "plain"))
    for _ in range(4000):                                         # cancelling pairs plus a residual around 2^-40 sumb (and around
        n = int(rng.integers(3, NMAX + 1))                        # 2^-40 sqrt(sumc) / wa), bases at powers of two
        half = (n - 1) // 2
        e = int(rng.integers(-30, 31))
        if rng.integers(0, 2):
            mag = np.full(half, 2.0 ** e)                          # equal powers of two: every order gives the same sumb
        else:
            mag = rng.uniform(0.5, 2.0, size=half) * 2.0 ** e
        w = np.zeros(n)
        w[:half] = mag
        w[half:2 * half] = -mag
        rng.shuffle(w[:2 * half])
        sumb = np.abs(w).sum()
        z = np.ones(n)
        by_wa = int(rng.integers(0, 2))
        wa = 2.0 ** int(rng.integers(-20, 21))
        base = sumb
        if rng.integers(0, 2) and by_wa:
            base = max(sumb, np.sqrt(float(n)) / wa)
        k = rng.choice([2.0 ** -40, 2.0 ** -40 * (1 + 2.0 ** -40), 2.0 ** -40 + 2.0 ** -46, 2.0 ** -46, 2.0 ** -50, 2.0 ** -52, 2.0 ** -30])
        w[n - 1] = base * k * (1.0 + rng.choice([0.0, 1.0, -1.0, 4.0, -4.0, 64.0, -64.0]) * 2.0 ** -48) * rng.choice([1.0, -1.0])
        out.append((w, z, by_wa, wa, "boundary"))
    for _ in range(3000):                                         # zeros, subnormals, 1e300, infinities, NaN among ordinary terms
        n = int(rng.integers(1, NMAX + 1))
        w = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3)
        z = rng.choice([1.0, 1.0, 2.0, 0.5, -1.0], size=n)
        for _k in range(int(rng.integers(1, 4))):
            w[int(rng.integers(0, n))] = rng.choice(SPECIALS)
        if rng.integers(0, 4) == 0:
            z[int(rng.integers(0, n))] = rng.choice(SPECIALS)
        if rng.integers(0, 4) == 0:
            w[:] = rng.choice([0.0, 5e-324, 1e-310, 1e300, 1e150], size=n) * rng.choice([1.0, -1.0], size=n)
        wa = float(rng.choice([1.0, 1e-300, 1e300, 0.0, -1.0, np.inf, np.nan, 5e-324, 1e-8]))
        out.append((w, z, int(rng.integers(0, 2)), wa, "special"))
    for _ in range(1500):                                         # sumb around vsmall = 1e-8
        n = int(rng.integers(1, NMAX + 1))
        w = rng.uniform(0.5, 1.5, size=n)
        w *= 1e-8 * (1.0 + rng.choice([0.0, 1.0, -1.0, 8.0, -8.0, 1e3, -1e3]) * 2.0 ** -47) / w.sum()
        out.append((w, np.ones(n), 0, 1.0, "vsmall"))
    return out


def test_route0_certificate_never_contradicts_the_reference():
    lib = _check_lib()
    rng = np.random.default_rng(20100)
    decided = {"plain": [0, 0], "boundary": [0, 0], "special": [0, 0], "vsmall": [0, 0]}
    for w, z, by_wa, wa, kind in _dep_cases(rng):
        w = np.ascontiguousarray(w, dtype=np.float64)
        z = np.ascontiguousarray(z, dtype=np.float64)
        with np.errstate(all="ignore"):
            r = lib.gs_check_dep(_dp(w), _dp(z), len(w), by_wa, wa, 1e-8)
        ref = bool(r & 256)
        for k in range(5):
            if r & (1 << k):
                assert ref, ("order %d certified route 0 against the reference's tests" % k, kind, w.tolist(), z.tolist(), by_wa, wa)
        decided[kind][0] += 1
        decided[kind][1] += int(r & 16 != 0)
    print({k: "%d of %d decided in the device's order" % (v[1], v[0]) for k, v in decided.items()})
    assert decided["plain"][1] >= 0.9 * decided["plain"][0], decided       # not vacuous
    assert 0 < decided["boundary"][1] < decided["boundary"][0], decided   # the boundary cases sit on both sides


def _xmag_cases(rng):
    out = []
    for _ in range(3000):                                         # plain: a few sums of comparable size -> no reset
        n, k = int(rng.integers(1, NMAX + 1)), int(rng.integers(1, 5))
        out.append((np.abs(rng.normal(size=(k, n))) * 10.0 ** rng.uniform(-6, 6), "plain"))
    for _ in range(3000):                                         # the last sum around 0.01 x an earlier one
        n = int(rng.integers(1, NMAX + 1))
        t = np.zeros((2, n))
        if rng.integers(0, 2):
            t[0] = 2.0 ** int(rng.integers(-20, 21))
        else:
            t[0] = rng.uniform(0.5, 2.0, size=n) * 2.0 ** int(rng.integers(-20, 21))
        t[1] = rng.uniform(0.5, 1.5, size=n)
        k = rng.choice([1.0, 1 + 2.0 ** -40, 1 - 2.0 ** -40, 1 + 2.0 ** -46, 1 - 2.0 ** -46, 1 + 2.0 ** -38, 1 - 2.0 ** -38, 1 + 2.0 ** -52, 0.5, 2.0])
        t[1] *= 0.01 * t[0].sum() * k / t[1].sum()
        out.append((t, "boundary"))
    for _ in range(2000):                                         # zeros, subnormals, huge values, infinities, NaN
        n, k = int(rng.integers(1, NMAX + 1)), int(rng.integers(1, 4))
        t = np.abs(rng.normal(size=(k, n)))
        for _j in range(int(rng.integers(1, 4))):
            t[int(rng.integers(0, k)), int(rng.integers(0, n))] = abs(rng.choice(SPECIALS))
        if rng.integers(0, 3) == 0:
            t[int(rng.integers(0, k))] = rng.choice([0.0, 5e-324, 1e300, 1e-310])
        out.append((t, "special"))
    return out


def test_magnitude_certificate_never_contradicts_the_reference():
    lib = _check_lib()
    rng = np.random.default_rng(20101)
    verdict = (C.c_int * 5)()
    seen = {"plain": [0, 0, 0], "boundary": [0, 0, 0], "special": [0, 0, 0]}     # doubt, no reset, reset (tree order)
    for t, kind in _xmag_cases(rng):
        t = np.ascontiguousarray(t, dtype=np.float64)
        with np.errstate(all="ignore"):
            ref = lib.gs_check_xmag(_dp(t), t.shape[0], t.shape[1], verdict)
        for k in range(5):
            assert verdict[k] in (-1, ref), ("order %d decided %d, the reference %d" % (k, verdict[k], ref), kind, t.tolist())
        seen[kind][verdict[3] + 1] += 1
    print(seen)
    assert seen["plain"][0] == 0, seen                              # not vacuous: comparable sums are decided
    assert all(v > 0 for v in seen["boundary"]), seen               # doubts, certified no-resets and certified resets all occur


def test_tree_order_is_a_balanced_tree_over_64_lanes():
    """guard_tree_sum against the definition the device's DPP steps implement, and a case where it differs from the index order."""
    lib = _check_lib()
    rng = np.random.default_rng(5)
    differ = 0
    for _ in range(200):
        n = int(rng.integers(1, NMAX + 1))
        t = np.ascontiguousarray(rng.normal(size=n) * 10.0 ** rng.uniform(-8, 8, size=n))
        v = np.zeros(64)
        v[:n] = t
        while len(v) > 1:
            v = v[1::2] + v[0::2]
        got = lib.gs_sum(_dp(t), n, 3)
        assert got == v[0]
        differ += int(got != lib.gs_sum(_dp(t), n, 0))
        # the dependence sums: lane j of a 16-lane row starts from (t_j + t_{j+16}) + t_{j+32}, then the row's tree
        p = np.zeros(48)
        p[:n] = t
        v = (p[0:16] + p[16:32]) + p[32:48]
        while len(v) > 1:
            v = v[1::2] + v[0::2]
        assert lib.gs_sum(_dp(t), n, 4) == v[0]
    assert differ > 0


# ---------------------------------------------------------------------------------------------------------------- the sample
@functools.lru_cache(maxsize=None)
def _hooked_oracle():
    import oraclelib as ol
    lines = open(os.path.join(ol.ORACLE_DIR, "ql_oracle.c")).read().split("\n")
    for pat, repl in _SITES:
        hit = [i for i, l in enumerate(lines) if re.match(pat, l)]
        assert len(hit) == 1, (pat, hit)
        lines[hit[0]] = re.sub(pat, repl, lines[hit[0]])
    d = _tmpdir("wg_guard_sample_")
    open(os.path.join(d, "hooks.h"), "w").write(_HOOKS_H)
    open(os.path.join(d, "ql_hooked.c"), "w").write("\n".join(lines))
    open(os.path.join(d, "hooks.cpp"), "w").write(_HOOKS_CPP)
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-std=c99", "-ffp-contract=off", "-fno-fast-math", "-I", ol.ORACLE_DIR,
                           "-include", os.path.join(d, "hooks.h"), "-c", "-o", os.path.join(d, "ql_hooked.o"), os.path.join(d, "ql_hooked.c")])
    subprocess.check_call(["g++"] + CXXFLAGS + ["-I", CSRC, "-c", "-o", os.path.join(d, "hooks.o"), os.path.join(d, "hooks.cpp")])
    so = os.path.join(d, "libql_hooked.so")
    subprocess.check_call(["g++", "-shared", "-o", so, os.path.join(d, "ql_hooked.o"), os.path.join(d, "hooks.o"), "-lm"])
    return C.CDLL(so)


@functools.lru_cache(maxsize=None)
def _sample_counts(scale):
    """Every QP of the sample's recipe at this scale, as the oracle's tick dumped it, solved again by the hooked build."""
    import herdt_replay as hr
    import test_iteration_paths_gpu as ip
    import workload as w
    lib = _hooked_oracle()
    count = (C.c_longlong * 8).in_dll(lib, "wg_gs_count")
    for k in range(8):
        count[k] = 0
    xl, xu = (C.c_double * 80)(*([-1e8] * 80)), (C.c_double * 80)(*([1e8] * 80))
    x, u, iact, hist = (C.c_double * 80)(), (C.c_double * 360)(), (C.c_int * 128)(), (C.c_int * hr.HIST_CAP)()
    pt = w.ptrig()
    model = hr.default_model()
    vel = ip._table(scale)
    dump, out = hr.QpDump(), hr.TickOut()

    def on_tick(t, s):
        ifail, nact, nit, hlen = C.c_int(-99), C.c_int(0), C.c_int(0), C.c_int(0)
        n, m = dump.n, dump.m
        assert n <= NMAX and dump.mmax <= 200
        lib.wgo_ql_solve(C.c_int(m), C.c_int(0), C.c_int(dump.mmax), C.c_int(n), C.c_int(n), dump.C, dump.d, dump.A, dump.b,
                         xl, xu, C.c_double(1e-8), x, u, C.byref(ifail), iact, C.byref(nact), C.byref(nit), hist,
                         C.c_int(hr.HIST_CAP), C.byref(hlen))
        assert (ifail.value, nit.value, nact.value, hlen.value) == (dump.ifail, dump.n_iter, dump.nact, dump.hist_len)   # the same solve

    for g in range(ip.B):
        w.oracle_follow(pt, model, w.start_state(hr.init_state, model), vel[:, g], ip.T, on_tick=on_tick, out=out, dump=dump)
    names = ("dep_tests", "dep_doubt", "dep_wrong", "dep_not_route0", "xmag_tests", "xmag_doubt", "xmag_wrong", "resets")
    return dict(zip(names, (int(v) for v in count)))


def test_sample_scale_1_is_decided_without_a_doubt():
    c = _sample_counts(1.0)
    print(c)
    assert c["dep_wrong"] == 0 and c["xmag_wrong"] == 0, c
    assert c["dep_tests"] > 0 and c["xmag_tests"] > 0, c
    assert c["dep_doubt"] == 0 and c["xmag_doubt"] == 0, c


def test_sample_scales_3_and_7_doubt_rarely_and_never_wrongly():
    for scale in (3.0, 7.0):
        c = _sample_counts(scale)
        print("scale %g:" % scale, c)
        assert c["dep_wrong"] == 0 and c["xmag_wrong"] == 0, (scale, c)
        assert c["dep_doubt"] > 0 and c["resets"] > 0, (scale, c)
        assert c["dep_doubt"] + c["xmag_doubt"] <= 0.01 * (c["dep_tests"] + c["xmag_tests"]), (scale, c)
        assert c["dep_doubt"] <= 0.01 * c["dep_tests"], (scale, c)
