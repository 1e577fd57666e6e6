#!/usr/bin/env python3
"""How far does the Morisawa-2007 method stay accurate in float64?  The measurement behind WG_MORISAWA_WALK_ARG_MAX
(include/wg_mpc.h) and DESIGN.md 3.13; its table is profiles/morisawa_admission.txt.

The restatement tests/morisawa.py alone, float64 (libm, numpy's LAPACK solve) against 50-digit mpmath: the library is not loaded,
the bound is not measured on the code it will admit.  d_ref(X) is the largest distance of a float64 sample from the 50-digit one
over the gaits whose largest omega_j dT_j is X -- CoM x, dx, y, dy, ZMP x, y and the twelve feet columns, at every sample of the
control clock where the interval changes, the last one and about 50 between (the rule of test_long_samples_against_the_mpmath_truth).

  X        8 .. 40 in steps of 0.5
  routes   "low"     a low CoM: t_single from SINGLE_TICKS, the height that makes omega * 3 t_single = X
           "single"  a height in [0.5, 1.0] m, the t_single that makes omega * 3 t_single = X
           "double"  a height in [0.5, 1.0] m, t_single = 0.5 s, the t_double that makes omega * t_double = X (the largest argument)
  gaits    per X and route, SEEDS seeded gaits at each S in (2, 7, 14, 24): steps, feet and start CoM drawn in the ranges of
           tests/morisawa_fleets.py's Fleet (restated here: that module loads the library for its structs)

X* is the largest grid value with D_REF_FACTOR * d_ref(X) < D_REF_CEILING at every grid X <= X* (the two constants of
tests/test_morisawa_host.py, DESIGN 3.13's contract).

    python tools/measure_morisawa_admission.py [--jobs N] [--seeds K] > profiles/morisawa_admission.txt"""
import argparse
import math
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import morisawa as mo  # noqa: E402

D_REF_FACTOR, D_REF_CEILING = 16.0, 1e-8         # tests/test_morisawa_host.py
T = 0.005
SINGLE_TICKS = (100, 120, 140, 156, 160)          # tests/morisawa_fleets.py
DOUBLE_TICKS = (4, 8, 12, 20)
ROUTES = ("low", "single", "double")
STEPS = (2, 7, 14, 24)
G = 9.86


def argument(h, ts, td):
    """the largest omega_j dT_j, as the library writes it"""
    om = math.sqrt(G / (h - 0.0))
    return max(om * (ts * 3.0), om * td)


def timing(route, X, rng):
    """(height, t_single, t_double) whose argument is X to a few ulp"""
    if route == "low":
        ts = SINGLE_TICKS[rng.integers(len(SINGLE_TICKS))] * T
        td = DOUBLE_TICKS[rng.integers(len(DOUBLE_TICKS))] * T
        return G * (3.0 * ts / X) ** 2, ts, td
    h = rng.uniform(0.5, 1.0)
    om = math.sqrt(G / h)
    if route == "single":
        return h, X / (3.0 * om), DOUBLE_TICKS[rng.integers(len(DOUBLE_TICKS))] * T
    return h, SINGLE_TICKS[0] * T, X / om         # omega * 3 t_single <= 6.67 < 8 <= X


def gait(S, b, rng):
    """steps, init_feet, (com x, com y) of one gait, as Fleet.__init__ draws gait b"""
    side = -1.0 if b % 2 == 0 else 1.0
    turn = (0.0, 10.0, -10.0, None)[b % 4]
    steps = []
    for i in range(S):
        th = rng.uniform(-10.0, 10.0) if turn is None else turn
        sx = 0.0 if i == 0 else rng.uniform(0.0, 0.25)
        sy = side * (0.105 if i == 0 else rng.uniform(0.17, 0.21))
        steps.append((sx, sy, th if i > 0 else 0.0))
        side = -side
    feet = [rng.uniform(-0.05, 0.05), rng.uniform(0.08, 0.1), rng.uniform(-5, 5) * (b % 3 == 0),
            rng.uniform(-0.05, 0.05), -rng.uniform(0.08, 0.1), rng.uniform(-5, 5) * (b % 3 == 0)]
    return steps, feet, (rng.uniform(0.0, 0.04), rng.uniform(-0.01, 0.01))


def d_ref_of(model, steps, feet, com0):
    """the largest distance of the float64 restatement's samples from the 50-digit one's, on the control clock from 2 t_single"""
    try:
        with np.errstate(all="ignore"):
            w64 = mo.Walk(mo.F64, model, steps, feet, com0)
    except np.linalg.LinAlgError:                  # Z singular to LAPACK: no walk at all
        return float("inf")
    truth = mo.Walk(mo.MP, model, steps, feet, com0)
    t0 = 2.0 * model["t_single"]
    L = mo.length(model, len(steps), t0)
    clk = mo.clock(t0, T, L)
    iv = [w64.interval(t) for t in clk]
    ks = sorted(set(list(range(0, L, max(1, L // 50))) + [L - 1] + [k for k in range(1, L) if iv[k] != iv[k - 1]]))
    worst = 0.0
    for k in ks:
        t, s = truth.sample(clk[k]), w64.sample(clk[k])
        tv = [float(x) for x in t["com"] + t["zmp"] + t["left"] + t["right"]]
        sv = s["com"] + s["zmp"] + s["left"] + s["right"]
        d = max(abs(a - c) for a, c in zip(sv, tv))
        worst = max(worst, d if d == d else float("inf"))
    return worst


def cell(task):
    X, r, S, seed = task
    rng = np.random.default_rng([2007, int(round(2 * X)), r, S, seed])
    h, ts, td = timing(ROUTES[r], X, rng)
    steps, feet, (cx, cy) = gait(S, seed + r, rng)
    model = dict(T=T, t_single=ts, t_double=td, step_height=rng.uniform(0.05, 0.1), omega=(0.0, 5.0)[seed % 2])
    return X, r, S, argument(h, ts, td), d_ref_of(model, steps, feet, (cx, cy, h))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--seeds", type=int, default=2, help="gaits per X, route and step count (default 2: 24 gaits per X)")
    a = ap.parse_args()
    grid = [8.0 + 0.5 * i for i in range(65)]
    tasks = [(X, r, S, seed) for X in grid for r in range(len(ROUTES)) for S in STEPS for seed in range(a.seeds)]
    tasks.sort(key=lambda t: -t[2])                # the 24-step gaits first: they take longest
    with multiprocessing.Pool(a.jobs) as pool:
        done = pool.map(cell, tasks, chunksize=1)
    worst = {(X, r): 0.0 for X in grid for r in range(len(ROUTES))}
    at_S = {(X, r): 0 for X in grid for r in range(len(ROUTES))}
    for X, r, S, arg, d in done:
        assert abs(arg - X) <= 1e-12 * X, (X, r, arg)
        if d >= worst[X, r]:
            worst[X, r], at_S[X, r] = d, S
    print("# Morisawa-2007 in float64 against 50 digits: d_ref (m) by the largest argument X = max omega_j dT_j")
    print("# tools/measure_morisawa_admission.py --seeds %d: %d gaits per X (routes %s; S in %s)" %
          (a.seeds, len(ROUTES) * len(STEPS) * a.seeds, ", ".join(ROUTES), ", ".join(map(str, STEPS))))
    print("# rule: %g x d_ref < %g m" % (D_REF_FACTOR, D_REF_CEILING))
    print("#    X   %-10s %-10s %-10s  d_ref      at S  16 x d_ref  holds" % ROUTES)
    x_star, holding = None, True
    for X in grid:
        ds = [worst[X, r] for r in range(len(ROUTES))]
        d = max(ds)
        ok = D_REF_FACTOR * d < D_REF_CEILING
        holding = holding and ok
        if holding:
            x_star = X
        print("%6.1f   %-10.3g %-10.3g %-10.3g  %-10.3g %-4d  %-10.3g  %s" %
              (X, ds[0], ds[1], ds[2], d, at_S[X, ds.index(d)], D_REF_FACTOR * d, "yes" if ok else "no"))
    assert x_star is not None, "the rule fails at the grid's first argument"
    print("X* = %.1f" % x_star)


if __name__ == "__main__":
    main()
