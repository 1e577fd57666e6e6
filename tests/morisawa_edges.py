"""The edge fleet of tests/test_morisawa_edges_host.py and tests/test_morisawa_edges_gpu.py, stated once: gaits of tests/morisawa_fleets.py
whose height and times put the largest argument omega_j dT_j between 8 and the admission bound WG_MORISAWA_WALK_ARG_MAX
(include/wg_mpc.h), on it from both sides, and beyond it.  The bound is one of accuracy: tools/measure_morisawa_admission.py and
DESIGN.md 3.13.

An argument X is reached by three routes:
  "low"     a low CoM: t_single from SINGLE_TICKS, the height that makes omega * 3 t_single = X
  "single"  a height in [0.5, 1.0] m and the long t_single that makes omega * 3 t_single = X
  "double"  a long t_double, omega * t_double = X the largest argument (t_single = 0.1 s; the height is low, which keeps the
            walk short enough to sample)
No tests here."""
import functools
import math
import os
import re
import types

import numpy as np

import morisawa_fleets as mf

ROUTES = ("low", "single", "double")
G = 9.86
B = 67
LN2 = math.log(2.0)
EXP_K_MIN_ARG = 10.75                     # int(x / ln 2 + 0.5) >= 16 from here on: mo_exp's `k & 16` products
# gaits of the edge fleet on the bound -- the last t_single within it ("in"), the first one past it ("out") -- and beyond it
ON_BOUND = {4: ("single", "in"), 5: ("single", "out"), 6: ("low", "out"), 7: ("low", "in")}
BEYOND = {21: lambda bound: bound + 0.5, 34: lambda bound: bound + 4.0, 47: lambda bound: 0.5 * (bound + 40.0), 63: lambda bound: 40.0,
          66: lambda bound: 41.0}


def header_bound():
    hdr = open(os.path.join(mf.ROOT, "include", "wg_mpc.h")).read()
    return float(re.search(r"#define WG_MORISAWA_WALK_ARG_MAX ([0-9.]+)", hdr).group(1))


def measured_bound():
    txt = open(os.path.join(mf.ROOT, "profiles", "morisawa_admission.txt")).read()
    return float(re.search(r"^X\* = ([0-9.]+)$", txt, re.M).group(1))


def arguments(h, ts, td):
    """omega * 3 t_single and omega * t_double in float64, as the library writes them"""
    om = math.sqrt(G / (h - 0.0))
    return om * (ts * 3.0), om * td


def argument(h, ts, td):
    return max(arguments(h, ts, td))


def is_admitted(h, ts, td, bound):
    a, b = arguments(h, ts, td)
    return a <= bound and b <= bound


def timing(route, X, rng, double_height=(0.5, 1.0), double_single=mf.SINGLE_TICKS[0] * 0.005):
    """(height, t_single, t_double) with the argument X to a few ulp"""
    T = 0.005
    if route == "low":
        ts = mf.SINGLE_TICKS[rng.integers(len(mf.SINGLE_TICKS))] * T
        return G * (3.0 * ts / X) ** 2, ts, mf.DOUBLE_TICKS[rng.integers(len(mf.DOUBLE_TICKS))] * T
    if route == "single":
        h = rng.uniform(0.5, 1.0)
        return h, X / (3.0 * math.sqrt(G / h)), mf.DOUBLE_TICKS[rng.integers(len(mf.DOUBLE_TICKS))] * T
    h = rng.uniform(*double_height)
    om = math.sqrt(G / h)
    assert om * (double_single * 3.0) < 8.0
    return h, double_single, X / om


def step_to_bound(route, h, ts, td, bound):
    """the route's time moved by nextafter onto the bound: ((h, ts, td) of the last argument within it, of the first one past it)"""
    which = 2 if route == "double" else 1
    v = [h, ts, td]
    arg = lambda x: arguments(*(v[:which] + [x] + v[which + 1:]))[0 if which == 1 else 1]  # noqa: E731
    x = v[which]
    while arg(x) > bound:
        x = float(np.nextafter(x, 0.0))
    while arg(float(np.nextafter(x, np.inf))) <= bound:
        x = float(np.nextafter(x, np.inf))
    y = float(np.nextafter(x, np.inf))
    assert arg(x) <= bound < arg(y) and bound - arg(x) <= 1e-12 * bound and arg(y) - bound <= 1e-12 * bound
    inside, outside = list(v), list(v)
    inside[which], outside[which] = x, y
    assert is_admitted(*inside, bound) and not is_admitted(*outside, bound)
    return tuple(inside), tuple(outside)


def set_timing(f, b, h, ts, td):
    f.com0[b, 2] = h
    f.models[b].t_single, f.models[b].t_double = ts, td


@functools.lru_cache(maxsize=None)
def edge_fleet(smax):
    """mf.Fleet(67, smax) with a height and times per gait; .arg [B] the largest argument, .admitted [B], .route [B], .bound.
    Shared between the tests and never modified: `without` makes the fleets that differ from it."""
    bound = header_bound()
    f = mf.Fleet(B, smax, 1600 + smax)
    rng = np.random.default_rng(1700 + smax)
    f.bound, f.route = bound, [ROUTES[b % 3] for b in range(B)]
    for b in range(B):
        if b in ON_BOUND:
            f.route[b], side = ON_BOUND[b]
            inside, outside = step_to_bound("single", *timing(f.route[b], bound, rng), bound)      # both routes step t_single
            set_timing(f, b, *(inside if side == "in" else outside))
            continue
        X = BEYOND[b](bound) if b in BEYOND else 8.0 + (bound - 8.0) * b / B      # 8 up to, not onto, the bound
        set_timing(f, b, *timing(f.route[b], X, rng, double_height=(0.05, 0.1), double_single=0.1))
    f.arg = np.array([argument(f.com0[b, 2], f.models[b].t_single, f.models[b].t_double) for b in range(B)])
    f.admitted = np.array([is_admitted(f.com0[b, 2], f.models[b].t_single, f.models[b].t_double, bound) for b in range(B)])
    # ---- what the fleet is for ----
    assert f.admitted.any() and (~f.admitted).any()
    assert sorted(np.nonzero(~f.admitted)[0]) == sorted(list(BEYOND) + [b for b, (_, side) in ON_BOUND.items() if side == "out"])
    k = [int(x / LN2 + 0.5) for x in f.arg]                  # mo_exp's k of the largest argument
    assert sum(1 for b in range(B) if f.admitted[b] and f.arg[b] >= EXP_K_MIN_ARG and k[b] >= 16) >= 8
    assert all(k[b] >= 16 for b in range(B) if f.arg[b] >= EXP_K_MIN_ARG)
    near = np.abs(f.arg - bound) <= 1e-12 * bound
    assert (near & f.admitted).sum() >= 2 and (near & ~f.admitted).sum() >= 2
    assert f.arg[f.admitted].min() <= 8.01 and {f.route[b] for b in range(B) if f.admitted[b] and f.arg[b] > bound - 1.0} == set(ROUTES)
    assert f.arg.max() > 40.0                                # one gait beyond what cosh / sinh are made for, too
    return f


def without(f, drop):
    """the fleet f without the gaits `drop`: (fleet-like namespace with models, steps, n_steps, init_feet, com0, B, smax; kept indices)"""
    w = mf.wg()
    keep = [b for b in range(f.B) if b not in set(drop)]
    s = types.SimpleNamespace(B=len(keep), smax=f.smax, model=f.model)
    s.models = (w.MorisawaModel * len(keep))(*[f.models[b] for b in keep])
    s.steps = (w.RelStep * (len(keep) * f.smax))(*[f.steps[b * f.smax + i] for b in keep for i in range(f.smax)])
    s.n_steps = np.ascontiguousarray(f.n_steps[keep])
    s.init_feet, s.com0 = np.ascontiguousarray(f.init_feet[keep]), np.ascontiguousarray(f.com0[keep])
    return s, keep


def nearest_admitted(f, count=4):
    """the `count` admitted gaits whose argument is nearest the bound"""
    order = sorted((b for b in range(f.B) if f.admitted[b]), key=lambda b: (f.bound - f.arg[b], b))
    return order[:count]


def truth_samples(mo, f, b, t0, L, between=40):
    """gait b against the restatements on the clock t0 + k T: (ks, truth [len(ks), 18], float64 restatement [len(ks), 18], natures) --
    CoM x, dx, y, dy, ZMP x, y, left 6, right 6 -- at every sample where the interval changes, the last and about `between` others"""
    m = mf.model_dict(f.models[b])
    w64 = mo.Walk(mo.F64, m, *f.gait(b))
    truth = mo.Walk(mo.MP, m, *f.gait(b))
    clk = mo.clock(t0, m["T"], L)
    iv = [w64.interval(t) for t in clk]
    ks = sorted(set(list(range(0, L, max(1, L // between))) + [L - 1] + [k for k in range(1, L) if iv[k] != iv[k - 1]]))
    tv, v64, nat = [], [], []
    for k in ks:
        t, s = truth.sample(clk[k]), w64.sample(clk[k])
        tv.append([float(x) for x in t["com"] + t["zmp"] + t["left"] + t["right"]])
        v64.append(s["com"] + s["zmp"] + s["left"] + s["right"])
        nat.append((t["ltype"], t["rtype"]))
    return ks, np.array(tv), np.array(v64, float), nat


def sampled_columns(r, ks, b):
    """the same 18 columns of gait b from a sampler's outputs (numpy arrays, time-major)"""
    return np.array([list(r["com"][k, :, b]) + [r["zmp_x"][k, b], r["zmp_y"][k, b]] + list(r["left"][k, :, b]) + list(r["right"][k, :, b])
                     for k in ks])
