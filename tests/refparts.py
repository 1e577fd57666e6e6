"""Test infrastructure (no tests): the cases and the ctypes plumbing that hold the project's three restatements of the reference's
dependency-free files -- ComputeConvexHull::DoComputeConvexHull (ConvexHull.cpp), Polynome (Polynome.cpp) and Polynome3/4/5
(PolynomeFoot.cpp) -- to those files compiled: oracle/_ref/libwalkgen_parts_ref.so, entry points in oracle/ref_parts_shim.cpp.

Used by tests/test_ref_parts_oracle.py (CPU: compiled reference == oracle == host wg_foot_constraints), by
tests/golden/make_golden.py (records the cases the GPU tests use into tests/golden/ref_parts.npz) and by
tests/test_ref_parts_gpu.py (kernels against the record; needs neither the reference tree nor oracle/_ref/).

A stance is a double support (lx, ly, ltheta, rx, ry, rtheta), headings in degrees.  Its eight corners always come from the
oracle's probe wgo_probe_foot_corners, so they are the bits the oracle and the kernels feed their hulls."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np

import oraclelib as ol

wg = importlib.import_module("jrl-walkgen_amd")

SOLE = (0.24, 0.138, 0.02, 0.02)             # sole 0.24 x 0.138, margins 0.02 / 0.02 (tests/test_dimitrov_walk_gpu.py)
PSZ = C.sizeof(wg.ZmpPolytope)
GOLDEN = os.path.join(ol.ROOT, "tests", "golden", "ref_parts.npz")
FAMILIES = ("generic", "grid5", "same_heading", "aligned_equal_x", "quarter_turns", "x_offset_1e-9", "crossing", "one_ulp",
            "in_line", "nan_right_x")
FAMILY_SEED = 20251019

_vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
_pt = None


def ptrig():
    """the oracle built on include/wg_trig.h: the bit-exact partner of the host call and the kernels"""
    global _pt
    if _pt is None:
        ol.build_oracle()
        subprocess.check_call(["make", "-s", "-C", ol.ORACLE_DIR, "libwg_oracle_ptrig.so"])
        _pt = C.CDLL(os.path.join(ol.ORACLE_DIR, "libwg_oracle_ptrig.so"))
    return _pt


# ---- stances -------------------------------------------------------------------------------------------------------------------
def stances(family, n, seed=FAMILY_SEED):
    """n stances [n][6] of one family, from a fixed seed.  Every row is made from its own row of one uniform table, so the first
    rows of a longer call are the rows of a shorter one (the record holds the first rows of the CPU test's families)."""
    U = np.random.default_rng([seed, FAMILIES.index(family)]).random((n, 12))
    uni = lambda c, lo, hi: lo + (hi - lo) * U[:, c]  # noqa: E731
    pick = lambda c, k: np.minimum((U[:, c] * k).astype(np.int64), k - 1)  # noqa: E731  (0 .. k - 1)
    lx, rx = uni(0, -0.2, 0.3), uni(1, -0.2, 0.3)
    ly, ry = uni(2, 0.055, 0.135), uni(3, -0.135, -0.055)
    lt, rt = uni(4, -40, 40), uni(5, -40, 40)
    if family == "grid5":                                  # the same heading, a multiple of 5 degrees: 0, 90, 180 among them
        lt = rt = 5.0 * (pick(6, 73) - 36)
    elif family == "same_heading":
        lt = rt = uni(6, -180, 180)
    elif family == "aligned_equal_x":                      # four corners on one vertical line through the lowest point
        lt = rt = np.zeros(n)
        rx = lx
    elif family == "quarter_turns":                        # each foot on its own quarter turn, centres on a millimetre grid
        q = np.array([0.0, 90.0, 180.0, 270.0, -90.0])
        lt, rt = q[pick(6, 5)], q[pick(7, 5)]
        lx, ly, rx, ry = (np.round(a, 3) for a in (lx, ly, rx, ry))
    elif family == "x_offset_1e-9":                        # aligned, the feet a few nanometres apart in x
        lt = rt = np.zeros(n)
        rx = lx + 1e-9 * (pick(6, 7) - 3)
    elif family == "crossing":                             # soles that cross: hulls of 7 and 8
        lx, ly, rx, ry = (uni(c, -0.03, 0.03) for c in range(4))
        lt = uni(4, -10, 10)
        rt = lt + uni(5, 55, 95)
    elif family == "one_ulp":                              # x, y or the heading of the feet one ulp apart
        which = pick(6, 4)
        up = np.where(pick(7, 2) == 1, np.inf, -np.inf)
        aligned = pick(8, 2) == 1
        lt = np.where(aligned, 0.0, lt)
        rt = lt.copy()
        rx = np.where(which == 0, np.nextafter(lx, up), np.where(which == 3, rx, lx))
        rt = np.where(which == 1, np.nextafter(lt, up), rt)
        ry = np.where(which == 2, np.nextafter(ly - 0.19, up), ry)
        ry = np.where(which == 3, ly - 0.19, ry)           # exactly one nominal foot distance below, other x
    elif family == "in_line":
        # Feet in line, aligned, soles on one level: four corners tie for the lowest y, and the lowest point the reference keeps
        # (the first of them, the left sole's front corner) lies BETWEEN the others.  With the right foot one sole length ahead,
        # the left sole's rear corner and the right sole's front corner are in opposite directions at the same distance: the
        # cross product is zero, the distances are equal, and `<=` makes the later point replace the earlier one.  The only
        # stances at which `distance1 <= distance2` differs from `<` (same direction and equal distance is a duplicate point).
        lt = rt = np.zeros(n)
        ry = ly
        hw = SOLE[0] * 0.5 - SOLE[2]
        rx = np.where(pick(6, 4) > 0, lx + 2.0 * hw, lx + uni(7, 0.0, 0.5))
    elif family == "nan_right_x":
        # The left foot below, the x of the right foot above it NaN: every cross product with the right sole's corners is NaN,
        # neither zero nor positive, so the erase loop passes them and the std::set finds each equivalent to the element it is
        # compared with and refuses it.  The only way to that refusal: between finite points "equivalent" coincides with a zero
        # cross product, which the erase loop has settled before.  (The finite corners come first, so three candidates are in
        # the set by then; with the NaN corners first the reference would keep one candidate and read past its list's end.)
        ly, ry = ry, ly
        rx = np.full(n, np.nan)
    else:
        assert family == "generic"
    return np.ascontiguousarray(np.stack([lx, ly, lt, rx, ry, rt], axis=1), dtype=np.float64)


def corners(lib, st, sole=SOLE):
    """the eight corners [n][8][2] of stances [n][6], by the oracle lib's probe: left foot 0..3, right foot 4..7"""
    st = np.ascontiguousarray(st, dtype=np.float64)
    xy = np.zeros((st.shape[0], 8, 2))
    lib.wgo_probe_foot_corners.argtypes = [C.c_int, C.c_void_p] + [C.c_double] * 4 + [C.c_void_p]
    lib.wgo_probe_foot_corners.restype = None
    lib.wgo_probe_foot_corners(2 * st.shape[0], _vp(st), *sole, _vp(xy))
    return xy


def _hull(fn, xy):
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    n, npts = xy.shape[:2]
    hull = np.full((n, npts + 1, 2), np.nan)
    count = np.full(n, -99, np.int32)
    fn.argtypes, fn.restype = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p], C.c_int
    assert fn(n, npts, _vp(xy), _vp(hull), _vp(count)) == 0
    return hull, count


def oracle_hull(lib, xy):
    """convex_hull of oracle/zmpdisc_oracle.c on point sets [n][npts][2]: (hull [n][npts + 1][2], count [n])"""
    return _hull(lib.wgo_probe_convex_hull, xy)


def ref_hull(xy):
    """ComputeConvexHull::DoComputeConvexHull, compiled, on the same sets"""
    return _hull(ol.ref_parts().wgr_convex_hull, xy)


def polytopes(lib, hull, count):
    """linear_system of oracle/zmpdisc_oracle.c on hulls [n][stride][2]: ((ZmpPolytope * n), rc [n])"""
    hull = np.ascontiguousarray(hull, dtype=np.float64)
    count = np.ascontiguousarray(count, dtype=np.int32)
    n = hull.shape[0]
    P = (wg.ZmpPolytope * n)()
    rc = np.full(n, -99, np.int32)
    lib.wgo_probe_linear_system.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.wgo_probe_linear_system.restype = None
    lib.wgo_probe_linear_system(n, hull.shape[1], _vp(hull), _vp(count), C.addressof(P), _vp(rc))
    return P, rc


def tie_counts(xy):
    """per point set: (a lowest-y tie, an exactly zero cross product about the lowest point between two other points that are
    not the lowest point's copies), in the arithmetic of ConvexHull.cpp:40-49 (numpy float64, no contraction)"""
    y = xy[:, :, 1]
    i0 = np.argmin(y, axis=1)                                  # the first of the lowest, as `<` keeps it
    tie = (y == y.min(axis=1, keepdims=True)).sum(axis=1) >= 2
    p0 = xy[np.arange(xy.shape[0]), i0]
    d = xy - p0[:, None, :]
    cr = d[:, :, None, 0] * d[:, None, :, 1] - d[:, None, :, 0] * d[:, :, None, 1]
    away = (d != 0.0).any(axis=2)
    pair = away[:, :, None] & away[:, None, :] & ~np.eye(xy.shape[1], dtype=bool)[None]
    return tie, ((cr == 0.0) & pair).any(axis=(1, 2))


def stance_trajectory(st, lift=0.03, T=0.005):
    """(time, left [2n][6], left_type, right) whose sample 2k is stance k as a double support by its step type (>= 10) and whose
    sample 2k + 1 lifts the left foot: every stance opens a new polytope, polytope 2k of the queue"""
    n = st.shape[0]
    left, right = np.zeros((2 * n, 6)), np.zeros((2 * n, 6))
    left[:, [0, 1, 3]] = np.repeat(st[:, 0:3], 2, axis=0)
    right[:, [0, 1, 3]] = np.repeat(st[:, 3:6], 2, axis=0)
    left[1::2, 2] = lift
    lt = np.zeros(2 * n, np.int32)
    lt[0::2] = 11
    return np.arange(2 * n) * T, left, lt, right


# ---- polynomials ---------------------------------------------------------------------------------------------------------------
NT = 4                                                     # times per parameter set


def poly_cases(n, seed):
    """n parameter sets (FT, FP, p0, v0, a0) and NT times each: random, with FT = 0, FP = 0 (the middle position of degree 4),
    zero initial conditions, t = 0 and t = FT mixed in"""
    rng = np.random.default_rng(seed)
    FT = rng.uniform(0.05, 2.0, n)
    FP = rng.normal(0, 0.3, n)
    p0, v0, a0 = rng.normal(0, 0.2, n), rng.normal(0, 0.5, n), rng.normal(0, 2.0, n)
    FT[rng.random(n) < 0.02] = 0.0
    FP[rng.random(n) < 0.05] = 0.0
    for a in (p0, v0, a0):
        a[rng.random(n) < 0.05] = 0.0
    t = rng.uniform(0.0, 1.0, (n, NT)) * FT[:, None]
    t[:, 0] = 0.0
    t[:, 1] = FT
    t[:, 3] = rng.uniform(-0.1, 2.5, n)                        # anywhere, past FT included
    return dict(FT=FT, FP=FP, p0=p0, v0=v0, a0=a0, t=np.ascontiguousarray(t))


def _poly(fn, degree, c, init, derivs):
    n = c["FT"].shape[0]
    out = [np.full((n, NT), np.nan) for _ in range(3 if derivs else 1)]
    par = [_vp(c["FT"]), _vp(c["FP"])] + ([_vp(c["p0"]), _vp(c["v0"]), _vp(c["a0"])] if init else [])
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * len(par) + [C.c_int, C.c_void_p] + [C.c_void_p] * len(out)
    assert fn(degree, n, *par, NT, _vp(c["t"]), *[_vp(o) for o in out]) == 0
    return out


def oracle_zd_poly(lib, degree, c):
    """zmpdisc_oracle.c: poly<degree>_set(FT, FP), poly_eval -> [value [n][NT]]"""
    return _poly(lib.wgo_probe_zd_poly, degree, c, init=False, derivs=False)


def oracle_tick_poly(lib, degree, c):
    """herdt_oracle.c: the tick's set forms, poly_eval / poly_d1 / poly_d2 -> [value, d1, d2]"""
    return _poly(lib.wgo_probe_tick_poly, degree, c, init=True, derivs=True)


def ref_poly_plain(degree, c):
    """Polynome<degree>(FT, FP).Compute, compiled -> [value]"""
    fn = ol.ref_parts().wgr_poly_plain
    n = c["FT"].shape[0]
    val = np.full((n, NT), np.nan)
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert fn(degree, n, _vp(c["FT"]), _vp(c["FP"]), NT, _vp(c["t"]), _vp(val), None, None) == 0
    return [val]


def ref_poly_init(degree, c):
    """the compiled classes set as the tick sets them, Compute / ComputeDerivative / ComputeSecDerivative -> [value, d1, d2]"""
    return _poly(ol.ref_parts().wgr_poly_init, degree, c, init=True, derivs=True)


def ref_swing_z(t_single, step_height, T, kmax):
    """Polynome4(t_single, step_height).Compute(k * T), k = 0 .. kmax, compiled; k * T as the feet queue forms it (k converted
    to double, one product)"""
    fn = ol.ref_parts().wgr_poly_plain
    t = np.ascontiguousarray(np.arange(kmax + 1, dtype=np.float64) * T)
    val = np.full(kmax + 1, np.nan)
    FT, FP = np.array([float(t_single)]), np.array([float(step_height)])
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert fn(4, 1, _vp(FT), _vp(FP), kmax + 1, _vp(t), _vp(val), None, None) == 0
    return val


# ---- the swing foot of a ZMPDiscretization run -----------------------------------------------------------------------------------
SWING_MODELS = ((0.005, 0.78, 0.07), (0.01, 0.7, 0.05), (0.004, 0.9, 0.1))    # (T, t_single, step_height)


def swing_samples(foot_type):
    """from one foot's stepType column: (indices of the samples this foot swings at, k of each) with k counted from the last
    sample before the swing (a double support: type >= 10).  The swinging foot carries the step's type, 1 .. 9; the support
    foot its negative."""
    ty = np.asarray(foot_type)
    sw = (ty > 0) & (ty < 10)
    idx = np.flatnonzero(sw)
    start = np.flatnonzero(sw & ~np.concatenate([[False], sw[:-1]]))       # first sample of each swing
    k = idx - (start[np.searchsorted(start, idx, side="right") - 1] - 1)
    return idx, k


# ---- the fleet of tests/test_ref_parts_gpu.py: stances from the record, dealt round-robin ------------------------------------------
CH = 64                                                    # wg_foot_constraints_chunk(); the GPU test asserts it
FLEET_B = 70                                               # one full wave and a part of a second
FLEET_LONGEST = 37                                         # the gait whose trajectory spans more than one block of the time axis
FLEET_QCAP = 128
FILL_B, FILL_D, FILL_I = 0xA5, -7.25, -77                  # what the outputs hold before a launch (tests/test_dimitrov_walk_gpu.py)
FLEET_T = 0.005


def fleet_lengths():
    """samples per gait: ragged, 3 .. 12, odd lengths (a last stance nothing follows) among them; one gait of CH + 48"""
    lens = np.array([3 + (7 * b) % 10 for b in range(FLEET_B)], np.int32)
    lens[FLEET_LONGEST] = CH + 48
    return lens


def fleet_deal():
    """(per gait: the list of (family index, row) of its stances; rows needed per family).  Stance s of a gait is its sample 2 s.
    Dealt stance-major over the gaits that have a stance s, so at every sample the lanes of a wave carry the families in turn."""
    lens = fleet_lengths()
    n_st = (lens + 1) // 2
    deal, used, g = [[] for _ in range(FLEET_B)], [0] * len(FAMILIES), 0
    for s in range(int(n_st.max())):
        for b in range(FLEET_B):
            if s < n_st[b]:
                f = g % len(FAMILIES)
                deal[b].append((f, used[f]))
                used[f] += 1
                g += 1
    return deal, max(used)


def fleet_trajectories(gold):
    """(time [lcap], left [lcap][6][B], left_type [lcap][B], right [lcap][6][B], lens) from the recorded stances; past a gait's
    length NaN feet and a step type that reads as double support, which nothing may read"""
    lens = fleet_lengths()
    lcap = int(lens.max())
    deal, _ = fleet_deal()
    left, right = np.full((lcap, 6, FLEET_B), np.nan), np.full((lcap, 6, FLEET_B), np.nan)
    lty = np.full((lcap, FLEET_B), 1 << 30, np.int32)
    st = gold["hull_stances"]
    for b in range(FLEET_B):
        rows = np.array([gold_row(gold, f, r) for f, r in deal[b]])
        _, l, t, r = stance_trajectory(st[rows])
        L = int(lens[b])
        left[:L, :, b], right[:L, :, b], lty[:L, b] = l[:L], r[:L], t[:L]
    return np.arange(lcap) * FLEET_T, left, lty, right, lens


def gold_row(gold, family, row):
    """index of row `row` of family `family` in the record (families are stored one after the other, equally many rows each)"""
    per = gold["hull_stances"].shape[0] // len(FAMILIES)
    assert row < per and gold["hull_family"][family * per + row] == family
    return family * per + row


_expect_cache = {}


def fleet_expectation(gold, lens=None):
    """what the queues must hold after the feet up to lens[b] (default: the whole trajectories): (queue bytes [B][QCAP * PSZ],
    t_start [B][QCAP], t_end, count [B]), untouched entries at their pre-fill.  Entry 2 s of a gait is the wg_trig.h oracle's
    linear_system of the RECORDED reference hull of stance s, entry 2 s + 1 that of the right sole's corners (by the oracle's
    corner probe), the intervals the sample times."""
    full = fleet_lengths()
    lens = full if lens is None else np.minimum(np.asarray(lens, np.int32), full)
    lib = ptrig()
    if "polys" not in _expect_cache:
        deal, _ = fleet_deal()
        st = gold["hull_stances"]
        per_gait = []
        for b in range(FLEET_B):
            rows = np.array([gold_row(gold, f, r) for f, r in deal[b]])
            xy = corners(lib, st[rows])
            assert ol.same_bits_nan_aware(xy, gold["hull_corners"][rows]), "the record is of other corners: regenerate it"
            ds, rc1 = polytopes(lib, gold["hull_vertices"][rows], gold["hull_count"][rows])
            ss, rc2 = polytopes(lib, xy[:, 4:8], np.full(len(rows), 4, np.int32))
            assert (rc1 == 0).all() and (rc2 == 0).all()
            q = np.empty((2 * len(rows), PSZ), np.uint8)
            q[0::2] = np.frombuffer(ds, np.uint8).reshape(-1, PSZ)
            q[1::2] = np.frombuffer(ss, np.uint8).reshape(-1, PSZ)
            per_gait.append(q)
        _expect_cache["polys"] = per_gait
    time = np.arange(int(full.max())) * FLEET_T
    Q = np.full((FLEET_B, FLEET_QCAP, PSZ), FILL_B, np.uint8)
    ts, te = np.full((FLEET_B, FLEET_QCAP), FILL_D), np.full((FLEET_B, FLEET_QCAP), FILL_D)
    count = np.full(FLEET_B, FILL_I, np.int32)
    for b in range(FLEET_B):
        L = int(lens[b])
        if L <= 0:
            continue
        Q[b, :L] = _expect_cache["polys"][b][:L]
        ts[b, :L] = time[:L]
        te[b, :L - 1] = time[1:L]
        te[b, L - 1] = time[L - 1]
        count[b] = L
    return Q.reshape(FLEET_B, -1), ts, te, count


# ---- the fleets of the swing-height test ---------------------------------------------------------------------------------------
SWING_SMAX = 5


def swing_fleet(i):
    """(model, steps, n_steps, init) of model i of SWING_MODELS: FLEET_B random step sequences (tests/test_zmpdisc_gpu.py's
    random_fleet: own support times, obstacle step types), omega = 0, feet that start on the ground"""
    from test_zmpdisc_gpu import random_fleet
    from test_zmpdisc_oracle import kajita_model
    zm = kajita_model()
    zm.T, zm.t_single, zm.step_height = SWING_MODELS[i]
    zm.omega = 0.0
    return (zm,) + random_fleet(np.random.default_rng(4100 + i), FLEET_B, SWING_SMAX, zm)


_swing_cache = {}


def swing_expectation(gold, i):
    """per gait of swing_fleet(i): (length, expected z column of the left foot, of the right foot), and the number of airborne
    samples in all.  While a foot swings its z is the RECORDED Polynome4(t_single, step_height).Compute(k T), k counted from the
    last grounded sample before the swing; a last swing shorter than t_single ends in the air and the end phase holds that
    height (k stays); everywhere else z = 0.  Which foot swings when comes from the wg_trig.h oracle's run of the fleet, and
    the columns are asserted on that run, bit for bit, before anything else uses them."""
    if i not in _swing_cache:
        from test_zmpdisc_gpu import gait_steps
        zm, steps, n_steps, init = swing_fleet(i)
        assert tuple(gold["swing_models"][i]) == (zm.T, zm.t_single, zm.step_height)
        zrec = gold["swing_z_%d" % i]
        res, airborne, held = [], 0, 0
        for b in range(FLEET_B):
            o = ol.zmpdisc(zm, gait_steps(steps, b, SWING_SMAX, int(n_steps[b])), init[b], lib=ptrig())
            cols = []
            for key in ("left", "right"):
                ty = o[key + "_type"]
                ix, k = swing_samples(ty)
                want = np.zeros(o["length"])
                if ix.size:                                    # a walk of two steps swings one foot only
                    assert k.min() == 1 and k.max() < zrec.shape[0]
                    want[ix] = zrec[k]
                    j = ix[-1] + 1
                    while j < o["length"] and ty[j] == 0:      # the end phase right after the last swing
                        want[j] = zrec[k[-1]]
                        j += 1
                    held += int(j - ix[-1] - 1) * int(zrec[k[-1]] > 0)
                assert ol.same_bits(o[key][:, 2], want), (i, b, key)
                airborne += int((want > 0).sum())
                cols.append(want)
            res.append((o["length"], cols[0], cols[1]))
        _swing_cache[i] = (res, airborne, held)
    return _swing_cache[i]
