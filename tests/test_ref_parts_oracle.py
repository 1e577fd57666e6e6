"""The project's restatements of the reference's dependency-free files, held to those files COMPILED, on the CPU, bit for bit.

  hull         ComputeConvexHull::DoComputeConvexHull (src/Mathematics/ConvexHull.cpp, a std::set ordered by the sign of a rounded
               cross product, with its "same direction, keep the farther" erase loop)
                 == convex_hull of oracle/zmpdisc_oracle.c, both trigonometry builds
                 == fc_hull8 of csrc/wg_footcons_geom.hpp through the host wg_foot_constraints (the kernels compile the same text;
                    tests/test_ref_parts_gpu.py runs them)
  polynomials  Polynome::Compute / ComputeDerivative / ComputeSecDerivative on Polynome3 / 4 / 5 (Polynome.cpp, PolynomeFoot.cpp)
                 == poly_eval, poly3/4/5_set of oracle/zmpdisc_oracle.c (the feet queue: plain forms, value)
                 == poly_eval, poly_d1, poly_d2, poly3/4/5_set of oracle/herdt_oracle.c (the tick: initial-condition forms, nine
                    values per case)

The compiled reference is oracle/_ref/libwalkgen_parts_ref.so (oracle/Makefile, target `ref`; entry points: oracle/ref_parts_shim.cpp).
It exists where the reference tree was present at build time; elsewhere these tests skip and tests/test_ref_parts_gpu.py still
holds the kernels to what tests/golden/make_golden.py recorded from it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oraclelib as ol  # noqa: E402
import refparts as rp  # noqa: E402

wg = rp.wg
needs_ref = pytest.mark.skipif(not ol.have_ref_parts(), reason="oracle/_ref/libwalkgen_parts_ref.so is built from the reference tree")

N_STANCES = 20000                               # per family
N_POLY = 100000                                 # parameter sets per form, rp.NT times each

_cases = {}


def family_case(family):
    """one family's stances, their corners by the wg_trig.h oracle and the compiled reference's hulls of them, computed once"""
    if family not in _cases:
        st = rp.stances(family, N_STANCES)
        xy = rp.corners(rp.ptrig(), st)
        hull, count = rp.ref_hull(xy)
        _cases[family] = dict(st=st, xy=xy, hull=hull, count=count)
    return _cases[family]


# ---- hull ----------------------------------------------------------------------------------------------------------------------
@needs_ref
def test_hull_cases_meet_their_preconditions():
    """what keeps the hull pin from being vacuous, from the inputs and the compiled reference's output alone"""
    sizes, ties, zeros = {}, 0, 0
    for fam in rp.FAMILIES:
        c = family_case(fam)
        assert c["st"].shape == (N_STANCES, 6) and (c["count"] >= 3).all() and (c["count"] <= 8).all(), fam
        tie, zero = rp.tie_counts(c["xy"])
        u, n = np.unique(c["count"], return_counts=True)
        print("%-16s hull sizes %s, lowest-y ties %d, zero cross products about the lowest point %d"
              % (fam, dict(zip(u.tolist(), n.tolist())), tie.sum(), zero.sum()))
        for k, v in zip(u.tolist(), n.tolist()):
            sizes[k] = sizes.get(k, 0) + v
        ties += int(tie.sum()); zeros += int(zero.sum())
    print("all families: sizes %s, ties %d, zero cross products %d" % (sizes, ties, zeros))
    assert {4, 5, 6, 7, 8} <= set(sizes)
    assert zeros >= 1000 and ties >= 1000
    assert len(_cases) == len(rp.FAMILIES) == 10


@needs_ref
@pytest.mark.parametrize("family", rp.FAMILIES)
def test_oracle_hull_is_the_compiled_reference(family):
    """vertex count and every coordinate bit; on the corners of either trigonometry build"""
    c = family_case(family)
    for lib, xy, want in ((rp.ptrig(), c["xy"], (c["hull"], c["count"])), (ol.oracle(), rp.corners(ol.oracle(), c["st"]), None)):
        hull, count = rp.oracle_hull(lib, xy)
        rh, rc = want or rp.ref_hull(xy)
        bad = np.flatnonzero((count != rc) | (hull.view(np.uint64) != rh.view(np.uint64)).any(axis=(1, 2)))
        assert bad.size == 0, (family, bad.size, bad[:5], c["st"][bad[:1]])


@needs_ref
@pytest.mark.parametrize("family", rp.FAMILIES)
def test_host_foot_constraints_build_the_polytope_of_the_reference_hull(family):
    """wg_foot_constraints (fc_hull8, fc_polytope) on a trajectory whose sample 2k is stance k: polytope 2k of its queue is the
    oracle's linear_system of the REFERENCE's hull -- nrows, A, B, centre, similar, every byte of the struct"""
    c = family_case(family)
    want, rc = rp.polytopes(rp.ptrig(), c["hull"][:, :8], c["count"])
    assert (rc == 0).all()
    time, left, lt, right = rp.stance_trajectory(c["st"])
    n = time.shape[0]
    polys = (wg.ZmpPolytope * n)(); ts = np.zeros(n); te = np.zeros(n)
    fn = wg.lib().wg_foot_constraints
    fn.argtypes, fn.restype = [C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_int] + [C.c_void_p] * 3, C.c_int
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert fn(n, vp(time), vp(left), vp(lt), vp(right), *rp.SOLE, n, C.addressof(polys), vp(ts), vp(te)) == n
    assert np.array_equal(ts, time)                                      # every sample opened a polytope
    got = np.frombuffer(polys, dtype=np.uint8).reshape(n, rp.PSZ)[0::2]
    exp = np.frombuffer(want, dtype=np.uint8).reshape(N_STANCES, rp.PSZ)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, (family, bad.size, bad[:5], c["st"][bad[:1]])
    assert polys[0].nrows == c["count"][0]


# ---- polynomials ---------------------------------------------------------------------------------------------------------------
def _edges(c):
    """the edge values the cases must hold"""
    assert c["FT"].shape[0] >= 100000
    assert (c["FT"] == 0).sum() > 100 and (c["FP"] == 0).sum() > 100 and ((c["FT"] != 0) & (c["FP"] != 0)).sum() > 50000
    assert (c["t"][:, 0] == 0).all() and (c["t"][:, 1] == c["FT"]).all() and (c["t"][:, 3] > c["FT"]).any()


@needs_ref
@pytest.mark.parametrize("build", ["libm", "wg_trig"])
@pytest.mark.parametrize("degree", [3, 4, 5])
def test_feet_queue_polynomials_are_the_compiled_classes(degree, build):
    """poly<degree>_set(FT, FP) + poly_eval of zmpdisc_oracle.c == Polynome<degree>(FT, FP).Compute: value"""
    c = rp.poly_cases(N_POLY, 7000 + degree)
    _edges(c)
    got = rp.oracle_zd_poly(ol.oracle() if build == "libm" else rp.ptrig(), degree, c)[0]
    want = rp.ref_poly_plain(degree, c)[0]
    assert np.isfinite(want).all()
    assert ol.same_bits(got, want), degree


@needs_ref
@pytest.mark.parametrize("build", ["libm", "wg_trig"])
@pytest.mark.parametrize("degree", [3, 4, 5])
def test_tick_polynomials_are_the_compiled_classes(degree, build):
    """the tick's set forms + poly_eval / poly_d1 / poly_d2 of herdt_oracle.c == Polynome3::SetParametersWithInitPosInitSpeed,
    Polynome4::SetParameters, Polynome5::SetParameters(FT, FP, p0, v0, a0) + Compute / ComputeDerivative / ComputeSecDerivative.
    Degree 5 divides by FT unguarded, there as here: FT = 0 gives infinities and NaNs, which must match as such."""
    c = rp.poly_cases(N_POLY, 7100 + degree)
    _edges(c)
    got = rp.oracle_tick_poly(ol.oracle() if build == "libm" else rp.ptrig(), degree, c)
    want = rp.ref_poly_init(degree, c)
    finite = np.isfinite(want[0])
    assert finite[c["FT"] != 0].all() and (degree == 5 or finite.all())
    for what, g, w in zip(("value", "first derivative", "second derivative"), got, want):
        assert ol.same_bits_nan_aware(g, w), (degree, what)
        assert np.abs(w[finite]).max() > 0


@needs_ref
@pytest.mark.parametrize("T,t_single,step_height", rp.SWING_MODELS)
def test_recorded_swing_heights_are_the_compiled_polynomial(T, t_single, step_height):
    """tests/golden/ref_parts.npz holds what the compiled reference gives today"""
    g = np.load(rp.GOLDEN)
    i = [tuple(m) for m in g["swing_models"].tolist()].index((T, t_single, step_height))
    z = g["swing_z_%d" % i]
    assert ol.same_bits(z, rp.ref_swing_z(t_single, step_height, T, z.shape[0] - 1))


@needs_ref
def test_recorded_hulls_are_the_compiled_reference():
    g = np.load(rp.GOLDEN)
    hull, count = rp.ref_hull(g["hull_corners"])
    assert np.array_equal(count, g["hull_count"]) and ol.same_bits(hull[:, :8], g["hull_vertices"])


# ---- the record alone: what tests/test_ref_parts_gpu.py expects, first held to the CPU side (runs without oracle/_ref/) ------------
def gold():
    return np.load(rp.GOLDEN)


def test_recorded_hull_cases_meet_their_preconditions():
    g = gold()
    _, per = rp.fleet_deal()
    assert list(g["families"]) == list(rp.FAMILIES) and g["hull_stances"].shape == (per * len(rp.FAMILIES), 6)
    assert np.array_equal(g["hull_family"], np.repeat(np.arange(len(rp.FAMILIES)), per))          # every family contributes
    for f, fam in enumerate(rp.FAMILIES):                                  # the rows are the first of the CPU test's families
        assert ol.same_bits_nan_aware(g["hull_stances"][f * per:(f + 1) * per], rp.stances(fam, N_STANCES)[:per]), fam
    tie, zero = rp.tie_counts(g["hull_corners"])
    xy = g["hull_corners"][g["hull_family"] == rp.FAMILIES.index("in_line")]
    replaced = (xy[:, 7] == xy[:, 0]).all(axis=1) & (np.abs(xy[:, 3, 0] - xy[:, 0, 0]) == np.abs(xy[:, 4, 0] - xy[:, 0, 0]))
    print("recorded: hull sizes %s, lowest-y ties %d, zero cross products %d, in-line stances with equal opposite distances %d"
          % (np.unique(g["hull_count"], return_counts=True), tie.sum(), zero.sum(), replaced.sum()))
    assert set(g["hull_count"].tolist()) == {4, 5, 6, 7, 8}
    assert tie.sum() >= 20 and zero.sum() >= 20 and replaced.sum() >= 5
    assert np.isnan(g["hull_stances"][g["hull_family"] == rp.FAMILIES.index("nan_right_x"), 3]).all()
    lens = rp.fleet_lengths()
    assert lens.max() == rp.CH + 48 and len(set(lens.tolist())) >= 8 and (lens % 2 == 1).any() and lens.max() <= rp.FLEET_QCAP


def _queue_of(fn, time, left, lt, right):
    """fn = w*_foot_constraints on pre-filled outputs of FLEET_QCAP entries: (bytes, t_start, t_end, return value)"""
    fn.argtypes, fn.restype = [C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_int] + [C.c_void_p] * 3, C.c_int
    cap = rp.FLEET_QCAP
    polys = (wg.ZmpPolytope * cap)(); C.memset(polys, rp.FILL_B, C.sizeof(polys))
    ts, te = np.full(cap, rp.FILL_D), np.full(cap, rp.FILL_D)
    time, left, right = (np.ascontiguousarray(a, dtype=np.float64) for a in (time, left, right))
    lt = np.ascontiguousarray(lt, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = fn(len(time), vp(time), vp(left), vp(lt), vp(right), *rp.SOLE, cap, C.addressof(polys), vp(ts), vp(te))
    return bytes(polys), ts, te, k


@pytest.mark.parametrize("cut", [None, rp.CH, rp.CH + 1])
def test_recorded_fleet_expectation_is_the_oracles_and_the_hosts_queue(cut):
    """the queues built from the recorded reference hulls are what wgo_foot_constraints (wg_trig.h build) and the host
    wg_foot_constraints give on the fleet's trajectories, whole and cut where the on-line test cuts them"""
    g = gold()
    time, left, lty, right, lens = rp.fleet_trajectories(g)
    if cut is not None:
        lens = np.minimum(lens, cut)
    Q, ts, te, count = rp.fleet_expectation(g, lens)
    for b in range(rp.FLEET_B):
        L = int(lens[b])
        for fn in (rp.ptrig().wgo_foot_constraints, wg.lib().wg_foot_constraints):
            pb, t0, t1, k = _queue_of(fn, time[:L], left[:L, :, b], lty[:L, b], right[:L, :, b])
            assert k == count[b] == L, (b, k)
            assert pb == Q[b].tobytes() and t0.tobytes() == ts[b].tobytes() and t1.tobytes() == te[b].tobytes(), b


@pytest.mark.parametrize("i", range(len(rp.SWING_MODELS)))
def test_swing_heights_of_the_oracle_are_the_recorded_polynomial(i):
    """every z of either foot over FLEET_B random walks: Polynome4(t_single, step_height).Compute(k T) as the compiled reference
    gave it (asserted inside swing_expectation), with thousands of airborne samples and last swings that end in the air"""
    res, airborne, held = rp.swing_expectation(gold(), i)
    print("model %s: %d airborne samples, %d of them held by the end phase" % (rp.SWING_MODELS[i], airborne, held))
    assert len(res) == rp.FLEET_B and airborne > 10000 and held > 0
