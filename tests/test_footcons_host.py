"""The host wg_foot_constraints (csrc/wg_footcons.cpp over csrc/wg_footcons_geom.hpp, the geometry the kernels compile too) held
to oracle/zmpdisc_oracle.c's wgo_foot_constraints of the wg_trig.h build, on the CPU: byte for byte over the polytopes, t_start,
t_end and the return value.  Both sides write into buffers two entries longer than the capacity they are given, pre-filled
alike, and the whole buffers are compared: what a call leaves untouched -- past the count, past the capacity -- is part of it.

Cases: every gait of fleet70() (the feet are the oracle's own, the inputs of test_dimitrov_walk_gpu's precondition test) at
cap = QCAP, at cap = 3 (the queues of all but the shortest walks overflow) and at cap = 0; the hand-made support codes of test_footcons_online_gpu (a z
exactly at the lifting threshold: samples that inherit, chains of them); a double support whose eight corners are collinear,
which is no polytope; crossing soles (8 rows); n = 0."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_zmpdisc_gpu import ptrig  # noqa: E402
from test_dimitrov_walk_gpu import BF, FILL_B, FILL_D, QCAP, SOLE, fleet70, oracle_queues, times  # noqa: E402
from test_footcons_online_gpu import hand_made_gaits  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")

BAD = -2                                       # WG_ERR_BAD_ARG
LIFTING = 0.00001
ARGTYPES = [C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_int] + [C.c_void_p] * 3


def call(fn, time, left, left_type, right, cap, sole=SOLE):
    """fn(n, ..., cap, ...) on pre-filled buffers of cap + 2 entries: (polytope bytes, t_start bytes, t_end bytes, return value)"""
    fn.argtypes, fn.restype = ARGTYPES, C.c_int
    polys = (wg.ZmpPolytope * (cap + 2))(); C.memset(polys, FILL_B, C.sizeof(polys))
    ts = np.full(cap + 2, FILL_D); te = np.full(cap + 2, FILL_D)
    time, left, right = (np.ascontiguousarray(a, dtype=np.float64) for a in (time, left, right))
    lt = np.ascontiguousarray(left_type, dtype=np.int32)
    assert left.shape == right.shape == (len(time), 6) and lt.shape == (len(time),)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = fn(len(time), vp(time), vp(left), vp(lt), vp(right), *sole, cap, C.addressof(polys), vp(ts), vp(te))
    return bytes(polys), ts.tobytes(), te.tobytes(), k


def both(gait, cap, sole=SOLE):
    return call(ptrig().wgo_foot_constraints, *gait, cap, sole), call(wg.lib().wg_foot_constraints, *gait, cap, sole)


def fleet_gaits():
    """(time, left, left_type, right) of every gait of fleet70(), feet from the oracle"""
    zm = fleet70()[0]
    return [(times(o["length"], zm.T), o["left"], o["left_type"], o["right"]) for o, _ in oracle_queues("t1", fleet70())]


def hand_gaits():
    B, lcap, _, lf, rf, lty = hand_made_gaits()
    return [(times(lcap, 0.005), lf[:, :, b], lty[:, b], rf[:, :, b]) for b in range(B)]


def crossed_gait():
    """Soles that cross (headings 80 or 65 degrees apart, centres a few centimetres apart): double supports whose hull keeps all
    eight corners -- no walk of fleet70() has more than 6 rows.  Double support, left foot in the air, double support."""
    n = 12
    left, right = np.zeros((n, 6)), np.zeros((n, 6))
    left[:, :4] = [0.0, 0.02, 0.0, 0.0]; right[:, :4] = [0.0, -0.02, 0.0, 90.0]
    left[4:8, 2] = 0.03
    left[8:, :4] = [0.0, 0.03, 0.0, 5.0]; right[8:, :4] = [0.02, -0.03, 0.0, 70.0]
    return times(n, 0.005), left, np.zeros(n, np.int32), right


def inherits(gait):
    """samples none of the reference's three tests holds for"""
    _, left, lt, right = gait
    lz, rz = np.asarray(left)[:, 2], np.asarray(right)[:, 2]
    return (np.asarray(lt) < 10) & ~(lz > LIFTING) & ~(rz > LIFTING) & ~((rz < LIFTING) & (lz < LIFTING))


def test_cases_meet_their_preconditions_on_the_oracle():
    """what the comparisons below must have covered, from the inputs and the oracle's output alone"""
    ds_rows, rows, sims, inheriting, longest_chain = set(), set(), set(), 0, 0
    for gait in fleet_gaits() + hand_gaits() + [crossed_gait()]:
        pb, tsb, _, k = call(ptrig().wgo_foot_constraints, *gait, QCAP)
        assert 1 <= k <= QCAP
        P, ts = (wg.ZmpPolytope * (QCAP + 2)).from_buffer_copy(pb), np.frombuffer(tsb)
        t64, l64, lt32, r64 = (np.asarray(a) for a in gait)
        inh = inherits(gait)
        inheriting += int(inh.sum())
        run = 0
        for v in inh:
            run = run + 1 if v else 0
            longest_chain = max(longest_chain, run)
        for q in range(k):
            i = int(np.searchsorted(t64, ts[q]))
            assert t64[i] == ts[q]
            rows.add(P[q].nrows)
            sims.update(P[q].similar[j] for j in range(P[q].nrows))
            if lt32[i] >= 10 or (l64[i, 2] < LIFTING and r64[i, 2] < LIFTING):
                ds_rows.add(P[q].nrows)
    print("rows %s (double supports %s), similar %s, %d inheriting samples, longest chain %d"
          % (sorted(rows), sorted(ds_rows), sorted(sims), inheriting, longest_chain))
    assert 4 in ds_rows and 6 in rows and max(rows) > 6
    assert sims - {0}
    assert inheriting > 0 and longest_chain >= 3


@pytest.mark.parametrize("cap", [QCAP, 3, 0])
def test_fleet_matches_the_oracle(cap):
    gaits = fleet_gaits()
    assert len(gaits) == BF
    overflows = 0
    for b, gait in enumerate(gaits):
        ref, got = both(gait, cap)
        assert got[3] == ref[3], (b, got[3], ref[3])
        for what, r, g in zip(("polytopes", "t_start", "t_end"), ref, got):
            assert g == r, (b, cap, what)
        overflows += ref[3] > cap
    print("cap %d: %d of %d queues overflow" % (cap, overflows, BF))
    assert overflows == {QCAP: 0, 0: BF}[cap] if cap != 3 else 0 < overflows <= BF


@pytest.mark.parametrize("cap", [QCAP, 1])
def test_hand_made_support_codes_match_the_oracle(cap):
    for b, gait in enumerate(hand_gaits() + [crossed_gait()]):
        assert inherits(gait).any() == (b == 0)               # gait 0 holds the chain of inheriting samples
        ref, got = both(gait, cap)
        assert ref[3] >= 3 and got == ref, (b, cap)


@pytest.mark.parametrize("cap", [QCAP, 0])
def test_collinear_double_support_is_refused(cap):
    """half height zero, both feet at the same y, heading 0: all eight corners on one line, fewer than two directions about the
    lowest point.  The oracle's -1 is the host's WG_ERR_BAD_ARG; neither writes anything."""
    sole = (SOLE[0], SOLE[1], SOLE[2], SOLE[1] * 0.5)
    foot = lambda x: np.array([[x, 0.1, 0.0, 0.0, 0.0, 0.0]])  # noqa: E731
    gait = (np.zeros(1), foot(0.0), np.zeros(1, np.int32), foot(0.3))
    ref, got = both(gait, cap, sole)
    assert ref[3] == -1 and got[3] == BAD
    assert got[:3] == ref[:3]


def test_no_samples():
    fn = wg.lib().wg_foot_constraints
    fn.argtypes, fn.restype = ARGTYPES, C.c_int
    assert fn(0, None, None, None, None, *SOLE, 0, None, None, None) == 0
    empty = (np.zeros(0), np.zeros((0, 6)), np.zeros(0, np.int32), np.zeros((0, 6)))
    ref, got = both(empty, QCAP)
    assert got == ref and got[3] == 0
