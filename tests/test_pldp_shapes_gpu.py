"""wg_pldp_solve_batch against oracle/pldp_oracle.c outside the band tests/test_pldp_gpu.py reaches: horizons below 16, more than
68 rows (the second slot of every lane in the step-length pass), reuse pairs across row 64, an exact arg-min tie between rows 63
and 64, ragged batches in slots smaller than WG_PLDP_MMAX, and the error exits -1, -2, -3.  Same lock-step driver
(tests/pldplock.py): ret, iteration count, activation sequence, X and hot-start state after every solve, bit for bit.  What each
family reaches is asserted on the oracle alone in tests/test_pldp_shapes_oracle.py; every case here is 12 gaits x 30 ticks."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimitrov as dv  # noqa: E402
import oraclelib as ol  # noqa: E402
import pldpgen as pg  # noqa: E402
import pldplock as pl  # noqa: E402
from test_pldp_gpu import _run_lockstep  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu

B, TICKS = 12, 30


def _family(name, N, **kw):
    plans, offs = pg.fleet(name, B)
    st = _run_lockstep(B, TICKS, 0, N=N, plans=plans, offs=offs, **kw)
    print("N = %2d %-9s %s" % (N, name, pl.summary(st)))
    return st


# ---- horizons ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["std", "rows8"])
@pytest.mark.parametrize("N", [1, 2, 3, 7, 12, 15])
def test_horizons_below_16(N, fam):
    st = _family(fam, N)
    assert st["solves"] >= 150 and st["rets"][0] >= 150
    if fam == "rows8":
        assert set(st["m"]) == {8 * N}                      # the slot is full: m = mcap of the fused tick at this horizon
    if N == 7:
        assert st["neg_alpha"] > 0                          # the exit(0) path at a horizon below 16


def test_one_context_reconfigured_16_5_16():
    """a stale model, staging size or carve would show in the second or third run"""
    for N in (16, 5, 16):
        for fam in ("std", "rows8"):
            plans, offs = pg.fleet(fam, 6)
            st = _run_lockstep(6, 12, 0, N=N, plans=plans, offs=offs)
            assert st["solves"] >= 60 and set(st["m"]) <= ({8 * N} if fam == "rows8" else set(range(4 * N, 4 * N + 5)))


# ---- both row halves -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_in_lds", ["0", "1"])
@pytest.mark.parametrize("fam", ["rows8", "rows6", "mixed", "straddle", "duplicate"])
def test_rows_in_both_lane_slots(fam, a_in_lds, monkeypatch):
    monkeypatch.setenv("WG_PLDP_A_IN_LDS", a_in_lds)
    st = _family(fam, 16)
    assert st["max_row"] >= 64 and st["both_halves"] > 50 and max(st["m"]) > 64
    if fam == "rows8":
        assert set(st["m"]) == {128} and st["max_row"] == 127 and st["neg_alpha"] > 0       # -2 occurs in the fleet
    if fam == "duplicate":
        assert st["rets"][-1] > 0                           # two identical active rows: NaN factor, the reference's -1
    if fam in ("straddle", "duplicate"):
        assert max(st["nact"]) >= 18


# ---- slots ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mcap", [128, 100, 1])
def test_ragged_batch_in_one_slot_size(mcap):
    ms, plans = pg.ragged_batch(np.random.default_rng(7), mcap)
    st = _run_lockstep(len(plans), TICKS, 0, mcap=mcap, plans=plans, offs=[0] * len(plans))
    print("mcap %3d %s" % (mcap, pl.summary(st)))
    assert set(st["m"]) == set(ms) and st["rets"][0] > 0.8 * st["solves"]


def _setup16():
    dm = dv.Dimitrov()
    wg.init(0)
    wg.pldp_configure(dm.N, dm.iPu, dm.Px, dm.Pu)
    return dm, ol.pldp_setup(dm.N, dm.iPu, dm.Px, dm.Pu)


def test_optional_outputs_null():
    """n_iter, active and n_active are optional: the same X, ret and states without them (mcap = 100, ragged m)"""
    dm, _ = _setup16()
    mcap = 100
    ms, plans = pg.ragged_batch(np.random.default_rng(7), mcap)
    nB = len(plans)
    probs = [dm.problem(np.array([0.01, 0.0, 0.0, -0.01, 0.0, 0.0]), pg.polys_at(p, 0, dm.N)) for p in plans]
    m, D, A, b, z, xk, sim = pl.pack(dm, probs, mcap)
    zero = np.zeros(nB, np.int32); one = np.ones(nB, np.int32)
    st_a = (wg.PldpState * nB)(); st_b = (wg.PldpState * nB)()
    full = wg.pldp_solve_batch(dm.N, mcap, m, D, A, b, z, xk, sim, zero, one, st_a)
    X = np.full((nB, 2 * dm.N), -7.25); ret = np.full(nB, -77, np.int32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = wg.lib().wg_pldp_solve_batch(nB, mcap, hp(m), hp(D), hp(A), hp(b), hp(z), hp(xk), hp(sim), hp(zero), hp(one), 0,
                                      C.addressof(st_b), hp(X), hp(ret), None, None, None)
    assert rc == 0
    assert ol.same_bits(X, full["X"]) and np.array_equal(ret, full["ret"]) and bytes(st_a) == bytes(st_b)
    assert (ret == 0).all()


# ---- exits -1 and -3 --------------------------------------------------------------------------------------------------------------
def _second_tick(craft):
    """Three gaits of the standard plans: tick 0 on both sides, then tick 1 with gait 1's inputs changed by craft(state, xk, m) -> xk.
    The neighbours (gaits 0 and 2) are held to the oracle as in every lock-step run.
    -> (GPU out, GPU states, gait 1's state as it went in, gait 1's problem, oracle model)"""
    dm, M = _setup16()
    plans, offs = pg.fleet("std", 3)
    st_g = (wg.PldpState * 3)(); st_o = [ol.PldpState() for _ in range(3)]
    xk = [np.array([0.002 * g, 0.0, 0.0, 0.0, 0.001 * g, 0.0]) for g in range(3)]
    probs = [dm.problem(xk[g], pg.polys_at(plans[g], offs[g], dm.N)) for g in range(3)]
    mcap = 68
    out = wg.pldp_solve_batch(dm.N, mcap, *pl.pack(dm, probs, mcap), np.zeros(3, np.int32), np.ones(3, np.int32), st_g)
    for g in range(3):
        p = probs[g]
        o = ol.pldp_solve(M, st_o[g], p["D"], p["m"], p["A"], p["b"], p["zmpref"], p["xk"], p["similar"], 0, True)
        assert out["ret"][g] == o["ret"] == 0 and ol.same_bits(out["X"][g], o["X"]) and pl.same_state(st_g[g], st_o[g])
        xk[g] = dm.step(xk[g], o["X"])
    n_removed = np.array([p["first_rows"] for p in probs], dtype=np.int32)
    assert n_removed[1] == 4
    m1 = sum(len(q[1]) for q in pg.polys_at(plans[1], 1 + offs[1], dm.N))
    xk[1] = craft(st_g[1], xk[1], m1)
    C.memmove(C.byref(st_o[1]), C.byref(st_g[1]), C.sizeof(wg.PldpState))
    went_in = ol.PldpState.from_buffer_copy(bytes(st_o[1]))
    probs = [dm.problem(xk[g], pg.polys_at(plans[g], 1 + offs[g], dm.N)) for g in range(3)]
    assert probs[1]["m"] == m1 and 64 <= m1 <= mcap
    out = wg.pldp_solve_batch(dm.N, mcap, *pl.pack(dm, probs, mcap), n_removed, np.zeros(3, np.int32), st_g)
    for g in (0, 2):                                         # the neighbours: untouched by what happens in the middle
        p = probs[g]
        o = ol.pldp_solve(M, st_o[g], p["D"], p["m"], p["A"], p["b"], p["zmpref"], p["xk"], p["similar"], int(n_removed[g]), False)
        assert out["ret"][g] == o["ret"] == 0 and out["n_iter"][g] == o["n_iter"] and np.array_equal(out["active"][g], o["active"])
        assert ol.same_bits(out["X"][g], o["X"]) and pl.same_state(st_g[g], st_o[g])
    return out, st_g, went_in, probs[1], M, int(n_removed[1]), st_o[1]


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_state_gives_the_references_minus_one(bad):
    def craft(state, xk, m):
        xk = xk.copy(); xk[1] = bad
        return xk
    out, st_g, _, p, M, n_removed, st_o = _second_tick(craft)
    o = ol.pldp_solve(M, st_o, p["D"], p["m"], p["A"], p["b"], p["zmpref"], p["xk"], p["similar"], n_removed, False)
    assert o["ret"] == -1 and out["ret"][1] == -1
    assert out["n_iter"][1] == o["n_iter"] and np.array_equal(out["active"][1], o["active"])
    assert np.isnan(o["X"]).any() and ol.same_bits_nan_aware(out["X"][1], o["X"])
    assert pl.same_state(st_g[1], st_o)


def _refused(craft):
    """the contract of WG_PLDP_CAPACITY for a refused hot start (include/wg_mpc.h): nothing solved, the state's members cleared, X the
    point the solve would have started from"""
    out, st_g, went_in, p, M, n_removed, _ = _second_tick(craft)
    assert out["ret"][1] == -3 and out["n_iter"][1] == 0
    assert st_g[1].n_prev == 0
    assert ol.same_bits(out["X"][1], ol.pldp_initial_solution(M, went_in, p["zmpref"], p["xk"], False))
    # the rest of the state is as it went in (a refused solve stores no ZMP solution and does not advance the clock)
    assert list(st_g[1].prev_zmp) == list(went_in.prev_zmp) and st_g[1].internal_time == went_in.internal_time


def test_hot_start_beyond_the_active_capacity_is_refused():
    def craft(state, xk, m):
        state.n_prev = 41                                    # WG_PLDP_ACTIVE_CAP + 1 valid, distinct rows (n_removed = 4: 0..40 after it)
        for i in range(41):
            state.prev_active[i] = 4 + i
        return xk
    _refused(craft)


def test_hot_start_row_beyond_m_is_refused():
    def craft(state, xk, m):
        state.n_prev = 2
        state.prev_active[0] = 9                             # row 5 after n_removed = 4: valid
        state.prev_active[1] = m + 4 + 2                     # row m + 2 after it: past the problem's last row
        return xk
    _refused(craft)
