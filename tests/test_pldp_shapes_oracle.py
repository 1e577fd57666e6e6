"""What the inputs of tests/test_pldp_shapes_gpu.py and tests/test_dimitrov_shapes_gpu.py reach, established on the oracle alone
(oracle/pldp_oracle.c, no GPU): those comparisons must not pass on empty coverage.  The families of tests/pldpgen.py drive the
oracle to m = 128, to active rows either side of row 64 in one solve, to active sets of 18 rows and more, to the exit(0) path (-2)
at N = 16 and below, through every horizon the GPU tests use; the straddle and duplicate layouts are what they claim to be, and the
first twin of the duplicate layout to be activated is row 63 (the reference's strict `>` in ComputeAlpha's running minimum,
PLDPSolver.cpp:622-633).

The property gate of pldplock.ql_gate (feasibility, f(X) >= f(v*), X == v* where the KKT signs hold; constants 5e-8, 2e-5, 1e-9 as
derived for the standard plans) runs on every successful oracle solve of the 8-row, 6-row and mixed families at N = 16 and N = 5.
Measured: it holds on all of them with the constants unchanged -- no family is excluded from the gate."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimitrov as dv  # noqa: E402
import oraclelib as ol  # noqa: E402
import pldpgen as pg  # noqa: E402
import pldplock as pl  # noqa: E402

B, TICKS = 12, 30                         # the size of every GPU case
HORIZONS = (1, 2, 3, 7, 12, 15)
ACTIVE_CAP = 40                           # WG_PLDP_ACTIVE_CAP: the oracle has no capacity, the kernel refuses beyond it


@functools.lru_cache(maxsize=None)
def oracle_run(name, N, gate=False):
    plans, offs = pg.fleet(name, B)
    g = pl.new_gate() if gate else None
    events = []
    st = pl.run_lockstep(dv.Dimitrov(N), plans, TICKS, offs, gate=g,
                         on_solve=lambda it, gi, p, o: events.append((it + offs[gi], p["m"], p["similar"].copy(), o["active"].copy(), o["ret"])))
    st["gate"], st["events"] = g, events
    print("N = %2d %-9s %s%s" % (N, name, pl.summary(st), "; gate %s" % g if gate else ""))
    return st


def test_rows_above_68_both_lane_slots_and_large_active_sets():
    r8, r6, mx = oracle_run("rows8", 16, True), oracle_run("rows6", 16, True), oracle_run("mixed", 16, True)
    assert set(r8["m"]) == {128} and r8["max_row"] == 127 and r8["both_halves"] > 200
    assert set(r6["m"]) == {96} and r6["both_halves"] > 150
    assert min(mx["m"]) < 64 < 100 < max(mx["m"]) and mx["both_halves"] > 50
    runs = [oracle_run(f, 16) for f in ("straddle", "duplicate")] + [r8, r6, mx]
    assert max(max(r["nact"]) for r in runs) >= 18
    # below the kernel's capacity everywhere: a -3 from the GPU would be a difference by design, not a finding
    assert all(max(r["nact"], default=0) <= ACTIVE_CAP for r in runs)


def test_exit_codes_occur():
    assert oracle_run("rows8", 16, True)["rets"][-2] > 0 and oracle_run("std", 7)["rets"][-2] > 0
    assert oracle_run("duplicate", 16)["rets"][-1] > 0          # the singular factor of two identical active rows ends in NaN


@pytest.mark.parametrize("N", HORIZONS + (5,))
def test_every_horizon_runs(N):
    for fam in ("std", "rows8"):
        st = oracle_run(fam, N, gate=(N == 5 and fam == "rows8"))
        assert st["solves"] >= 150 and st["rets"][0] >= 150 and max(st["iters"]) >= 3, (N, fam, pl.summary(st))
        if fam == "rows8":
            assert set(st["m"]) == {8 * N}
    assert max(oracle_run("std", 1)["m"]) <= 6 and oracle_run("rows8", 15)["both_halves"] > 100


def test_empty_family_reaches_m_zero():
    for N in (16, 5, 1):
        st = oracle_run("empty", N)
        assert 0 in st["m"] and max(st["m"]) <= 24 and any(0 < m for m in st["m"]), pl.summary(st)


def test_straddle_layout():
    st = oracle_run("straddle", 16)
    hits = [e for e in st["events"] if e[0] % 16 == 0]
    assert len(hits) >= 20
    for (_, m, sim, act, _) in hits:
        assert m == 67 and list(sim[61:67]) == [0, 0, 0, -3, -3, -3]
    assert set(st["m"]) == {67}
    # the hexagon's rows do get activated, on both sides of the boundary
    assert any(set(e[3]) & {61, 62, 63} for e in hits) and any(set(e[3]) & {64, 65, 66} for e in hits)


def test_duplicate_layout_and_first_twin():
    plans, offs = pg.fleet("duplicate", B)
    dm = dv.Dimitrov(16)
    for g in (0, 1):                                            # the twins really are one half-plane, as problem rows
        p = dm.problem(np.zeros(6), pg.polys_at(plans[g], 16, 16))
        A = p["A"].reshape((32, p["m"] + 1)).T
        assert p["m"] == 65 and np.array_equal(A[63], A[64]) and p["b"][63] == p["b"][64] and not p["similar"][63:65].any()
    st = oracle_run("duplicate", 16)
    hits = [e for e in st["events"] if e[0] % 16 == 0]
    firsts = [[r for r in e[3] if r in (63, 64)] for e in hits]
    assert sum(bool(f) for f in firsts) >= 4                   # the tie is decided in several solves ...
    assert all(f[0] == 63 for f in firsts if f)                # ... always for the lower index


def test_ragged_batches():
    for mcap in (128, 100, 1):
        ms, plans = pg.ragged_batch(np.random.default_rng(7), mcap)
        assert ms == [m for m in pg.RAGGED_M if m <= mcap] and all(len(p) >= TICKS + 16 for p in plans)
        st = pl.run_lockstep(dv.Dimitrov(16), plans, TICKS)
        assert set(st["m"]) == set(ms) and st["rets"][0] > 0.8 * st["solves"], pl.summary(st)


def test_property_gate_on_the_new_families():
    """pldplock.ql_gate on every successful oracle solve of the 8-row, 6-row and mixed families at N = 16 and N = 5"""
    for N in (16, 5):
        for fam in ("rows8", "rows6", "mixed"):
            g = oracle_run(fam, N, True)["gate"]
            assert g["solves"] >= 80 and g["optimal"] >= 10 and g["optimal"] + g["stuck"] == g["solves"], (N, fam, g)
