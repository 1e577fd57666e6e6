"""GPU parity of the PLDP/OptCholesky back-end (through the C ABI) against oracle/pldp_oracle.c: bit-identical
solutions, iteration counts, active-set index sequences (activation order) and hot-start states, over whole
receding-horizon gaits with de-synchronised footstep plans, including the solves that end in the reference's
"initial solution is incorrect" exit."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimitrov as dv  # noqa: E402
import oraclelib as ol  # noqa: E402
import pldplock as pl  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu


from pldplock import pack as _pack, ql_gate as _ql_gate, state_tuple as _state_tuple  # noqa: E402,F401  (shared with the shape tests)


def _run_lockstep(B, n_ticks, seed0, max_iter=0, mcap=wg.PLDP_MMAX, gate=None, N=16, plans=None, offs=None):
    """B gaits x n_ticks on the GPU and the oracle in lock step (tests/pldplock.py); the standard plans unless `plans` is given"""
    dm = dv.Dimitrov(N)
    wg.init(0)
    wg.pldp_configure(dm.N, dm.iPu, dm.Px, dm.Pu)
    if plans is None:
        plans = [dv.plan(np.random.default_rng(seed0 + g), n_steps=4 + g % 5) for g in range(B)]
    if offs is None:
        offs = [(3 * g) % 9 for g in range(B)]              # de-synchronise the gaits in time
    return pl.run_lockstep(dm, plans[:B], n_ticks, offs[:B], max_iter=max_iter, mcap=mcap, gate=gate, gpu_solve=wg.pldp_solve_batch,
                           gpu_states=(wg.PldpState * B)())


@pytest.mark.parametrize("a_in_lds", ["0", "1"])
def test_pldp_gaits_bit_exact(a_in_lds, monkeypatch):
    """both placements of the constraint matrix (staged in LDS / read in place from L2, the default at m = 128)"""
    monkeypatch.setenv("WG_PLDP_A_IN_LDS", a_in_lds)
    st = _run_lockstep(B=24, n_ticks=45, seed0=100)
    assert st["solves"] > 600 and max(st["nact"]) >= 10 and max(st["iters"]) >= 6
    assert st["neg_alpha"] > 0                              # the reference's exit(0) path is among the solves compared


def test_pldp_solutions_against_the_pinned_ql_oracle_on_every_solve():
    """the property gate of _ql_gate on every successful solve of 24 de-synchronised gaits x 45 ticks (GPU solutions)"""
    gate = dict(solves=0, optimal=0, stuck=0, worst_gap=0.0, worst_dx=0.0)
    _run_lockstep(B=24, n_ticks=45, seed0=100, gate=gate)
    print("PLDP vs QL:", gate)
    # measured (same numbers on the CPU restatement, whose bits the GPU reproduces): ~7 % of the solves end at the optimum,
    # the others on a vertex PLDP could not leave (objective up to 2 x the optimum's) -- the method trades optimality for
    # speed by design (Dimitrov 2008); what holds on every solve is feasibility and f(X) >= f(v*)
    assert gate["solves"] > 600 and gate["optimal"] >= 30 and gate["optimal"] + gate["stuck"] == gate["solves"], gate


def test_pldp_iteration_cap_bit_exact():
    st = _run_lockstep(B=8, n_ticks=25, seed0=300, max_iter=3)
    assert st["solves"] > 100 and max(st["iters"]) == 3


def test_pldp_small_slots_and_rejections():
    # mcap below the largest m is refused per problem, positive SimilarConstraint offsets too
    dm = dv.Dimitrov()
    wg.init(0)
    wg.pldp_configure(dm.N, dm.iPu, dm.Px, dm.Pu)
    segs = dv.plan(np.random.default_rng(5))
    p = dm.problem(np.zeros(6), dv.polys_at(segs, 0, dm.N))
    assert p["m"] == 64
    m, D, A, b, z, xk, sim = _pack(dm, [p, p], 64)
    st = (wg.PldpState * 2)()
    sim[1, 0] = 3
    out = wg.pldp_solve_batch(dm.N, 64, m, D, A, b, z, xk, sim, np.zeros(2, np.int32), np.ones(2, np.int32), st)
    assert out["ret"][0] == 0 and out["ret"][1] == -4
    M = ol.pldp_setup(dm.N, dm.iPu, dm.Px, dm.Pu)
    o = ol.pldp_solve(M, ol.PldpState(), p["D"], p["m"], p["A"], p["b"], p["zmpref"], p["xk"], p["similar"], 0, True)
    assert np.array_equal(out["X"][0], o["X"])
    m2 = m.copy(); m2[0] = 65
    out = wg.pldp_solve_batch(dm.N, 64, m2, D, A, b, z, xk, sim, np.zeros(2, np.int32), np.ones(2, np.int32), st)
    assert out["ret"][0] == -4
    lib = wg.lib()
    assert lib.wg_pldp_solve_batch(1, 500, None, None, None, None, None, None, None, None, None, 0, None, None, None, None,
                                   None, None) != 0
    assert wg.pldp_lds_bytes() <= 64 * 1024
