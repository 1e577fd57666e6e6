"""The inputs of tests/test_models_gpu.py, proved good on the CPU: every model and gait tests/modelgen.py generates runs on
the portable-trig oracle alone, the share of (model, gait) pairs with a failed QP stays within a tenth, the traces cover what
the sweep is meant to cover, and a scan over step periods fixes -- from the oracle, not from the library -- which models
preview more than the four steps the tick kernels hold.

What the scan finds at T = 0.1 s (largest nb_prw_steps over three step periods of walking; 99: more than the oracle's own
six):
    step_period  2.0 1.6 1.2 1.0 0.9 0.8 0.75 0.7 0.65 0.6 0.55 0.5 0.45 0.4 0.35 0.3 0.25 0.2
    N = 16         1   1   2   2   2   2   2    3   3    3   3    3   3    4   4    5   5    99
    N = 32         2   2   3   4   4   4   4    5   5    6   6    99  99   99  99   99  99   99
Five steps first appear at step_period = 0.3 (N = 16) and 0.7 (N = 32); wg_mpc_configure refuses both."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modelgen as mg  # noqa: E402
import workload as w  # noqa: E402

RC, IFAIL, NS, NVAR, PHASE, LEFT, HIP = range(7)                 # columns of modelgen.oracle_trace


@pytest.fixture(scope="module")
def sweep():
    """{(config, model name, gait): trace} of the whole model sweep"""
    pt = w.ptrig()
    res = {}
    for name in mg.SWEEP_NAMES:
        for k, (mname, m) in enumerate(mg.sweep_models(name)):
            seg = mg.stretch_ticks(m)
            for g, vel in enumerate(mg.sweep_gaits(name, k)):
                rows, states = mg.oracle_trace(pt, m, vel, seg * len(vel), seg)
                assert len(states) == seg * len(vel) and (rows[:, RC] == 0).all(), (name, mname, g, rows[-1, RC])
                assert not any(np.isnan(np.frombuffer(s, dtype=np.float64)).any() for s in states), (name, mname, g)
                res[(name, mname, g)] = rows
    return res


def test_every_generated_model_and_gait_runs_on_the_oracle(sweep):
    assert len(sweep) == sum(len(c[3]) + len(c[4]) for c in mg.SWEEP) * mg.SWEEP_GAITS
    for key, rows in sweep.items():
        assert (rows[:, NVAR] == 2 * dict((c[0], c[1]) for c in mg.SWEEP)[key[0]] + 2 * rows[:, NS]).all(), key


def test_failed_solves_stay_within_a_tenth_of_the_pairs(sweep):
    """ticks whose QP fails are part of the comparison on the GPU (never skipped); here their share is bounded"""
    failing = sorted(k for k, rows in sweep.items() if (rows[:, IFAIL] != 0).any())
    print("pairs with a failed QP: %d of %d: %s" % (len(failing), len(sweep), failing))
    assert 0 < len(failing) <= 0.1 * len(sweep), failing
    # both kinds: a model that fails throughout and one that fails on a few ticks and solves again
    shares = [float((sweep[k][:, IFAIL] != 0).mean()) for k in failing]
    assert max(shares) > 0.5 and min(shares) < 0.25, shares


def test_the_sweep_covers_steps_phases_stops_and_hip_limits(sweep):
    for name in mg.SWEEP_NAMES:
        rows = np.concatenate([r for k, r in sweep.items() if k[0] == name])
        N = dict((c[0], c[1]) for c in mg.SWEEP)[name]
        seen = set(rows[:, NS].astype(int))
        most = max(mg.max_previewed_steps(N, m.T, m.step_period) for _, m in mg.sweep_models(name))
        assert seen == set(range(most + 1)), (name, seen, most)           # every count the configuration can pose
        assert set(rows[:, PHASE].astype(int)) == {0, 1}, name            # single and double support
    everything = np.concatenate(list(sweep.values()))
    assert set(everything[:, NS].astype(int)) == {0, 1, 2, 3, 4}
    assert {"16c": 2, "16e": 4, "32": 4}.items() <= {n: int(max(r[:, NS].max() for k, r in sweep.items() if k[0] == n))
                                                     for n in mg.SWEEP_NAMES}.items()
    stopped_and_walked_again, on_hip_limit = [], []
    for key, rows in sweep.items():
        z = np.flatnonzero((rows[:, LEFT] == 0) & (rows[:, PHASE] == 1))  # no steps left, standing in double support
        if len(z) and (rows[z[0]:, PHASE] == 0).any() and (rows[z[0]:, LEFT] > 0).any():
            stopped_and_walked_again.append(key)
        # verify_angle_hip_joint steers the trunk to 0.9 of the limit at the end of the support phase: a gait whose trunk
        # is held there has ticks beyond 0.8 of it
        if (np.abs(rows[:, HIP]) >= 0.8).any():
            on_hip_limit.append(key)
    print("stop + restart: %d gaits; on a hip limit: %s" % (len(stopped_and_walked_again), on_hip_limit))
    assert len(stopped_and_walked_again) >= len(sweep) // 2
    assert on_hip_limit
    clamped = {k[0] for k, rows in sweep.items() if (rows[:, HIP] != 0).any()}
    assert clamped == set(mg.SWEEP_NAMES), clamped                       # the limit intervened in every configuration


def test_every_horizon_previews_all_the_steps_it_can():
    pt = w.ptrig()
    n_ticks = mg.HORIZON_STRETCH_TICKS * len(mg.HORIZON_STRETCHES)
    for N in range(2, 33):
        m = mg.horizon_model(N)
        seen = set()
        for vel in mg.gaits(N, 4, mg.HORIZON_STRETCHES):
            rows, _ = mg.oracle_trace(pt, m, vel, n_ticks, mg.HORIZON_STRETCH_TICKS)
            assert len(rows) == n_ticks and (rows[:, RC] == 0).all() and (rows[:, IFAIL] == 0).all(), N
            seen |= set(rows[:, NS].astype(int))
        # the most steps the horizon can hold, and another count next to it (the long horizons never preview fewer than
        # one or two steps: the first ones lie 1.6 and 2.4 s ahead of the start)
        most = mg.max_previewed_steps(N, m.T, m.step_period)
        assert max(seen) == most and {most - 1, most} <= seen, (N, seen)


def test_view_models_pose_the_steps_their_view_is_for():
    pt = w.ptrig()
    most = {}
    for p in mg.VIEW_STEP_PERIODS:
        m = mg.view_model(p)
        seg = mg.stretch_ticks(m)
        traces = [mg.oracle_trace(pt, m, vel, 2 * seg, seg) for vel in mg.gaits(int(p * 100), 3, mg.HORIZON_STRETCHES)]
        rows = np.concatenate([t[0] for t in traces])
        assert (rows[:, RC] == 0).all(), p
        assert not any(np.isnan(np.frombuffer(s, dtype=np.float64)).any() for t in traces for s in t[1]), p
        print("step_period %.2f: %d of %d QPs failed" % (p, int((rows[:, IFAIL] != 0).sum()), len(rows)))
        most[p] = int(rows[:, NS].max())
        assert mg.compact_view(m) == (p >= 0.8)
    assert most == {2.0: 1, 1.6: 1, 1.0: 2, 0.8: 2, 0.75: 2, 0.7: 3, 0.5: 3, 0.4: 4}, most


SCAN = {16: {2.0: 1, 1.6: 1, 1.2: 2, 1.0: 2, 0.9: 2, 0.8: 2, 0.75: 2, 0.7: 3, 0.65: 3, 0.6: 3, 0.55: 3, 0.5: 3, 0.45: 3, 0.4: 4,
             0.35: 4, 0.3: 5, 0.25: 5, 0.2: 99},
        32: {2.0: 2, 1.6: 2, 1.2: 3, 1.0: 4, 0.9: 4, 0.8: 4, 0.75: 4, 0.7: 5, 0.65: 5, 0.6: 6, 0.55: 6, 0.5: 99, 0.45: 99, 0.4: 99,
             0.35: 99, 0.3: 99, 0.25: 99, 0.2: 99}}
# the last grid point that previews at most four steps / the first where the oracle sees five (tests/test_models_gpu.py)
LAST_ACCEPTED = {16: 0.35, 32: 0.75}
FIRST_REFUSED = {16: 0.3, 32: 0.7}


@pytest.mark.parametrize("N", [16, 32])
def test_scan_of_previewed_steps_over_the_step_period(N):
    """The oracle's own count, next to the bound wg_mpc_configure refuses by (modelgen.max_previewed_steps restates
    tick_max_prw_steps of wg_capi.hip): the bound is never below what the oracle saw, so no model that previews more than
    four steps is accepted."""
    scan = mg.scan_previewed_steps(w.ptrig(), N)
    print("N = %d: %s" % (N, scan))
    assert scan == SCAN[N]
    grid = list(mg.STEP_PERIOD_GRID)
    assert all(scan[a] <= scan[b] for a, b in zip(grid, grid[1:]))        # shorter steps, more of them
    for p, seen in scan.items():
        bound = mg.max_previewed_steps(N, 0.1, p)
        assert bound >= min(seen, 7), (p, seen, bound)                    # 99: more than the oracle's six
        assert (bound > mg.S_MAX) == (seen > mg.S_MAX), (p, seen, bound)  # and it refuses nothing the tick could hold
    five = [p for p in grid if scan[p] > mg.S_MAX]
    assert five[0] == FIRST_REFUSED[N] and grid[grid.index(five[0]) - 1] == LAST_ACCEPTED[N]
    assert scan[LAST_ACCEPTED[N]] == mg.S_MAX


def test_the_library_states_the_same_bound():
    """wg_mpc_tick_lds_bytes_for is host arithmetic (no GPU): 0 for exactly the grid points the scan found to preview more
    than four steps"""
    import importlib
    wg = importlib.import_module("jrl-walkgen_amd")
    for N in (16, 32):
        for p, seen in SCAN[N].items():
            m = mg.defaults(N)
            mg.set_step_period(m, p)
            lds = wg.lib().wg_mpc_tick_lds_bytes_for(C.byref(m))
            assert (lds == 0) == (seen > mg.S_MAX), (N, p, seen, lds)
