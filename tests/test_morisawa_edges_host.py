"""The Morisawa families between the arguments the other tests reach (omega * 3 t_single <= 10.66) and the admission bound
WG_MORISAWA_WALK_ARG_MAX (include/wg_mpc.h), on the bound and beyond it: the host twins wg_morisawa_solve*, wg_morisawa_long_solve* and
their samplers against the restatement tests/morisawa.py in float64 and in 50-digit mpmath.  No GPU.

The rule is the one of tests/test_morisawa_host.py: d_ref is the largest distance of the float64 restatement from the
50-digit one, the host twin stays within D_REF_FACTOR x d_ref, and D_REF_FACTOR x d_ref stays below D_REF_CEILING.  Here d_ref is taken
per argument X and family, over the gaits that reach X -- d_ref(X) of tools/measure_morisawa_admission.py, whose table
profiles/morisawa_admission.txt fixes the bound: what is admitted is accurate, what would not be is refused, and nothing at or
below the bound is refused.

Measured here (figures also in DESIGN.md 3.13):
  test_what_is_admitted_is_accurate, the worst admitted argument X = 13.5: short d_ref = 2.4e-10 m, host twin 1.4e-10 m; long
  d_ref = 8.7e-11 m, host twin 1.5e-10 m; the largest 16 x d_ref is 3.8e-9 m.  With the parent's library (every argument up to 40
  admitted) the test fails at X = 15.0, short family: d_ref = 1.3e-9 m, 16 x d_ref = 2.1e-8 m.
  test_truth_at_64_steps: see there."""
import numpy as np
import pytest

import morisawa as mo
import morisawa_edges as me
import morisawa_fleets as mf
import morisawa_replan as rp
from test_morisawa_host import D_REF_CEILING, D_REF_FACTOR

SHORT_S, LONG_S = (2, 7, 14), (15, 24)


@pytest.fixture(scope="module")
def wg():
    return mf.wg()


def one_gait(S, seed, h, ts, td):
    f = mf.Fleet(1, S, seed)
    me.set_timing(f, 0, h, ts, td)
    return f


def distances(fam, f, blocks, between=50):
    """(d_ref, d_twin) of gait 0 of the one-gait fleet f, sampled from its block on its own clock from 2 t_single"""
    m, S = f.models[0], int(f.n_steps[0])
    t0 = mf.t_start_of(m)
    L = fam.length(m, S, t0)
    assert L == mo.length(mf.model_dict(m), S, t0) > 100
    r = fam.sample(blocks[0:1], None, f.smax, t0, m.T, L)
    assert list(r["length"]) == [L]
    ks, tv, v64, nat = me.truth_samples(mo, f, 0, t0, L, between)
    tw = me.sampled_columns(r, ks, 0)
    assert [(r["left_type"][k, 0], r["right_type"][k, 0]) for k in ks] == nat
    return float(np.abs(v64 - tv).max()), float(np.abs(tw - tv).max())


def test_what_is_admitted_is_accurate(wg):
    """Arguments 8 .. 40 in steps of 1, of 0.5 within 2 of the bound; the three routes; short at S = 2, 7, 14, long at S = 15, 24.  A gait
    is refused (WG_MORISAWA_BAD_INPUT, and then its argument is beyond the bound) or WG_OK within 16 x d_ref(X) of the truth with
    16 x d_ref(X) < 1e-8 m, d_ref(X) over the family's gaits at X."""
    bound = me.header_bound()
    grid = sorted(set([8.0 + i for i in range(33)] + [x for x in (8.0 + 0.5 * i for i in range(65)) if abs(x - bound) <= 2.0]))
    assert grid[0] == 8.0 and grid[-1] == 40.0 and any(x <= bound for x in grid) and any(x > bound for x in grid)
    worst = {}
    for X in grid:
        for long_, sizes in ((False, SHORT_S), (True, LONG_S)):
            fam = rp.Family(long_)
            found = []
            for r, route in enumerate(me.ROUTES):
                for S in sizes:
                    rng = np.random.default_rng([1800, int(2 * X), r, S])
                    f = one_gait(S, 1800 + int(2 * X) + r, *me.timing(route, X, rng))
                    arg = me.argument(f.com0[0, 2], f.models[0].t_single, f.models[0].t_double)
                    assert abs(arg - X) <= 1e-12 * X
                    blocks, st = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, S)
                    if st[0] != 0:
                        assert st[0] == wg.MORISAWA_BAD_INPUT and arg > bound, (X, route, S, int(st[0]))    # nothing within the bound is refused
                        continue
                    found.append((route, S) + distances(fam, f, blocks))
            if found:
                d_ref, d_twin = max(d[2] for d in found), max(d[3] for d in found)
                print("X %.1f %s: d_ref %.3g, host twin %.3g, bound %.3g" % (X, fam.name, d_ref, d_twin, D_REF_FACTOR * d_ref))
                assert D_REF_FACTOR * d_ref < D_REF_CEILING, (X, fam.name, found)
                assert d_twin <= D_REF_FACTOR * d_ref, (X, fam.name, found)
                worst[long_] = max(worst.get(long_, (0.0, 0.0, 0.0)), (d_ref, d_twin, X))
    assert set(worst) == {False, True}
    print("worst admitted: short d_ref %.3g twin %.3g at %.1f; long d_ref %.3g twin %.3g at %.1f" % (worst[False] + worst[True]))


@pytest.mark.parametrize("long_,S", ((False, 3), (True, 15)))
def test_the_bound_is_the_measured_one(wg, long_, S):
    """the header's macro is X* of profiles/morisawa_admission.txt; on each route the last time within it is WG_OK and the next double
    past it is refused with the caller's pattern left in the block"""
    bound = me.header_bound()
    assert bound == me.measured_bound()
    fam = rp.Family(long_)
    for r, route in enumerate(me.ROUTES):
        rng = np.random.default_rng([1900, r, S])
        inside, outside = me.step_to_bound(route, *me.timing(route, bound, rng), bound)
        for timing, ok in ((inside, True), (outside, False)):
            f = one_gait(S, 1900 + r, *timing)
            blocks = np.full((1, fam.words(S)), rp.PATTERN)
            _, st = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, S, blocks=blocks)
            one, st1 = fam.solve(f.models[0], f.steps, f.n_steps, f.init_feet, f.com0, S, blocks=np.full((1, fam.words(S)), rp.PATTERN))
            assert st[0] == st1[0] == (0 if ok else wg.MORISAWA_BAD_INPUT), (route, ok)
            assert one.tobytes() == blocks.tobytes()
            if ok:
                assert fam.view(blocks[0], S)["n_steps"] == S and not (blocks[0] == rp.PATTERN).any()
            else:
                assert (blocks == rp.PATTERN).all()
        # the re-plan admits what the solve admits: a factor block of the inside timing, the plan's model one double past it
        f = one_gait(S, 1900 + r, *inside)
        fac, st = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, S)
        assert st[0] == 0
        got, st = fam.resolve(f.models, fac, None, f.steps, f.init_feet, f.com0, S, blocks=np.full_like(fac, rp.PATTERN))
        assert st[0] == 0 and got.tobytes() == fac.tobytes()
        g = one_gait(S, 1900 + r, *outside)
        got, st = fam.resolve(g.models, fac, None, g.steps, g.init_feet, g.com0, S, blocks=np.full_like(fac, rp.PATTERN))
        assert st[0] == wg.MORISAWA_BAD_INPUT and (got == rp.PATTERN).all()


def test_truth_at_64_steps(wg):
    """one gait at the long family's cap under the rule of test_long_samples_against_the_mpmath_truth (the 50-digit solve of
    n = 264 takes about a minute), at the corner of mf.Fleet's ranges.  Measured: argument 10.66, d_ref = 1.5e-12 m, host twin
    1.1e-12 m."""
    fam = rp.Family(True)
    f = mf.Fleet(1, 64, 6400)
    me.set_timing(f, 0, 0.5, max(mf.SINGLE_TICKS) * f.model.T, f.models[0].t_double)      # the corner of mf.Fleet's ranges: argument 10.66
    assert f.n_steps[0] == 64
    blocks, st = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, 64)
    assert st[0] == 0 and fam.view(blocks[0], 64)["n"] == 264
    d_ref, d_twin = distances(fam, f, blocks, between=40)
    print("argument %.2f: d_ref %.3g, host twin %.3g, bound %.3g" %
          (me.argument(f.com0[0, 2], f.models[0].t_single, f.models[0].t_double), d_ref, d_twin, D_REF_FACTOR * d_ref))
    assert D_REF_FACTOR * d_ref < D_REF_CEILING
    assert d_twin <= D_REF_FACTOR * d_ref


@pytest.mark.parametrize("long_,smax", ((False, 3), (True, 15)))
def test_edge_fleet_refusals_are_per_gait(wg, long_, smax):
    """the edge fleet through the fleet solve: the gaits beyond the bound are refused and keep the caller's pattern, every other gait has
    the bytes it has in a fleet without them"""
    fam = rp.Family(long_)
    f = me.edge_fleet(smax)
    blocks, st = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, smax, blocks=np.full((f.B, fam.words(smax)), rp.PATTERN))
    refused = [b for b in range(f.B) if not f.admitted[b]]
    assert [b for b in range(f.B) if st[b] != 0] == refused and all(st[b] == wg.MORISAWA_BAD_INPUT for b in refused)
    assert all((blocks[b] == rp.PATTERN).all() for b in refused)
    assert any(f.admitted[b - 1] and f.admitted[b + 1] for b in refused if 0 < b < f.B - 1)
    g, keep = me.without(f, refused)
    alone, st = fam.solve(g.models, g.steps, g.n_steps, g.init_feet, g.com0, smax)
    assert list(st) == [0] * g.B
    for i, b in enumerate(keep):
        assert blocks[b].tobytes() == alone[i].tobytes(), b
