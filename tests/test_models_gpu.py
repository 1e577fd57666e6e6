"""The tick kernels against the portable-trig oracle across MODELS: every horizon wg_mpc_configure accepts, both sides of
the view selection at N = 16, a seeded sweep over every wg_model_t field (tests/modelgen.py; its inputs are proved good on
the CPU by tests/test_models_oracle.py), and the limit of four previewed steps.

Every comparison is on bytes: the wg_gait_state_t of every gait after EVERY tick, the six diagnostic ints of every tick
(ifail, iterations, active-set size, n, m, previewed steps) and the last tick's whole wg_tick_out_t.  Ticks whose QP fails
(ifail != 0) are compared like any other."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_oracle as fo  # noqa: E402
import modelgen as mg  # noqa: E402
import workload as w  # noqa: E402
from test_models_oracle import FIRST_REFUSED, LAST_ACCEPTED, SCAN  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu
SZ, OSZ = C.sizeof(wg.GaitState), C.sizeof(wg.TickOut)
COMPACT_LDS, ELEMENT_LDS_MAX = 20240, 12800
STATE_WORDS, OUT_WORDS = fo.word_names(wg.GaitState), fo.word_names(wg.TickOut)
DIAG_OFF = wg.TickOut.ifail.offset


def _lds(model):
    return int(wg.lib().wg_mpc_tick_lds_bytes_for(C.byref(model)))


def _follow(model, vels, n_ticks, redraw, what):
    """The gaits with references vels[g] ([n_seg, 3], redrawn every `redraw` ticks) through wg_mpc_tick_batch, one launch per
    tick, on the model as configured by the caller: state bytes and diag after every tick and the last tick's outs against
    the oracle.  Returns (diag [n_ticks, B, 6], final state bytes per gait)."""
    pt = w.ptrig()
    B = len(vels)
    st = w.start_array(wg.gait_init, model, B)
    assert w.state_bytes(st[0]) == w.state_bytes(mg.start_state(model))       # the two libraries' start states are one
    last = [wg.TickOut() for _ in range(B)]
    ref = [mg.oracle_trace(pt, model, vels[g], n_ticks, redraw, last_out=last[g]) for g in range(B)]
    for g in range(B):
        assert len(ref[g][1]) == n_ticks and (ref[g][0][:, 0] == 0).all(), (what, g)
    diags = np.zeros((n_ticks, B, 6), dtype=np.int32)
    outs = None
    for t in range(n_ticks):
        if t % redraw == 0:
            for g in range(B):
                st[g].vref[0], st[g].vref[1], st[g].vref[2] = vels[g][t // redraw]
        outs, diag, _, _ = wg.mpc_tick_batch(st, want_out=(t == n_ticks - 1), advance_calls=w.advance_calls(t))
        diags[t] = diag
        want = b"".join(ref[g][1][t] for g in range(B))
        fo.assert_records_equal(want, w.state_bytes(st), SZ, "%s, tick %d" % (what, t), names=STATE_WORDS)
        rows = np.stack([ref[g][0][t] for g in range(B)])
        assert np.array_equal(diag, rows[:, [1, 7, 8, 3, 9, 2]].astype(np.int32)), (what, t, diag, rows)      # diag's order
    fo.assert_records_equal(b"".join(bytes(o) for o in last), bytes(outs), OSZ, "%s, outs of the last tick" % what, names=OUT_WORDS)
    got = np.frombuffer(bytes(outs), dtype=np.int32).reshape(B, -1)[:, DIAG_OFF // 4:DIAG_OFF // 4 + 6]
    assert np.array_equal(got, diags[-1]), what                                # diag is the outs' six ints
    return diags, [ref[g][1][-1] for g in range(B)]


def _configured(model):
    class _Scope:
        def __enter__(self):
            wg.mpc_configure(model)

        def __exit__(self, *a):
            wg.mpc_configure(wg.model_defaults())
    return _Scope()


# ------------------------------------------------------------------------------------------------------- 1. every horizon
@pytest.mark.parametrize("N", list(range(2, 33)))
def test_every_horizon_through_the_view_configure_picks(N):
    """N = 2 .. 32, odd ones and the neighbours of every layout decision included: TickLds::elem_overlay_apart (apart up to
    N = 12: 10 576 B of LDS there, 7 696 B at 13), the compact horizon 16 and the first ones above it, one or two rows
    per lane (n > 64: N = 29 on), the column cap of R and the n | 1 leading dimension of Z, which the host computes per
    model."""
    wg.init(0)
    model = mg.horizon_model(N)
    lds = _lds(model)
    assert lds == COMPACT_LDS if N == 16 else 0 < lds <= ELEMENT_LDS_MAX, lds
    n_ticks = mg.HORIZON_STRETCH_TICKS * len(mg.HORIZON_STRETCHES)
    with _configured(model):
        diags, _ = _follow(model, mg.gaits(N, 4, mg.HORIZON_STRETCHES), n_ticks, mg.HORIZON_STRETCH_TICKS, "N = %d" % N)
    most = mg.max_previewed_steps(N, model.T, model.step_period)
    assert diags[:, :, 5].max() == most and (diags[:, :, 3] == 2 * N + 2 * diags[:, :, 5]).all()
    assert (diags[:, :, 0] == 0).all()


# --------------------------------------------------------------------------------------------- 2. the view, by the model
@pytest.mark.parametrize("step_period", mg.VIEW_STEP_PERIODS)
def test_view_selection_by_the_step_period_at_the_benchmark_horizon(step_period):
    """tick_compact: the compact view iff N == 16 and N T <= 2 step_period -- both sides of it chosen by the MODEL (not by
    WG_TICK_VIEW): one previewed step at most from 1.6 s on, two down to 0.8 s (compact), three and four below (element)."""
    wg.init(0)
    assert not os.environ.get("WG_TICK_VIEW") and not os.environ.get("WG_TICK_DENSE")
    model = mg.view_model(step_period)
    lds = _lds(model)
    if step_period >= 0.8:
        assert lds == COMPACT_LDS, lds
    else:
        assert 0 < lds <= ELEMENT_LDS_MAX, lds
    seg = mg.stretch_ticks(model)
    with _configured(model):
        assert wg.mpc_tick_lds_bytes() == lds
        diags, _ = _follow(model, mg.gaits(int(step_period * 100), 3, mg.HORIZON_STRETCHES), 2 * seg, seg,
                           "step_period = %g" % step_period)
    want = {2.0: 1, 1.6: 1, 1.0: 2, 0.8: 2, 0.75: 2, 0.7: 3, 0.5: 3, 0.4: 4}[step_period]
    assert diags[:, :, 5].max() == want                                       # 3 and 4 really appeared on the element side
    if step_period >= 1.6:
        assert diags[:, :, 5].max() <= 1


# ------------------------------------------------------------------------------------------------------ 3. the model sweep
@pytest.mark.parametrize("name", mg.SWEEP_NAMES)
def test_model_sweep_per_tick_and_in_multi_tick_launches(name):
    """every field of wg_model_t moved (tests/modelgen.py), gaits that walk, turn into the hip limits, stop and walk again:
    per-tick launches against the oracle, then the same gaits on device-resident states through wg_mpc_run_batch_dev (one
    launch per stretch of the references, tests/workload.py:run_dev) -- which must end in the same bytes"""
    wg.init(0)
    seen = set()
    try:
        for k, (mname, model) in enumerate(mg.sweep_models(name)):
            lds = _lds(model)
            assert lds == COMPACT_LDS if name == "16c" else 0 < lds <= ELEMENT_LDS_MAX, (mname, lds)
            vels = mg.sweep_gaits(name, k)
            seg = mg.stretch_ticks(model)
            n_ticks = seg * len(mg.STRETCHES)
            wg.mpc_configure(model)
            diags, fin = _follow(model, vels, n_ticks, seg, "%s / %s" % (name, mname))
            seen |= set(int(v) for v in diags[:, :, 5].ravel())
            fin_dev, diag_dev = w.run_dev(wg, model, list(range(len(vels))), n_ticks, vel=np.stack(vels, 1), redraw=seg)
            fo.assert_records_equal(b"".join(fin), fin_dev.tobytes(), SZ, "%s / %s, multi-tick launches" % (name, mname),
                                    names=STATE_WORDS)
            fo.assert_diag_equal(diags, diag_dev, "%s / %s, multi-tick launches" % (name, mname))
    finally:
        wg.mpc_configure(wg.model_defaults())
    N = dict((c[0], c[1]) for c in mg.SWEEP)[name]
    most = max(mg.max_previewed_steps(N, m.T, m.step_period) for _, m in mg.sweep_models(name))
    assert seen == set(range(most + 1)), (name, seen)


# ------------------------------------------------------------------------------------------ 4. more than four previewed steps
@pytest.mark.parametrize("N", [16, 32])
def test_the_last_step_period_within_four_previewed_steps_runs_bit_exact(N):
    wg.init(0)
    model = mg.defaults(N)
    mg.set_step_period(model, LAST_ACCEPTED[N])
    assert SCAN[N][LAST_ACCEPTED[N]] == 4 and 0 < _lds(model) <= ELEMENT_LDS_MAX
    n_ticks = int(np.ceil((model.dsss_period + 3.0 * model.step_period) / model.T)) + 2
    vels = [np.array([[0.2, 0.0, 0.0]])] + [v[:1] for v in mg.gaits(N, 3, ("walk",))]     # the scan's own gait first
    with _configured(model):
        diags, _ = _follow(model, vels, n_ticks, n_ticks, "N = %d, step_period = %g" % (N, LAST_ACCEPTED[N]))
    assert diags[:, 0, 5].max() == 4 and diags[:, :, 5].max() == 4


@pytest.mark.parametrize("N", [16, 32])
def test_models_that_preview_more_than_four_steps_are_refused(N):
    """the kernels hold kSMax = 4 previewed steps; a model whose horizon can hold a fifth would be solved as a silently
    truncated QP.  wg_mpc_configure refuses every grid point at which the oracle saw more than four (the CPU scan), names
    step_period, and leaves the configured model as it was."""
    wg.init(0)
    wg.mpc_configure(wg.model_defaults())
    lds0 = wg.mpc_tick_lds_bytes()
    for p, seen in SCAN[N].items():
        model = mg.defaults(N)
        mg.set_step_period(model, p)
        rc = wg.lib().wg_mpc_configure(C.byref(model))
        if seen > mg.S_MAX:
            assert rc == -2, (N, p, seen, rc)                                  # WG_ERR_BAD_ARG
            assert "step_period" in wg.lib().wg_last_error().decode(), wg.lib().wg_last_error()
            assert _lds(model) == 0
            assert wg.mpc_tick_lds_bytes() == lds0                             # still the default model
        else:
            assert rc == 0, (N, p, seen, wg.lib().wg_last_error())
            wg.mpc_configure(wg.model_defaults())
    first = mg.defaults(N)
    mg.set_step_period(first, FIRST_REFUSED[N])
    with pytest.raises(wg.WgError, match="step_period"):
        wg.mpc_configure(first)
    wg.mpc_configure(wg.model_defaults())
