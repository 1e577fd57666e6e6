"""Herdt fleets with a model per gait: wg_mpc_tick_fleet_dev / wg_mpc_run_fleet_dev against the portable-trig oracle and against
configured contexts -- on bytes (the wg_gait_state_t of every gait after every tick, the six diagnostic ints of every tick, the
last tick's whole wg_tick_out_t).  Ticks whose QP fails are compared like any other.

Small fleets: the 7 models of a sweep of tests/modelgen.py, two gaits each (mg.sweep_gaits), 96 ticks, the references redrawn
every 16 ticks.  The oracle traces are made once per sweep (mg.oracle_trace, one model per gait) and shared by the tests.
A refused gait leaves WG_IFAIL_NO_MODEL and five zeros in its six ints and nothing else."""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_oracle as fo  # noqa: E402
import modelgen as mg  # noqa: E402
import workload as w  # noqa: E402
from test_mpc_blocks_host import refused_models  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu
SZ, OSZ = C.sizeof(wg.GaitState), C.sizeof(wg.TickOut)
STATE_WORDS, OUT_WORDS = fo.word_names(wg.GaitState), fo.word_names(wg.TickOut)
DIAG_OFF = wg.TickOut.ifail.offset
N_TICKS, REDRAW, PER_MODEL = 96, 16, 2
NO_MODEL = np.array([wg.IFAIL_NO_MODEL, 0, 0, 0, 0, 0], dtype=np.int32)
CANARY = 0x5A
BAD_ARG = -2


# -------------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def sweep_fleet(name):
    """the fleet of one sweep, with its oracle: models [7], and per gait (two per model, in model order) its model index, its
    references [6, 3], its oracle diag rows [N_TICKS, 6] (diag's order), its state bytes after every tick, its last out struct"""
    pt = w.ptrig()
    models = [m for _, m in mg.sweep_models(name)]
    gaits = []
    for k, m in enumerate(models):
        for vel in mg.sweep_gaits(name, k, PER_MODEL):
            last = wg.TickOut()
            rows, states = mg.oracle_trace(pt, m, vel, N_TICKS, REDRAW, last_out=last)
            assert len(states) == N_TICKS and (rows[:, 0] == 0).all(), (name, k)
            gaits.append(dict(model=k, vel=vel, diag=rows[:, [1, 7, 8, 3, 9, 2]].astype(np.int32), states=states, last=bytes(last)))
    return models, gaits


def start_bytes(model):
    return w.state_bytes(w.start_state(wg.gait_init, model))


class Fleet:
    """blocks of `models` made on the device, an int per gait, the descriptor -- kept alive together"""

    def __init__(self, base, models, model_of, host_blocks=None):
        M = len(models)
        if host_blocks is None:
            arr = (wg.Model * M)(*models)
            d_models = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
            self.blocks = torch.zeros(M * wg.mpc_block_bytes(), dtype=torch.uint8, device="cuda")
            self.status = torch.zeros(M, dtype=torch.int32, device="cuda")
            wg.mpc_blocks_batch_dev(M, d_models.data_ptr(), self.blocks.data_ptr(), self.status.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        else:
            self.blocks = torch.from_numpy(np.concatenate(host_blocks)).cuda()
        self.model_of = torch.tensor(list(model_of), dtype=torch.int32, device="cuda")
        self.B = len(model_of)
        self.desc = wg.mpc_fleet(base, M, self.blocks.data_ptr(), self.model_of.data_ptr())


def set_vref(states, vel_row):
    """gait g's reference <- vel_row[g] (what wg_mpc_set_velref_dev does; it needs no configured model)"""
    vt = torch.from_numpy(np.ascontiguousarray(vel_row, dtype=np.float64)).cuda()
    wg.mpc_set_velref_dev(vel_row.shape[0], states.data_ptr(), vt.data_ptr())
    torch.cuda.synchronize()


def per_tick(fleet, starts, vels, n_ticks=N_TICKS, keep_outs_from=None, ctx=None, hist_cap=0):
    """one wg_mpc_tick_fleet_dev launch per tick on device-resident states.  Returns the state bytes after every tick
    [n_ticks][B * SZ], diag [n_ticks, B, 6], the outs of ticks >= keep_outs_from (default: the last tick) as bytes per tick,
    and (hist, hist_len) of the last tick.  Out buffers start as CANARY bytes."""
    B = fleet.B
    states = torch.frombuffer(bytearray(b"".join(starts)), dtype=torch.uint8).cuda()
    diag = torch.full((n_ticks, B, 6), 99, dtype=torch.int32, device="cuda")
    keep_outs_from = n_ticks - 1 if keep_outs_from is None else keep_outs_from
    outs = torch.full((n_ticks - keep_outs_from, B * OSZ), CANARY, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(B, max(hist_cap, 1), dtype=torch.int32, device="cuda")
    hlen = torch.zeros(B, dtype=torch.int32, device="cuda")
    after = []
    for t in range(n_ticks):
        if t % REDRAW == 0:
            set_vref(states, np.stack([v[t // REDRAW] for v in vels]))
        op = outs[t - keep_outs_from].data_ptr() if t >= keep_outs_from else None
        rc = wg.mpc_tick_fleet_dev(B, fleet.desc, states.data_ptr(), op, diag[t].data_ptr(), w.advance_calls(t),
                                   hist.data_ptr() if hist_cap else None, hist_cap, hlen.data_ptr() if hist_cap else None, ctx=ctx)
        assert rc == 0, (rc, wg.lib().wg_last_error())
        torch.cuda.synchronize()
        after.append(states.cpu().numpy().tobytes())
    return after, diag.cpu().numpy(), [o.cpu().numpy().tobytes() for o in outs], (hist.cpu().numpy(), hlen.cpu().numpy())


def with_vref(state, vel):
    """a state's bytes with its references replaced: what the test's own set-velref leaves of a gait no tick touches"""
    b = bytearray(state)
    off = wg.GaitState.vref.offset
    b[off:off + 24] = np.asarray(vel, dtype=np.float64).tobytes()
    return bytes(b)


def hold_to_oracle(what, gaits, accepted, after, diag, last_outs, starts):
    """accepted gaits: state bytes and diag of every tick, the last tick's out struct, against the oracle; refused ones: the
    start state after every tick (with the references the test itself set), WG_IFAIL_NO_MODEL and five zeros in diag and in
    the out struct, the canary everywhere else"""
    B = len(gaits)
    for t in range(len(after)):
        want = b"".join(gaits[g]["states"][t] if accepted[g] else with_vref(starts[g], gaits[g]["vel"][t // REDRAW]) for g in range(B))
        fo.assert_records_equal(want, after[t], SZ, "%s, tick %d" % (what, t), names=STATE_WORDS)
        rows = np.stack([gaits[g]["diag"][t] if accepted[g] else NO_MODEL for g in range(B)])
        assert np.array_equal(diag[t], rows), (what, t, diag[t], rows)
    canary = bytearray([CANARY]) * OSZ
    canary[DIAG_OFF:DIAG_OFF + 24] = NO_MODEL.tobytes()
    want = b"".join(gaits[g]["last"] if accepted[g] else bytes(canary) for g in range(B))
    if len(after) == N_TICKS:
        fo.assert_records_equal(want, last_outs, OSZ, "%s, outs of the last tick" % what, names=OUT_WORDS)


def sweep_launch(name, base, **kw):
    models, gaits = sweep_fleet(name)
    fleet = Fleet(base, models, [g["model"] for g in gaits])
    assert (fleet.status.cpu().numpy() == 0).all()
    starts = [start_bytes(models[g["model"]]) for g in gaits]
    after, diag, outs, _ = per_tick(fleet, starts, [g["vel"] for g in gaits], **kw)
    return models, gaits, fleet, starts, after, diag, outs


# ------------------------------------------------------------------------------------------------------ 1, 2. the sweeps
def test_compact_fleet():
    wg.init(0)
    base = mg.defaults(16)
    assert int(wg.lib().wg_mpc_tick_lds_bytes_for(C.byref(base))) == 20240
    models, gaits, fleet, starts, after, diag, outs = sweep_launch("16c", base)
    assert len(gaits) == 14
    hold_to_oracle("16c fleet", gaits, [True] * 14, after, diag, outs[-1], starts)


@pytest.mark.parametrize("name", ["16e", "12", "32"])
def test_element_fleets(name):
    wg.init(0)
    models, _ = sweep_fleet(name)
    base = models[0]
    assert 0 < int(wg.lib().wg_mpc_tick_lds_bytes_for(C.byref(base))) <= 12800
    models, gaits, fleet, starts, after, diag, outs = sweep_launch(name, base)
    hold_to_oracle("%s fleet" % name, gaits, [True] * 14, after, diag, outs[-1], starts)
    if name == "16e":
        assert diag[:, :, 5].max() == 4


# ----------------------------------------------------------------------------------------- 3. both classes in one launch
def _both_classes(base):
    me, ge = sweep_fleet("16e")
    mc, gc = sweep_fleet("16c")
    gaits = list(ge) + [dict(g, model=g["model"] + 7) for g in gc]
    fleet = Fleet(base, me + mc, [g["model"] for g in gaits])
    starts = [start_bytes((me + mc)[g["model"]]) for g in gaits]
    return gaits, fleet, starts


def test_both_step_classes_in_one_element_launch():
    wg.init(0)
    gaits, fleet, starts = _both_classes(sweep_fleet("16e")[0][0])
    after, diag, outs, _ = per_tick(fleet, starts, [g["vel"] for g in gaits])
    hold_to_oracle("16e + 16c in the element view", gaits, [True] * 28, after, diag, outs[-1], starts)


def test_a_compact_launch_refuses_the_four_step_class():
    wg.init(0)
    gaits, fleet, starts = _both_classes(mg.defaults(16))
    after, diag, outs, _ = per_tick(fleet, starts, [g["vel"] for g in gaits])
    hold_to_oracle("16e + 16c in the compact view", gaits, [False] * 14 + [True] * 14, after, diag, outs[-1], starts)


# ---------------------------------------------------------------------------------------------------------- 4. run form
@pytest.mark.parametrize("name", ["16c", "12"])
def test_run_form_against_the_per_tick_launches(name):
    """wg_mpc_run_fleet_dev on device-resident states: once with the references staged (vref_sched, period 16), once as
    set-velref plus an unstaged run per stretch; final states and all diag rows equal the per-tick launches', the outs of one
    run launch (tick-major) the per-tick outs.  The control loop's first two ticks are single-tick launches in every plan
    (their clock advance differs), the first stretch therefore ends with an unstaged run of 14 ticks."""
    wg.init(0)
    models, _ = sweep_fleet(name)
    base = mg.defaults(16) if name == "16c" else models[0]
    last_stretch = N_TICKS - REDRAW
    models, gaits, fleet, starts, after, diag, outs = sweep_launch(name, base, keep_outs_from=last_stretch)
    hold_to_oracle("%s fleet" % name, gaits, [True] * 14, after, diag, outs[-1], starts)
    B = fleet.B
    vt = np.stack([np.stack([g["vel"][k] for g in gaits]) for k in range(N_TICKS // REDRAW)])         # [seg, B, 3]
    for staged in (True, False):
        what = "%s fleet, %s run" % (name, "staged" if staged else "unstaged")
        states = torch.frombuffer(bytearray(b"".join(starts)), dtype=torch.uint8).cuda()
        dg = torch.full((N_TICKS, B, 6), 99, dtype=torch.int32, device="cuda")
        ro = torch.full((REDRAW, B * OSZ), CANARY, dtype=torch.uint8, device="cuda")
        sp = states.data_ptr()
        set_vref(states, vt[0])
        for t in (0, 1):
            assert wg.mpc_tick_fleet_dev(B, fleet.desc, sp, None, dg[t].data_ptr(), w.advance_calls(t)) == 0
        assert wg.mpc_run_fleet_dev(B, fleet.desc, sp, REDRAW - 2, 20, None, 1, None, dg[2].data_ptr()) == 0
        if staged:
            sched = torch.from_numpy(np.ascontiguousarray(vt[1:-1])).cuda()
            assert wg.mpc_run_fleet_dev(B, fleet.desc, sp, last_stretch - REDRAW, 20, sched.data_ptr(), REDRAW, None,
                                        dg[REDRAW].data_ptr()) == 0
            sched2 = torch.from_numpy(np.ascontiguousarray(vt[-1:])).cuda()
            assert wg.mpc_run_fleet_dev(B, fleet.desc, sp, REDRAW, 20, sched2.data_ptr(), REDRAW, ro.data_ptr(),
                                        dg[last_stretch].data_ptr()) == 0
        else:
            for k in range(1, N_TICKS // REDRAW):
                torch.cuda.synchronize()
                set_vref(states, vt[k])
                assert wg.mpc_run_fleet_dev(B, fleet.desc, sp, REDRAW, 20, None, 1, ro.data_ptr() if k * REDRAW == last_stretch else None,
                                            dg[k * REDRAW].data_ptr()) == 0
        torch.cuda.synchronize()
        fo.assert_records_equal(after[-1], states.cpu().numpy().tobytes(), SZ, what, names=STATE_WORDS)
        fo.assert_diag_equal(diag, dg.cpu().numpy(), what)
        got = ro.cpu().numpy()
        for k in range(REDRAW):
            fo.assert_records_equal(outs[k], got[k].tobytes(), OSZ, "%s, outs of tick %d" % (what, last_stretch + k), names=OUT_WORDS)


# ------------------------------------------------------------------------------------------------------ 5. refused gaits
def _refusal_fleet():
    """the 16c fleet's first three models (gaits 0 .. 5 of the sweep) with refused gaits between them: model_of = -1, = M, a
    failed (all-zero) block, a good block of another N, a good block of another T"""
    models, gaits = sweep_fleet("16c")
    other_n = mg.horizon_model(12)
    other_t = mg.defaults(16, T=0.05)
    assert wg.mpc_block(other_t)[0] == 0
    blocks = [wg.mpc_block(m)[1] for m in models[:3]] + [np.zeros(wg.mpc_block_bytes(), dtype=np.uint8), wg.mpc_block(other_n)[1],
                                                         wg.mpc_block(other_t)[1]]
    M = len(blocks)
    #            ok  -1  ok  M  ok  failed ok  other N  ok  other T  ok
    model_of = [0, -1, 0, M, 1, 3, 1, 4, 2, 5, 2]
    src = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5]                                     # whose references and start state the gait has
    fl_gaits = [gaits[s] for s in src]
    accepted = [mo in (0, 1, 2) for mo in model_of]
    fleet = Fleet(mg.defaults(16), [None] * M, model_of, host_blocks=blocks)
    starts = [start_bytes(models[g["model"]]) for g in fl_gaits]
    return fl_gaits, accepted, fleet, starts


def test_refused_gaits_in_tick_launches():
    wg.init(0)
    gaits, accepted, fleet, starts = _refusal_fleet()
    assert accepted.count(False) == 5
    after, diag, outs, _ = per_tick(fleet, starts, [g["vel"] for g in gaits])
    hold_to_oracle("refused gaits, per-tick launches", gaits, accepted, after, diag, outs[-1], starts)


def test_refused_gaits_in_run_launches():
    wg.init(0)
    gaits, accepted, fleet, starts = _refusal_fleet()
    B = fleet.B
    n = 2 * REDRAW
    states = torch.frombuffer(bytearray(b"".join(starts)), dtype=torch.uint8).cuda()
    dg = torch.full((n, B, 6), 99, dtype=torch.int32, device="cuda")
    ro = torch.full((REDRAW, B * OSZ), CANARY, dtype=torch.uint8, device="cuda")
    sp = states.data_ptr()
    vt = np.stack([np.stack([g["vel"][k] for g in gaits]) for k in range(2)])
    set_vref(states, vt[0])
    for t in (0, 1):
        assert wg.mpc_tick_fleet_dev(B, fleet.desc, sp, None, dg[t].data_ptr(), w.advance_calls(t)) == 0
    assert wg.mpc_run_fleet_dev(B, fleet.desc, sp, REDRAW - 2, 20, None, 1, None, dg[2].data_ptr()) == 0
    sched = torch.from_numpy(np.ascontiguousarray(vt[1:])).cuda()
    assert wg.mpc_run_fleet_dev(B, fleet.desc, sp, REDRAW, 20, sched.data_ptr(), REDRAW, ro.data_ptr(), dg[REDRAW].data_ptr()) == 0
    torch.cuda.synchronize()
    fin = states.cpu().numpy().tobytes()
    # a refused gait keeps the references the test's own set-velref gave it: the second stretch's are never staged for it
    want = b"".join(gaits[g]["states"][n - 1] if accepted[g] else with_vref(starts[g], vt[0][g]) for g in range(B))
    fo.assert_records_equal(want, fin, SZ, "refused gaits, run launches", names=STATE_WORDS)
    rows = np.stack([np.stack([gaits[g]["diag"][t] if accepted[g] else NO_MODEL for g in range(B)]) for t in range(n)])
    fo.assert_diag_equal(rows, dg.cpu().numpy(), "refused gaits, run launches")
    got = ro.cpu().numpy().reshape(REDRAW, B, OSZ)
    canary = bytearray([CANARY]) * OSZ
    canary[DIAG_OFF:DIAG_OFF + 24] = NO_MODEL.tobytes()
    for g in range(B):
        if not accepted[g]:
            assert all(got[k, g].tobytes() == bytes(canary) for k in range(REDRAW)), g
        else:
            ints = got[:, g, DIAG_OFF:DIAG_OFF + 24].copy().view(np.int32)
            assert np.array_equal(ints, gaits[g]["diag"][REDRAW:n]), g


def test_host_side_refusals_leave_the_states_untouched():
    wg.init(0)
    gaits, accepted, fleet, starts = _refusal_fleet()
    B = fleet.B
    states = torch.frombuffer(bytearray(b"".join(starts)), dtype=torch.uint8).cuda()
    sp = states.data_ptr()
    d = fleet.desc
    bad_base = wg.mpc_fleet(refused_models()[2][1], d.M, d.blocks, d.model_of)
    assert wg.mpc_block(bad_base.base)[0] == BAD_ARG
    cases = [("NULL fleet", B, None), ("NULL blocks", B, wg.mpc_fleet(d.base, d.M, None, d.model_of)),
             ("NULL model_of", B, wg.mpc_fleet(d.base, d.M, d.blocks, None)), ("M = 0", B, wg.mpc_fleet(d.base, 0, d.blocks, d.model_of)),
             ("B = -1", -1, d), ("a refused base", B, bad_base)]
    for what, b, f in cases:
        assert wg.mpc_tick_fleet_dev(b, f, sp, None, None, 20) == BAD_ARG, what
        assert wg.mpc_run_fleet_dev(b, f, sp, 4, 20) == BAD_ARG, what
    assert wg.mpc_tick_fleet_dev(0, d, sp, None, None, 20) == 0 and wg.mpc_run_fleet_dev(0, d, sp, 4, 20) == 0
    torch.cuda.synchronize()
    assert states.cpu().numpy().tobytes() == b"".join(starts)


# ------------------------------------------------------------------------------------ 6. against configured contexts
def test_contract_against_configured_contexts():
    """three models of "16c" on three contexts through wg_mpc_tick_batch_dev_ctx, and one fleet launch per tick on a fourth
    context that was never configured: the same states, outs, diag and hist rows.  Then wg_mpc_reserve on the fleet's context
    (which sizes by a configured model: the base) is honoured by the fleet launches that follow."""
    wg.init(0)
    models, gaits = sweep_fleet("16c")
    n_ticks, cap = 24, 64
    use = [g for g in gaits if g["model"] < 3]                                  # six gaits, two per model
    B = len(use)
    starts = [start_bytes(models[g["model"]]) for g in use]
    ref_states, ref_outs, ref_diag, ref_hist, ref_hlen = [], [], [], [], []
    for k in range(3):
        with wg.Context(0) as ctx:
            ctx.mpc_configure(models[k])
            idx = [i for i, g in enumerate(use) if g["model"] == k]
            st = torch.frombuffer(bytearray(b"".join(starts[i] for i in idx)), dtype=torch.uint8).cuda()
            outs = torch.zeros(len(idx) * OSZ, dtype=torch.uint8, device="cuda")
            dg = torch.zeros(n_ticks, len(idx), 6, dtype=torch.int32, device="cuda")
            hist = torch.zeros(len(idx), cap, dtype=torch.int32, device="cuda")
            hlen = torch.zeros(len(idx), dtype=torch.int32, device="cuda")
            for t in range(n_ticks):
                if t % REDRAW == 0:
                    set_vref(st, np.stack([use[i]["vel"][t // REDRAW] for i in idx]))
                ctx.mpc_tick_batch_dev(len(idx), st.data_ptr(), outs.data_ptr(), dg[t].data_ptr(), w.advance_calls(t), hist.data_ptr(),
                                       cap, hlen.data_ptr())
            torch.cuda.synchronize()
            ref_states.append(st.cpu().numpy().tobytes()); ref_outs.append(outs.cpu().numpy().tobytes())
            ref_diag.append(dg.cpu().numpy()); ref_hist.append(hist.cpu().numpy()); ref_hlen.append(hlen.cpu().numpy())
    fleet = Fleet(mg.defaults(16), models[:3], [g["model"] for g in use])
    with wg.Context(0) as fctx:
        after, diag, outs, (hist, hlen) = per_tick(fleet, starts, [g["vel"] for g in use], n_ticks=n_ticks, ctx=fctx, hist_cap=cap)
        fo.assert_records_equal(b"".join(ref_states), after[-1], SZ, "fleet against configured contexts", names=STATE_WORDS)
        fo.assert_records_equal(b"".join(ref_outs), outs[-1], OSZ, "fleet against configured contexts, outs", names=OUT_WORDS)
        fo.assert_diag_equal(np.concatenate(ref_diag, axis=1), diag, "fleet against configured contexts")
        assert np.array_equal(np.concatenate(ref_hlen), hlen) and hlen.max() > 0
        assert np.array_equal(np.concatenate(ref_hist), hist)
        hold_to_oracle("fleet on an unconfigured context", use, [True] * B, after, diag, outs[-1], starts)
        # reserve needs a configured model to size by; the fleet launches then find their slots and run buffer in place
        fctx.mpc_configure(mg.defaults(16))
        before = int(fctx.call("wg_overlap_serialised"))
        assert fctx.call("wg_mpc_reserve", B) == 0
        again, diag2, _, _ = per_tick(fleet, starts, [g["vel"] for g in use], n_ticks=n_ticks, ctx=fctx)
        assert again[-1] == after[-1] and np.array_equal(diag, diag2)
        st = torch.frombuffer(bytearray(b"".join(starts)), dtype=torch.uint8).cuda()
        assert wg.mpc_run_fleet_dev(B, fleet.desc, st.data_ptr(), 4, 20, ctx=fctx) == 0, wg.lib().wg_last_error()
        torch.cuda.synchronize()
        assert int(fctx.call("wg_overlap_serialised")) == before
