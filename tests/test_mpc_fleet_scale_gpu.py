"""Herdt fleets with a model per gait at queue-loading sizes: wg_mpc_tick_fleet_dev / wg_mpc_run_fleet_dev on the fleets of
tests/mixedfleet.py (B = 2600 / 3300 gaits, 16 - 64 models, a refused gait in every 101), every gait against the portable-trig
oracle -- on bytes: the wg_gait_state_t, the six diagnostic ints of every tick, whole wg_tick_out_t records.

tests/test_mpc_fleet_gpu.py holds the same entry points at up to 28 gaits, where every gait has a wave of its own.  Here B
exceeds the waves the device keeps resident, so a wave serves a long sequence of gaits with different models from one LDS area
and one solver slot, the rings of the run kernel fill, the keep rule runs (and counts refused gaits), and the tick launches
take the longest-first start order.

The oracle runs on a pool of spawned host processes (tests/fleet_oracle.py: submit_fleet), queued for all four kinds before the
first GPU call; each test collects what it needs.  tests/test_mpc_fleet_scale_oracle.py proves the recipe on the CPU.

Launch plan of the run cases: ticks 0 and 1 are single wg_mpc_tick_fleet_dev launches (their clock advance differs), ticks
2 .. redraw - 1 one unstaged wg_mpc_run_fleet_dev launch (staged references take effect on launch-relative multiples of the
period, so a staged launch starts on a redraw), the rest -- three stretches -- ONE staged launch."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_oracle as fo  # noqa: E402
import mixedfleet as mf  # noqa: E402
import workload as w  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu
SZ, OSZ = C.sizeof(wg.GaitState), C.sizeof(wg.TickOut)
STATE_WORDS, OUT_WORDS = fo.word_names(wg.GaitState), fo.word_names(wg.TickOut)
DIAG_OFF = wg.TickOut.ifail.offset
VREF_OFF = wg.GaitState.vref.offset
NO_MODEL = np.array([wg.IFAIL_NO_MODEL, 0, 0, 0, 0, 0], dtype=np.int32)
CANARY = 0x5A
HIST_CAP = 64
# The most tick waves the library keeps on a CU in any view: WG_TICK32_WPE = 3 waves per SIMD in the N = 32 view, times the four
# SIMDs of a CU, is 12 (the any-horizon element view keeps no more); the compact view keeps 2 per SIMD, 8 per CU.  A fleet
# larger than that times the CUs cannot have a wave per gait: run_launch's grid is below B and tick_launch orders the start.
WAVES_PER_CU = {"compact": 8, "element16": 12, "n12": 12, "n32": 12}
WAVES_PER_CU_ANY = 12


# ------------------------------------------------------------------------------------------------------------------ fixture
@pytest.fixture(scope="module")
def scale():
    """{kind: its oracle job}, queued on one pool before the first GPU call; the jobs keep every tick's diag and the last two
    ticks' outs as raw bytes"""
    bench = w.bench_module()
    wg.init(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name in mf.KINDS:
        assert mf.kind(name).B > WAVES_PER_CU[name] * cus, (name, mf.kind(name).B, cus)
    fo.build_oracle()
    layout = fo.layout_of(wg)
    workers = fo.pool_size(bench)
    with fo.make_pool(workers) as pool:
        jobs = {}
        for name in mf.KINDS:
            K = mf.kind(name)
            jobs[name] = fo.submit_fleet(pool, layout, K.oracle_models(), K.model_of, K.starts(), K.vel, K.redraw, K.ticks,
                                         keep_ticks=(K.ticks - 2, K.ticks - 1))
        print("\noracle for %s queued on %d processes" % (", ".join(mf.KINDS), workers))
        yield {"jobs": jobs, "results": {}, "fleets": {}, "cus": cus}


def oracle_of(scale, name):
    """the oracle's result of a kind (collected once), checked for what the comparison relies on"""
    if name not in scale["results"]:
        K = mf.kind(name)
        res = scale["jobs"][name].result(timeout=900)
        assert np.array_equal(res["accepted"], K.accepted)
        d = res["diag"][:, K.accepted]
        assert (d[..., 1] > 0).all() and len(np.unique(d[..., 3])) > 1 and len(np.unique(d[..., 1])) > 20      # no vacuous pass
        st = (wg.GaitState * K.B).from_buffer_copy(res["states"])
        assert all(s.tick_count == (K.ticks if K.accepted[g] else 0) for g, s in enumerate(st))
        scale["results"][name] = res
    return scale["results"][name]


class DeviceFleet:
    """the blocks of a kind on the device -- the M good ones made there by wg_mpc_blocks_batch_dev, the extra ones made on
    the host and copied behind them --, model_of and the descriptor, kept alive together"""

    def __init__(self, K):
        bb = wg.mpc_block_bytes()
        arr = (wg.Model * K.M)(*K.models)
        d_models = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
        self.blocks = torch.full((K.n_blocks * bb,), CANARY, dtype=torch.uint8, device="cuda")
        status = torch.full((K.M,), -1, dtype=torch.int32, device="cuda")
        wg.mpc_blocks_batch_dev(K.M, d_models.data_ptr(), self.blocks.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 0).all()
        host = []
        for what, m in K.extras:
            if m is None:
                host.append(np.zeros(bb, dtype=np.uint8))
            else:
                rc, blk = wg.mpc_block(m)
                assert rc == 0, what
                host.append(np.asarray(blk, dtype=np.uint8))
        self.blocks[K.M * bb:] = torch.from_numpy(np.concatenate(host)).cuda()
        self.model_of = torch.from_numpy(K.model_of.copy()).cuda()
        self.B = K.B
        self.desc = wg.mpc_fleet(K.base, K.n_blocks, self.blocks.data_ptr(), self.model_of.data_ptr())
        torch.cuda.synchronize()


def fleet_of(scale, name):
    if name not in scale["fleets"]:
        K = mf.kind(name)
        # the start pose of the oracle's wgo_gait_init is wg_gait_init's, byte for byte
        assert K.model_starts[-1] == w.state_bytes(w.start_state(wg.gait_init, K.models[-1]))
        scale["fleets"][name] = DeviceFleet(K)
    return scale["fleets"][name]


def dev_bytes(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def dev_f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def set_vref(states, vel_row):
    """gait g's reference <- vel_row[g] (wg_mpc_set_velref_dev needs no configured model)"""
    vt = dev_f64(vel_row)
    wg.mpc_set_velref_dev(vel_row.shape[0], states.data_ptr(), vt.data_ptr())
    torch.cuda.synchronize()


def ok(rc):
    assert rc == 0, (rc, wg.lib().wg_last_error())


# --------------------------------------------------------------------------------------------------------------- expectation
def want_states(K, res, seg):
    """the oracle's final states; a refused gait: its start state with the references of stretch `seg`, the last the test
    itself set for it (staged references are not written for a gait that sits its ticks out)"""
    a = np.frombuffer(res["states"], dtype=np.uint8).reshape(K.B, SZ).copy()
    for g in np.flatnonzero(~K.accepted):
        a[g] = np.frombuffer(K.start_of(g), dtype=np.uint8)
        a[g, VREF_OFF:VREF_OFF + 24] = np.frombuffer(K.vel[seg, g].tobytes(), dtype=np.uint8)
    return a.tobytes()


def want_diag(K, res):
    d = res["diag"].copy()
    d[:, ~K.accepted] = NO_MODEL
    return d


def want_outs(K, res, t):
    """the oracle's outs of tick t; a refused gait: WG_IFAIL_NO_MODEL and five zeros in the six ints, the canary elsewhere"""
    a = np.frombuffer(res["outs"][t], dtype=np.uint8).reshape(K.B, OSZ).copy()
    a[~K.accepted] = CANARY
    a[~K.accepted, DIAG_OFF:DIAG_OFF + 24] = np.frombuffer(NO_MODEL.tobytes(), dtype=np.uint8)
    return a.tobytes()


# ------------------------------------------------------------------------------------------------------------------- drivers
def run_case(scale, name, what):
    """Case 1 for one kind (module docstring for the plan).  Then, from a copy of the states after the first stretch, the same
    staged launch two ticks shorter and one more two-tick run launch that stores its outs (tick-major): those two ticks'
    diag and out records and the final states once more."""
    K = mf.kind(name)
    fl = fleet_of(scale, name)
    B, T, R = K.B, K.ticks, K.redraw
    states = dev_bytes(K.starts())
    sp = states.data_ptr()
    dg = torch.full((T, B, 6), 99, dtype=torch.int32, device="cuda")
    set_vref(states, K.vel[0])
    for t in (0, 1):
        ok(wg.mpc_tick_fleet_dev(B, fl.desc, sp, None, dg[t].data_ptr(), w.advance_calls(t)))
    ok(wg.mpc_run_fleet_dev(B, fl.desc, sp, R - 2, 20, None, 1, None, dg[2].data_ptr()))
    torch.cuda.synchronize()
    mid = states.clone()
    sched = dev_f64(K.vel[1:])                                                   # [3, B, 3]: the stretches that start inside the launch
    ok(wg.mpc_run_fleet_dev(B, fl.desc, sp, T - R, 20, sched.data_ptr(), R, None, dg[R].data_ptr()))
    torch.cuda.synchronize()
    res = oracle_of(scale, name)
    fo.assert_diag_equal(want_diag(K, res), dg.cpu().numpy(), "%s: diag" % what)
    fo.assert_records_equal(want_states(K, res, 0), states.cpu().numpy().tobytes(), SZ, "%s: final states" % what, names=STATE_WORDS)

    dg2 = torch.full((2, B, 6), 99, dtype=torch.int32, device="cuda")
    ro = torch.full((2, B * OSZ), CANARY, dtype=torch.uint8, device="cuda")
    mp = mid.data_ptr()
    ok(wg.mpc_run_fleet_dev(B, fl.desc, mp, T - R - 2, 20, sched.data_ptr(), R, None, None))
    ok(wg.mpc_run_fleet_dev(B, fl.desc, mp, 2, 20, None, 1, ro.data_ptr(), dg2.data_ptr()))
    torch.cuda.synchronize()
    fo.assert_diag_equal(want_diag(K, res)[T - 2:], dg2.cpu().numpy(), "%s: diag of the two-tick launch" % what, first_tick=T - 2)
    got = ro.cpu().numpy()
    for k in range(2):
        fo.assert_records_equal(want_outs(K, res, T - 2 + k), got[k].tobytes(), OSZ, "%s: outs of tick %d" % (what, T - 2 + k),
                                names=OUT_WORDS)
    fo.assert_records_equal(want_states(K, res, 0), mid.cpu().numpy().tobytes(), SZ, "%s: final states after the two-tick launch" % what,
                            names=STATE_WORDS)


def per_tick(scale, name):
    """one wg_mpc_tick_fleet_dev launch per tick, the references set by the test at every redraw.  Returns the final states'
    bytes, diag [T, B, 6], the last tick's outs and its add / drop history (hist [B, HIST_CAP], hist_len [B])."""
    K = mf.kind(name)
    fl = fleet_of(scale, name)
    B, T, R = K.B, K.ticks, K.redraw
    states = dev_bytes(K.starts())
    dg = torch.full((T, B, 6), 99, dtype=torch.int32, device="cuda")
    outs = torch.full((B * OSZ,), CANARY, dtype=torch.uint8, device="cuda")
    hist = torch.zeros(B, HIST_CAP, dtype=torch.int32, device="cuda")
    hlen = torch.zeros(B, dtype=torch.int32, device="cuda")
    for t in range(T):
        if t % R == 0:
            set_vref(states, K.vel[t // R])
        last = t == T - 1
        ok(wg.mpc_tick_fleet_dev(B, fl.desc, states.data_ptr(), outs.data_ptr() if last else None, dg[t].data_ptr(), w.advance_calls(t),
                                 hist.data_ptr() if last else None, HIST_CAP if last else 0, hlen.data_ptr() if last else None))
    torch.cuda.synchronize()
    return states.cpu().numpy().tobytes(), dg.cpu().numpy(), outs.cpu().numpy().tobytes(), hist.cpu().numpy(), hlen.cpu().numpy()


def spread_gaits(K, n=64, n_refused=8):
    """n gaits spread over the fleet, n_refused refused ones among them"""
    refused = np.flatnonzero(~K.accepted)
    picked = [int(g) for g in refused[np.linspace(0, len(refused) - 1, n_refused).astype(int)]]
    for g in np.linspace(0, K.B - 2, n - n_refused).astype(int):
        picked.append(int(g) if K.accepted[g] else int(g) + 1)                 # refused gaits have accepted neighbours
    assert len(picked) == n and len(set(picked)) == n
    return sorted(picked)


# --------------------------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize("name", mf.KINDS)
def test_one_run_launch_every_kind(name, scale, monkeypatch):
    monkeypatch.delenv("WG_RUN_KEEP", raising=False)
    run_case(scale, name, "%s fleet" % name)


@pytest.mark.parametrize("keep", ["off", "0", "3"])
@pytest.mark.parametrize("name", ["compact", "n32"])
def test_hand_over_policy_is_scheduling_only(name, keep, scale, monkeypatch):
    """WG_RUN_KEEP = off (the plain ring), 0 (what a loaded launch takes by default) and 3: all three give the oracle's bytes.
    The keep rule's prog / count hold the refused gaits too, whose ticks take no time."""
    monkeypatch.setenv("WG_RUN_KEEP", keep)
    run_case(scale, name, "%s fleet, WG_RUN_KEEP=%s" % (name, keep))


@pytest.mark.parametrize("name", ["compact", "n32"])
def test_one_launch_per_tick_with_the_start_order(name, scale, monkeypatch):
    """B exceeds the resident waves, so every tick launch after the first starts its gaits longest-first by the iteration counts
    of the tick before (a refused gait reports 0); WG_TICK_LPT=0 starts them in index order.  Both equal the oracle."""
    K = mf.kind(name)
    T = K.ticks
    runs = {}
    for lpt in (None, "0"):
        if lpt is None:
            monkeypatch.delenv("WG_TICK_LPT", raising=False)
        else:
            monkeypatch.setenv("WG_TICK_LPT", lpt)
        runs[lpt] = per_tick(scale, name)
    res = oracle_of(scale, name)
    for lpt, (fin, diag, outs, hist, hlen) in runs.items():
        what = "%s fleet, a launch per tick, WG_TICK_LPT %s" % (name, "unset" if lpt is None else "= " + lpt)
        fo.assert_diag_equal(want_diag(K, res), diag, "%s: diag" % what)
        fo.assert_records_equal(want_states(K, res, K.n_seg - 1), fin, SZ, "%s: final states" % what, names=STATE_WORDS)
        fo.assert_records_equal(want_outs(K, res, T - 1), outs, OSZ, "%s: outs of the last tick" % what, names=OUT_WORDS)
    (_, _, _, hist_a, hlen_a), (_, _, _, hist_b, hlen_b) = runs[None], runs["0"]
    assert np.array_equal(hlen_a, hlen_b) and (hlen_a[~K.accepted] == 0).all() and hlen_a.max() > 0
    picked = spread_gaits(K)
    assert sum(not K.accepted[g] for g in picked) == 8
    for g in picked:
        n = min(int(hlen_a[g]), HIST_CAP)
        assert np.array_equal(hist_a[g, :n], hist_b[g, :n]), (name, g)
    assert sum(int(hlen_a[g]) > 0 for g in picked) > len(picked) // 4          # the histories compared are not all empty


@pytest.mark.parametrize("N,B,T", [(16, 4096, 50), (32, 3300, 10)])
def test_one_block_for_everybody_equals_the_configured_context(N, B, T, scale):
    """The benchmark workload (tests/workload.py: the default model, every gait from the one start pose, the references of
    velocity_table redrawn every w.REDRAW ticks) through wg_mpc_run_sched_dev on a configured context and through
    wg_mpc_run_fleet_dev with M = 1, model_of all zero, on a context that was never configured: the same bytes.  HIP against
    HIP; the configured side is what tests/test_fleet_parity_gpu.py holds to the oracle.  Plan: ticks 0 and 1 single launches,
    ticks 2 .. T - 2 one staged run launch with every tick's diag, tick T - 1 a one-tick staged run launch that stores its outs."""
    assert B > WAVES_PER_CU_ANY * scale["cus"] and T <= w.REDRAW
    model = wg.model_defaults()
    model.N = N
    start = w.start_bytes(wg.gait_init, model)
    vtab = dev_f64(w.velocity_table(0, B, 1))                                   # [1, B, 3]

    def plan(tick, run, velref):
        states = w.to_device(start, B)
        sp = states.data_ptr()
        dg = torch.full((T, B, 6), 99, dtype=torch.int32, device="cuda")
        outs = torch.full((B * OSZ,), CANARY, dtype=torch.uint8, device="cuda")
        velref(B, sp, vtab.data_ptr())
        for t in (0, 1):
            tick(sp, dg[t].data_ptr(), w.advance_calls(t))
        run(sp, T - 3, None, dg[2].data_ptr())
        run(sp, 1, outs.data_ptr(), dg[T - 1].data_ptr())
        torch.cuda.synchronize()
        return states.cpu().numpy().tobytes(), dg.cpu().numpy(), outs.cpu().numpy().tobytes()

    with wg.Context(0) as ctx:
        ctx.mpc_configure(model)
        ref = plan(lambda sp, dp, adv: ctx.mpc_tick_batch_dev(B, sp, None, dp, adv),
                   lambda sp, n, op, dp: ctx.mpc_run_sched_dev(B, sp, n, vtab.data_ptr(), w.REDRAW, 20, op, dp),
                   ctx.mpc_set_velref_dev)
    rc, blk = wg.mpc_block(model)
    assert rc == 0
    blocks = torch.from_numpy(np.asarray(blk, dtype=np.uint8).copy()).cuda()
    model_of = torch.zeros(B, dtype=torch.int32, device="cuda")
    desc = wg.mpc_fleet(model, 1, blocks.data_ptr(), model_of.data_ptr())
    with wg.Context(0) as fctx:
        got = plan(lambda sp, dp, adv: ok(wg.mpc_tick_fleet_dev(B, desc, sp, None, dp, adv, ctx=fctx)),
                   lambda sp, n, op, dp: ok(wg.mpc_run_fleet_dev(B, desc, sp, n, 20, vtab.data_ptr(), w.REDRAW, op, dp, ctx=fctx)),
                   fctx.mpc_set_velref_dev)
    what = "one block for everybody, N = %d" % N
    # no vacuous pass: the configured side solved a QP on every tick, and its last launch stored that tick's outs
    assert (ref[1][..., 1] > 0).all() and len(np.unique(ref[1][..., 1])) > 10
    ints = np.frombuffer(ref[2], dtype=np.uint8).reshape(B, OSZ)[:, DIAG_OFF:DIAG_OFF + 24].copy().view(np.int32)
    assert np.array_equal(ints, ref[1][T - 1])
    fo.assert_diag_equal(ref[1], got[1], what)
    fo.assert_records_equal(ref[0], got[0], SZ, "%s: final states" % what, names=STATE_WORDS)
    fo.assert_records_equal(ref[2], got[2], OSZ, "%s: outs of the last tick" % what, names=OUT_WORDS)
