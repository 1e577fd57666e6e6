"""wg_dimitrov_follow_dev: the Dimitrov walk with a clock and a tick count per gait, over exactly the ticks each gait's own queue
has made safe.  The contract is equality with what the project already computes: whatever the calls and their cuts, states[b],
rows [0, ticks[b]) of outs and ran_out[b] (as an OR) are the bytes ONE wg_dimitrov_walk_dev(t0 = the gait's initial clock,
n_ticks = ticks[b]) over the gait's final queue leaves; everything else keeps its canary.  Every comparison is byte equality.

The reference walks write into outs pre-filled with the same canary as the follow calls': a tick whose solver fails leaves the
interpolated rows of its out struct unwritten, so those bytes are the pre-fill's on both sides.  States and ran_out of the
canary-filled reference are held to tests/test_dimitrov_walk_gpu.py's device_walk once per case.

Shapes: the 70-gait fleet70(0.7, 0.13) (64 + 6: four-wave select blocks and a partial one), QCAP = 64, 60 ticks -- at the 25
ticks of the existing on-line tests every gait is safe after its first call (tests/test_dimitrov_follow_host.py)."""
import ctypes as C
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_zmpdisc_online_gpu import Fleet, Walk  # noqa: E402
from test_dimitrov_walk_gpu import (BF, FILL_I, OSZ, QCAP, SMAX, SOLE, SSZ, _setup_dimitrov, _stream, device_queues,  # noqa: E402
                                    device_walk, fleet70, fresh_states, times, to_dev)
from test_footcons_online_gpu import new_queues, poison_past_length  # noqa: E402
from test_dimitrov_follow_host import N_TICKS, feeding, replay, safe_ticks  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
gpu = pytest.mark.gpu

CANARY = 0x5C                                  # outs before any call
BAD = -2                                       # WG_ERR_BAD_ARG
FINAL = 1                                      # WG_DIMITROV_FOLLOW_ALL_FINAL


@pytest.fixture(scope="module")
def fleet():
    """fleet70(0.7, 0.13) through wg_zmpdisc_full_batch_dev -> wg_foot_constraints_batch_dev: the final queues"""
    import torch
    wg.init(0)
    fl = fleet70(0.7, 0.13)
    zm, steps, n_steps, init = fl
    f = Fleet(zm, steps, n_steps, init, SMAX, check_oracle=False)
    time = torch.from_numpy(times(f.lcap, zm.T)).cuda()
    F = dict(B=f.B, lcap=f.lcap, ln=f.full["length"], time=time, lf=f.full["left"], lty=f.full["left_type"], rf=f.full["right"])
    return dict(fl=fl, f=f, time=time, Q=device_queues(F), refs={})


def arrays(B, tick_cap, clock0=None, ran_fill=FILL_I):
    """fresh states, a clock and a tick count per gait, outs and ran_out holding their canaries"""
    import torch
    clock = torch.zeros(B, dtype=torch.float64, device="cuda") if clock0 is None else torch.from_numpy(np.asarray(clock0, np.float64)).cuda()
    return dict(B=B, tick_cap=tick_cap, st=to_dev(fresh_states(B)), clock=clock, ticks=torch.zeros(B, dtype=torch.int32, device="cuda"),
                outs=torch.full((tick_cap, B * OSZ), CANARY, dtype=torch.uint8, device="cuda"),
                ran=torch.full((B,), ran_fill, dtype=torch.int32, device="cuda"))


def follow(Q, A, time_t, have_t, max_ticks, flags=0, walk=None, lcap=None, rc=0, **over):
    """one wg_dimitrov_follow_dev through the raw C ABI; `over` replaces single arguments (B, qcap, tick_cap, or a pointer by name)"""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    a = dict(B=A["B"], qcap=Q["qcap"], queues=p(Q["queues"]), ts=p(Q["ts"]), te=p(Q["te"]), count=p(Q["count"]),
             lcap=int(time_t.shape[0]) if lcap is None else lcap, time=p(time_t), have=p(have_t), walk=p(walk), flags=flags, clock=p(A["clock"]),
             ticks=p(A["ticks"]), tick_cap=A["tick_cap"], max_ticks=max_ticks, st=p(A["st"]), outs=p(A["outs"]), ran=p(A["ran"]))
    a.update(over)
    got = wg.lib().wg_dimitrov_follow_dev(a["B"], a["qcap"], a["queues"], a["ts"], a["te"], a["count"], a["lcap"], a["time"], a["have"],
                                          a["walk"], a["flags"], a["clock"], a["ticks"], a["tick_cap"], a["max_ticks"], a["st"],
                                          a["outs"], a["ran"], 0, _stream())
    assert got == rc, (got, wg.lib().wg_last_error())


def ref_walk(Q, n_ticks, t0=0.0, B=None):
    """ONE wg_dimitrov_walk_dev from fresh states at t0, outs pre-filled with the canary: (states, outs, ran_out) on the host"""
    import torch
    B = B or Q["B"]
    st = to_dev(fresh_states(B))
    outs = torch.full((n_ticks, B * OSZ), CANARY, dtype=torch.uint8, device="cuda")
    ran = torch.full((B,), FILL_I, dtype=torch.int32, device="cuda")
    wg.dimitrov_walk_dev(B, Q["qcap"], Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(), Q["count"].data_ptr(), t0, n_ticks,
                         st.data_ptr(), outs.data_ptr(), ran.data_ptr(), 0, _stream())
    torch.cuda.synchronize()
    return st.cpu().numpy().reshape(B, SSZ), outs.cpu().numpy().reshape(n_ticks, B, OSZ), ran.cpu().numpy()


def final_ref(fleet, key, B=BF):
    """the reference of the whole fleet at t0 = 0 over N_TICKS ticks, once per configured model (key); held to device_walk"""
    k = (key, B)
    if k not in fleet["refs"]:
        st, outs, ran = ref_walk(fleet["Q"], N_TICKS, B=B)
        st0, _, ran0 = device_walk(fleet["Q"], N_TICKS, B=B)
        assert st0.cpu().numpy().tobytes() == st.tobytes() and np.array_equal(ran0.cpu().numpy(), ran)
        fleet["refs"][k] = (st, outs, ran)
    return fleet["refs"][k]


def host(A):
    import torch
    torch.cuda.synchronize()
    B = A["B"]
    return dict(st=A["st"].cpu().numpy().reshape(B, SSZ), outs=A["outs"].cpu().numpy().reshape(A["tick_cap"], B, OSZ),
                ran=A["ran"].cpu().numpy(), clock=A["clock"].cpu().numpy(), ticks=A["ticks"].cpu().numpy())


def ored(ran_ref, fill=FILL_I):
    """what a ran_out pre-filled with `fill` holds behind the follow calls: 1 where a tick of the gait ran out, else never written"""
    return np.where(ran_ref != 0, 1, fill).astype(np.int32)


def assert_equals_walk(h, ref, ticks, gaits=None, what=""):
    """gait by gait: state, rows [0, ticks) of outs and ran_out are the reference's; rows >= ticks hold the canary"""
    st, outs, ran = ref
    for b in range(h["st"].shape[0]) if gaits is None else gaits:
        n = int(ticks[b]) if np.ndim(ticks) else int(ticks)
        assert h["st"][b].tobytes() == st[b].tobytes(), (what, b, "state")
        assert h["outs"][:n, b].tobytes() == outs[:n, b].tobytes(), (what, b, "outs")
        assert (h["outs"][n:, b] == CANARY).all(), (what, b, "rows past ticks")
        assert h["ran"][b] == ored(ran)[b], (what, b, "ran_out")


def lens_dev(fleet):
    return fleet["f"].full["length"]


# ---- 3. final queues ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B", [1, BF])
@pytest.mark.parametrize("solver", [0, 1, 2], ids=["PLDP", "QLD", "QLDANDLQ"])
def test_final_queues_in_one_call_equal_the_walk(fleet, solver, B):
    _setup_dimitrov(solver)
    try:
        ref = final_ref(fleet, solver, B)
        A = arrays(B, N_TICKS)
        follow(fleet["Q"], A, fleet["time"], lens_dev(fleet), N_TICKS, flags=FINAL)
        h = host(A)
        assert (h["ticks"] == N_TICKS).all() and (h["clock"] == wg.dimitrov_walk_time(0.0, N_TICKS)).all()
        assert_equals_walk(h, ref, N_TICKS)
        if B == BF:
            rets = {wg.DimitrovOut.from_buffer_copy(h["outs"][k, b].tobytes()).ret for k in (0, N_TICKS - 1) for b in range(B)}
            assert (0 in rets) if solver != 1 else (2 in rets)        # mode QLD is the reference's: ifail = 2 on the first tick
    finally:
        wg.dimitrov_configure(wg.dimitrov_defaults())


@gpu
def test_final_queues_with_a_horizon_of_five(fleet):
    """N = 5: a horizon hard-coded into the rule or the select would show (whole queues, not final: the rule decides)"""
    model = wg.dimitrov_defaults()
    model.N = 5
    wg.dimitrov_configure(model)
    try:
        ref = ref_walk(fleet["Q"], N_TICKS)
        A = arrays(BF, N_TICKS)
        follow(fleet["Q"], A, fleet["time"], lens_dev(fleet), N_TICKS, flags=FINAL)
        assert_equals_walk(host(A), ref, N_TICKS, what="N = 5, final")
        # and the rule itself at N = 5: whole queues that are not declared final stop where 5 instants fit, not 16
        t_of = times(fleet["f"].lcap, fleet["f"].m.T)
        want = np.array([wg.dimitrov_walk_safe_ticks(0.0, float(t_of[L - 1])) for L in fleet["f"].lens], np.int32)
        cap = int(want.max()) + 2
        A = arrays(BF, cap)
        follow(fleet["Q"], A, fleet["time"], lens_dev(fleet), cap + 1)
        assert np.array_equal(host(A)["ticks"], want)
        assert all(want[b] > safe_ticks(0.0, float(t_of[L - 1])) for b, L in enumerate(fleet["f"].lens))     # more than 16 instants allow
    finally:
        wg.dimitrov_configure(wg.dimitrov_defaults())


# ---- 4. cuts -----------------------------------------------------------------------------------------------------------------
@gpu
def test_any_cut_into_max_ticks_is_the_same_walk(fleet):
    _setup_dimitrov(0)
    ref = final_ref(fleet, 0)
    A = arrays(BF, N_TICKS)
    total = 0
    for n in (7, 0, 17, 1, 60):
        follow(fleet["Q"], A, fleet["time"], lens_dev(fleet), n, flags=FINAL)
        total = min(total + n, N_TICKS)
        h = host(A)
        assert (h["ticks"] == total).all() and (h["clock"] == wg.dimitrov_walk_time(0.0, total)).all(), n
        assert (h["outs"][total:] == CANARY).all(), n
    assert total == N_TICKS
    assert_equals_walk(h, ref, N_TICKS, what="cuts")


# ---- 5. own clocks -----------------------------------------------------------------------------------------------------------
@gpu
def test_every_gait_walks_by_its_own_clock(fleet):
    _setup_dimitrov(0)
    clock0 = np.array([0.1 * (b % 3) for b in range(BF)])
    A = arrays(BF, N_TICKS, clock0=clock0)
    follow(fleet["Q"], A, fleet["time"], lens_dev(fleet), N_TICKS, flags=FINAL)
    h = host(A)
    assert (h["ticks"] == N_TICKS).all()
    for r in range(3):
        t0 = 0.1 * r
        ref = ref_walk(fleet["Q"], N_TICKS, t0=t0)
        gaits = range(r, BF, 3)
        assert_equals_walk(h, ref, N_TICKS, gaits=gaits, what="t0 = %g" % t0)
        assert all(h["clock"][b] == wg.dimitrov_walk_time(t0, N_TICKS) for b in gaits)
    assert h["st"][1].tobytes() != ref_walk(fleet["Q"], N_TICKS)[0][1].tobytes()      # the clocks matter


# ---- 6. the rule without finality --------------------------------------------------------------------------------------------
@gpu
def test_whole_queues_that_are_not_final_stop_at_their_safe_ticks(fleet):
    import torch
    _setup_dimitrov(0)
    f, Q = fleet["f"], fleet["Q"]
    t_of = times(f.lcap, f.m.T)
    want = np.array([wg.dimitrov_walk_safe_ticks(0.0, float(t_of[L - 1])) for L in f.lens], np.int32)
    assert len(set(want)) >= 4                                            # ragged across the fleet
    cap = int(want.max()) + 2
    A = arrays(BF, cap, ran_fill=0)
    follow(Q, A, fleet["time"], lens_dev(fleet), cap + 3)                 # flags = 0, walk = NULL: more rounds than any gait has use for
    h = host(A)
    assert np.array_equal(h["ticks"], want)
    assert not h["ran"].any()
    assert all(h["clock"][b] == wg.dimitrov_walk_time(0.0, int(want[b])) for b in range(BF))
    # the reference: a loop of one-tick walks, the states snapshot after every tick
    st = to_dev(fresh_states(BF))
    outs = torch.full((cap, BF * OSZ), CANARY, dtype=torch.uint8, device="cuda")
    snaps = [st.clone()]
    t = 0.0
    for k in range(int(want.max())):
        wg.dimitrov_walk_dev(BF, QCAP, Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(), Q["count"].data_ptr(), t, 1,
                             st.data_ptr(), outs[k].data_ptr(), None, 0, _stream())
        snaps.append(st.clone())
        t = wg.dimitrov_walk_time(t, 1)
    torch.cuda.synchronize()
    snaps = [s.cpu().numpy().reshape(BF, SSZ) for s in snaps]
    outs = outs.cpu().numpy().reshape(cap, BF, OSZ)
    for b in range(BF):
        n = int(want[b])
        assert h["st"][b].tobytes() == snaps[n][b].tobytes(), b
        assert h["outs"][:n, b].tobytes() == outs[:n, b].tobytes() and (h["outs"][n:, b] == CANARY).all(), b


# ---- 7. on line --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("solver", [0, 2], ids=["PLDP", "QLDANDLQ"])
def test_online_fleet_follows_each_gaits_own_queue(fleet, solver, K):
    import torch
    _setup_dimitrov(solver)
    try:
        f, Qfull = fleet["f"], fleet["Q"]
        ref = final_ref(fleet, solver)
        calls = feeding(fleet["fl"], K)
        want_ticks = replay(fleet["fl"], K)
        w = Walk(f, ("left", "left_type", "right", "right_type"))
        Q = new_queues(BF)
        A = arrays(BF, N_TICKS)
        done = np.zeros(BF, np.int32)
        for i, (what, arg, lens_want, _) in enumerate(calls):
            lens = w.begin(arg) if what == "begin" else (w.append(arg) if what == "append" else w.end(arg))
            assert np.array_equal(lens, lens_want), (i, what)
            poison_past_length(w, lens)
            wg.foot_constraints_append_dev(BF, w.lcap, int(done.min()), Q["done"].data_ptr(), w.buf["length"].data_ptr(),
                                           fleet["time"].data_ptr(), w.buf["left"].data_ptr(), w.buf["left_type"].data_ptr(),
                                           w.buf["right"].data_ptr(), *SOLE, QCAP, Q["queues"].data_ptr(), Q["ts"].data_ptr(),
                                           Q["te"].data_ptr(), Q["count"].data_ptr(), _stream())
            done = lens.copy()
            follow(Q, A, fleet["time"], Q["done"], N_TICKS, walk=w.state)
            h = host(A)
            assert np.array_equal(h["ticks"], want_ticks[i][0]), (i, what)
            for b in range(BF):                                           # rows [0, ticks[b]) already the final rows; nothing else written
                n = int(h["ticks"][b])
                assert h["outs"][:n, b].tobytes() == ref[1][:n, b].tobytes(), (i, b)
                assert (h["outs"][n:, b] == CANARY).all(), (i, b)
        assert w.ended.all() and np.array_equal(Q["done"].cpu().numpy(), f.lens)
        assert (h["ticks"] == N_TICKS).all()
        assert_equals_walk(h, ref, N_TICKS, what="on line")
        assert all(h["clock"][b] == wg.dimitrov_walk_time(0.0, N_TICKS) for b in range(BF))
        for k in ("queues", "ts", "te", "count"):                         # the queues are the batch call's, pre-fill included
            assert torch.equal(Q[k], Qfull[k]), k
    finally:
        wg.dimitrov_configure(wg.dimitrov_defaults())


# ---- 8. sit-outs and refusals ------------------------------------------------------------------------------------------------
@gpu
def test_sit_outs_refusals_and_the_arguments_of_the_call(fleet):
    import torch
    _setup_dimitrov(0)
    f = fleet["f"]
    refs = {N_TICKS: final_ref(fleet, 0), 10: ref_walk(fleet["Q"], 10)}
    Q = dict(fleet["Q"])
    Q["count"] = fleet["Q"]["count"].clone()
    have = lens_dev(fleet).clone()
    A = arrays(BF, N_TICKS)
    SIT, REFUSED = range(0, 4), range(4, 7)
    A["ticks"][0] = N_TICKS                                               # has all its ticks
    A["ticks"][1] = -7                                                    # an earlier error
    Q["count"][2] = BAD                                                   # a gait wg_zmpdisc_* refused
    have[3] = 0                                                           # no samples yet
    A["ticks"][4] = N_TICKS + 1
    have[5] = f.lcap + 1
    A["clock"][6] = float("nan")
    before = host(A)
    for n in (10, N_TICKS):                                               # the second call finds the refusals again: sticky
        follow(Q, A, fleet["time"], have, n, flags=FINAL)
        h = host(A)
        for b in list(SIT) + list(REFUSED):
            for k in ("st", "ran", "clock"):
                assert h[k][b].tobytes() == before[k][b].tobytes(), (n, b, k)
            assert h["outs"][:, b].tobytes() == before["outs"][:, b].tobytes(), (n, b)
            assert h["ticks"][b] == (before["ticks"][b] if b in SIT else BAD), (n, b)
        others = range(7, BF)
        assert all(h["ticks"][b] == n for b in others)
        assert_equals_walk(h, refs[n], n, gaits=others, what="neighbours")   # the bytes of a run without the offenders
    # the arguments of the call itself: refused on the host, nothing launched
    A2 = arrays(BF, N_TICKS)
    was = host(A2)
    t, ln = fleet["time"], lens_dev(fleet)
    for over in (dict(B=-1), dict(qcap=0), dict(lcap=0), dict(tick_cap=-1), dict(max_ticks=-1), dict(flags=2), dict(flags=FINAL | 4),
                 dict(queues=None), dict(ts=None), dict(te=None), dict(count=None), dict(time=None), dict(have=None), dict(clock=None),
                 dict(ticks=None), dict(st=None)):
        follow(fleet["Q"], A2, t, ln, over.pop("max_ticks", N_TICKS), rc=BAD, **dict(dict(flags=FINAL), **over))
    with wg.Context(0) as ctx:                                            # a context nobody configured
        p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
        q = fleet["Q"]
        assert wg.lib().wg_dimitrov_follow_dev_ctx(ctx.handle, BF, QCAP, p(q["queues"]), p(q["ts"]), p(q["te"]), p(q["count"]), f.lcap, p(t),
                                                   p(ln), None, FINAL, p(A2["clock"]), p(A2["ticks"]), N_TICKS, N_TICKS, p(A2["st"]),
                                                   p(A2["outs"]), p(A2["ran"]), 0, _stream()) == BAD
    follow(fleet["Q"], A2, t, ln, N_TICKS, flags=FINAL, B=0)              # WG_OK, and nothing to do
    follow(fleet["Q"], A2, t, ln, 0, flags=FINAL)
    now = host(A2)
    for k in was:
        assert now[k].tobytes() == was[k].tobytes(), k
    assert torch.equal(Q["queues"], fleet["Q"]["queues"])


# ---- 9. the fleet program ----------------------------------------------------------------------------------------------------
@gpu
def test_dimitrov_fleet_follow_prints_the_whole_sequence_checksum(tmp_path):
    """host/dimitrov_fleet.cpp --online K --follow: the checksum of the run without --online, on a fleet file and --ragged"""
    zm, steps, n_steps, init = fleet70(0.7, 0.13, aligned=range(BF))
    path = tmp_path / "fleet.bin"
    with open(path, "wb") as fh:
        fh.write(np.array([BF, SMAX], np.int32).tobytes() + bytes(zm) + bytes(steps) + np.ascontiguousarray(n_steps, np.int32).tobytes()
                 + np.ascontiguousarray(init, np.float64).tobytes())
    exe = os.path.join(ROOT, "jrl-walkgen_amd", "bin", "dimitrov_fleet")

    def checksum(args):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "%d walks" % BF in r.stdout, r.stdout + r.stderr
        return re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1)

    base = ["--fleet", str(path), "--ticks", str(N_TICKS)]
    sums = [checksum(base + extra) for extra in ([], ["--online", "1", "--follow"], ["--online", "3", "--follow"])]
    assert sums[0] == sums[1] == sums[2], sums
    ragged = ["--batch", str(BF), "--steps", "8", "--ticks", str(N_TICKS), "--ragged"]
    sums = [checksum(ragged), checksum(ragged + ["--online", "2", "--follow"])]
    assert sums[0] == sums[1], sums
    r = subprocess.run([exe, "--follow"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "FAILED" in r.stderr
