"""Dimitrov-2008 fleets on the device: wg_foot_constraints_batch_dev (polytope queues of B feet trajectories),
wg_dimitrov_select_polys_dev (the queue walk of one tick) and wg_dimitrov_walk_dev (n ticks on a stream), through the C ABI.
Every comparison is byte equality: against oracle/zmpdisc_oracle.c's wgo_foot_constraints, against the host wg_foot_constraints,
against the queue walk the existing Dimitrov test does in Python (_polytopes_for_tick), against oracle/pldp_oracle.c's tick,
and HIP against HIP against today's host-fed loop.

The byte-exact partner of the kernels is the oracle built on include/wg_trig.h (libwg_oracle_ptrig.so), the one
test_zmpdisc_gpu.test_foot_constraints_match_oracle uses: oraclelib.foot_constraints goes through the libm build, whose sin / cos
differ from wg_trig.h in the last bit for a few rotated soles per fleet (the precondition test below counts them), so the same
wgo_foot_constraints is called on the wg_trig.h build here.

The fleet of test 1 is random_fleet(seed 1, smax = 9): ragged, rotated steps, non-zero start yaw.  No seed alone gives what the
test must also cover -- a vertical edge (|dx| <= 1e-7) needs an exactly axis-aligned sole and a SimilarConstraints entry of -3 a
hexagon with exactly opposite rows; 195 seeds were scanned on the CPU oracle, one had vertical edges, none a -3 -- so the six
gaits of the partial second wave (lanes 64-69) start with zero yaw and take unrotated steps.  The preconditions are asserted on
the oracle's output in the `not gpu` test."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oraclelib as ol  # noqa: E402
from test_zmpdisc_oracle import kajita_model  # noqa: E402
from test_zmpdisc_gpu import gait_steps, ptrig, random_fleet  # noqa: E402
from test_dimitrov_gpu import _polytopes_for_tick  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
gpu = pytest.mark.gpu

SOLE = (0.24, 0.138, 0.02, 0.02)             # sole 0.24 x 0.138, margins 0.02 / 0.02
QCAP, SMAX, SEED, BF = 64, 9, 1, 70
PSZ = C.sizeof(wg.ZmpPolytope)
SSZ = C.sizeof(wg.DimitrovState)
OSZ = C.sizeof(wg.DimitrovOut)
FILL_B, FILL_D, FILL_I = 0xA5, -7.25, -77    # what the outputs hold before a launch


# ---- fleets and CPU references ---------------------------------------------------------------------------------------------
def _align(zm, steps, init, gaits):
    """axis-aligned soles, the model's support times (as the existing Dimitrov pipeline test does)"""
    for b in gaits:
        init[b] = [0.0, 0.095, 0.0, 0.0, -0.095, 0.0]
        for i in range(SMAX):
            s = steps[b * SMAX + i]
            s.theta = 0.0; s.ss_time, s.ds_time = zm.t_single, 0.0; s.step_type = 1


def fleet70(t_single=0.78, t_double=0.02, aligned=range(64, BF)):
    zm = kajita_model()
    zm.t_single, zm.t_double = t_single, t_double
    steps, n_steps, init = random_fleet(np.random.default_rng(SEED), BF, SMAX, zm)
    _align(zm, steps, init, aligned)
    return zm, steps, n_steps, init


def oracle_fc(time, left, left_type, right, cap=QCAP):
    """wgo_foot_constraints of the wg_trig.h build: (polys, t_start, t_end, count), outputs pre-filled like the device's"""
    lib = ptrig()
    lib.wgo_foot_constraints.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_int] + [C.c_void_p] * 3
    polys = (wg.ZmpPolytope * cap)(); C.memset(polys, FILL_B, C.sizeof(polys))
    ts = np.full(cap, FILL_D); te = np.full(cap, FILL_D)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    time, left, right = (np.ascontiguousarray(a, dtype=np.float64) for a in (time, left, right))
    lt = np.ascontiguousarray(left_type, dtype=np.int32)
    k = lib.wgo_foot_constraints(len(time), vp(time), vp(left), vp(lt), vp(right), *SOLE, cap, C.addressof(polys), vp(ts), vp(te))
    return polys, ts, te, k


def times(n, T):
    return np.cumsum(np.full(n, T)) - T


_oracle_cache = {}


def oracle_queues(key, fleet):
    """the CPU chain wgo_zmpdisc -> wgo_foot_constraints for every gait of a fleet, computed once"""
    if key not in _oracle_cache:
        zm, steps, n_steps, init = fleet
        res = []
        for b in range(len(n_steps)):
            o = ol.zmpdisc(zm, gait_steps(steps, b, SMAX, int(n_steps[b])), init[b], lib=ptrig())
            res.append((o, oracle_fc(times(o["length"], zm.T), o["left"], o["left_type"], o["right"])))
        _oracle_cache[key] = res
    return _oracle_cache[key]


def test_fleet_preconditions_on_the_oracle():
    """conditions on the inputs of the GPU tests, from the oracle alone (no GPU)"""
    res = oracle_queues("t1", fleet70())
    counts = [q[3] for _, q in res]
    assert min(counts) >= 3 and max(counts) <= QCAP
    nrows, sims, sloped, vertical, libm_differs = set(), set(), 0, 0, 0
    for o, (P, ts, te, k) in res:
        for q in range(k):
            nrows.add(P[q].nrows)
            for j in range(P[q].nrows):
                sims.add(P[q].similar[j])
                if P[q].A[j][1] == 0.0:
                    vertical += 1                     # the |dx| <= 1e-7 branch: c = 0
                else:
                    sloped += 1
        P2, _, _, k2 = ol.foot_constraints(wg.ZmpPolytope, times(o["length"], 0.005), o["left"], o["left_type"], o["right"], *SOLE,
                                           cap=QCAP)
        libm_differs += k2 != k or bytes(P2)[:k * PSZ] != bytes(P)[:k * PSZ]
    print("fleet of test 1: counts %d..%d, rows %s, sloped %d, vertical %d, similar %s; libm oracle differs on %d gaits"
          % (min(counts), max(counts), sorted(nrows), sloped, vertical, sorted(sims), libm_differs))
    assert {4, 6} <= nrows and sloped > 0 and vertical > 0 and {-2, -3} <= sims
    zm, steps, n_steps, init = fleet70()
    assert sorted(set(int(n) for n in n_steps)) == list(range(2, SMAX + 1))          # ragged
    assert all(init[b][2] != 0.0 for b in range(64)) and any(steps[b * SMAX + 1].theta != 0.0 for b in range(64))
    # tests 4 and 6: at 0.7 / 0.13 every queue outlasts 25 ticks plus the preview window, and starts at 0
    for key, fl in (("t4", fleet70(0.7, 0.13)), ("t6", fleet70(0.7, 0.13, aligned=range(BF)))):
        for _, (P, ts, te, k) in oracle_queues(key, fl):
            assert ts[0] == 0.0 and te[k - 1] > (25 + 16) * 0.1


# ---- device plumbing --------------------------------------------------------------------------------------------------------
def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def device_feet(fleet, B=None):
    """step sequences -> wg_zmpdisc_full_batch_dev: the feet of the first B gaits, time-major, and the shared time array"""
    import torch
    zm, steps, n_steps, init = fleet
    B = B or len(n_steps)
    lens = [wg.zmpdisc_length(zm, gait_steps(steps, b, SMAX, int(n_steps[b]))) for b in range(B)]
    lcap = max(lens)
    d_steps = torch.from_numpy(np.frombuffer(steps, dtype=np.uint8)[:B * SMAX * C.sizeof(wg.RelStep)].copy()).cuda()
    d_ns = torch.from_numpy(np.ascontiguousarray(n_steps[:B])).cuda(); d_init = torch.from_numpy(np.ascontiguousarray(init[:B])).cuda()
    z = lambda *shape, dt=torch.float64: torch.zeros(*shape, dtype=dt, device="cuda")  # noqa: E731
    F = dict(B=B, lcap=lcap, lens=lens, zm=zm, lf=z(lcap, 6, B), rf=z(lcap, 6, B), lty=z(lcap, B, dt=torch.int32), ln=z(B, dt=torch.int32),
             time=torch.from_numpy(times(lcap, zm.T)).cuda())
    rc = wg.lib().wg_zmpdisc_full_batch_dev(C.byref(zm), B, SMAX, d_steps.data_ptr(), d_ns.data_ptr(), d_init.data_ptr(), lcap, None, None,
                                            None, None, F["lf"].data_ptr(), F["lty"].data_ptr(), F["rf"].data_ptr(), None,
                                            F["ln"].data_ptr(), _stream())
    assert rc == 0
    return F


def device_queues(F, qcap=QCAP):
    """wg_foot_constraints_batch_dev on pre-filled outputs: dict of device tensors"""
    import torch
    B = F["B"]
    Q = dict(B=B, qcap=qcap, queues=torch.full((B, qcap * PSZ), FILL_B, dtype=torch.uint8, device="cuda"),
             ts=torch.full((B, qcap), FILL_D, dtype=torch.float64, device="cuda"),
             te=torch.full((B, qcap), FILL_D, dtype=torch.float64, device="cuda"),
             count=torch.full((B,), FILL_I, dtype=torch.int32, device="cuda"))
    wg.foot_constraints_batch_dev(B, F["lcap"], F["ln"].data_ptr(), F["time"].data_ptr(), F["lf"].data_ptr(), F["lty"].data_ptr(),
                                  F["rf"].data_ptr(), *SOLE, qcap, Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(),
                                  Q["count"].data_ptr(), _stream())
    torch.cuda.synchronize()
    return Q


def queues_to_host(Q):
    return Q["queues"].cpu().numpy(), Q["ts"].cpu().numpy(), Q["te"].cpu().numpy(), Q["count"].cpu().numpy()


def assert_queue(dev, b, ref, qcap=QCAP, what=""):
    """gait b of the device output == (polys, ts, te, k) of a CPU call with the same capacity and fill, entry for entry"""
    qb, ts, te, cnt = dev
    P, rts, rte, k = ref
    assert cnt[b] == k, (what, b, cnt[b], k)
    assert qb[b].tobytes() == bytes(P), (what, b, "polytopes")          # the first min(k, qcap) entries AND the untouched tail
    assert ts[b].tobytes() == rts.tobytes() and te[b].tobytes() == rte.tobytes(), (what, b, "intervals")


@pytest.fixture(scope="module")
def fleet1():
    """test 1's fleet on the device: feet, queues, and both copied back"""
    wg.init(0)
    fl = fleet70()
    F = device_feet(fl)
    Q = device_queues(F)
    return dict(fleet=fl, F=F, Q=Q, host=queues_to_host(Q), lf=F["lf"].cpu().numpy(), rf=F["rf"].cpu().numpy(),
                lty=F["lty"].cpu().numpy())


# ---- 1. queues against the oracle -------------------------------------------------------------------------------------------
@gpu
def test_queues_match_oracle_and_host_call(fleet1):
    zm = fleet1["fleet"][0]
    F, dev = fleet1["F"], fleet1["host"]
    ora = oracle_queues("t1", fleet1["fleet"])
    assert list(F["ln"].cpu().numpy()) == F["lens"]
    for b in range(BF):
        L = F["lens"][b]
        left, right, lt = fleet1["lf"][:L, :, b], fleet1["rf"][:L, :, b], fleet1["lty"][:L, b]
        ref = oracle_fc(times(L, zm.T), left, lt, right)                 # the oracle on this gait's feet copied back
        assert_queue(dev, b, ref, what="oracle")
        o, (P, ts, te, k) = ora[b]                                        # ... which is the oracle chain's own result
        assert k == ref[3] and bytes(P) == bytes(ref[0])
        hp, hts, hte, hk = wg.foot_constraints(times(L, zm.T), left, lt, right, *SOLE, cap=QCAP)     # the host call
        assert hk == k and bytes(hp)[:k * PSZ] == dev[0][b].tobytes()[:k * PSZ], (b, "host polytopes")
        assert hts.tobytes() == dev[1][b, :k].tobytes() and hte.tobytes() == dev[2][b, :k].tobytes(), (b, "host intervals")


@gpu
@pytest.mark.parametrize("B", [1, 64])
def test_queues_do_not_depend_on_the_batch(fleet1, B):
    part = queues_to_host(device_queues(device_feet(fleet1["fleet"], B)))
    for a, full in zip(part, fleet1["host"]):
        assert a.tobytes() == full[:B].tobytes()


# ---- 2. chunk edges ---------------------------------------------------------------------------------------------------------
@gpu
def test_chunk_edges():
    import torch
    wg.init(0)
    CH = wg.foot_constraints_chunk()
    assert CH >= 32
    lens = [1, CH - 1, 2 * CH + 1]
    B, lcap = 3, 2 * CH + 1
    DS, LA, RA, INH = 0, 1, 2, 3                       # double support, left / right foot in the air, "none of the three tests"
    st = [[DS] * lcap for _ in range(B)]
    st[0][0] = LA                                      # length 1: one polytope, a change at sample 0
    st[1][:CH - 2] = [LA] * (CH - 2)                   # one chunk minus 1: changes at sample 0 and at the gait's last sample
    g = st[2]
    g[:CH - 1] = [RA] * (CH - 1)                       # change at sample 0; back to double support at the LAST sample of chunk 0
    g[CH:CH + 5] = [LA] * 5                            # change at the FIRST sample of chunk 1
    g[CH + 5] = DS                                     # two consecutive samples, each a change
    g[CH + 6:2 * CH - 2] = [RA] * (CH - 8)
    g[2 * CH - 2] = g[2 * CH - 1] = g[2 * CH] = INH    # left z == 0.00001, right z == 0 as the first sample of chunk 2 (behind two
    lf = np.zeros((lcap, 6, B)); rf = np.zeros((lcap, 6, B)); lty = np.zeros((lcap, B), np.int32)          # more: the walk back)
    for b in range(B):
        for i in range(lcap):
            lf[i, :2, b] = [0.001 * i, 0.095 + 0.01 * b]; rf[i, :2, b] = [0.0005 * i, -0.095]
            lf[i, 3, b] = rf[i, 3, b] = 3.0 * (b == 2)
            lf[i, 2, b] = {DS: 0.0, LA: 0.03, RA: 0.0, INH: 0.00001}[st[b][i]]
            rf[i, 2, b] = {DS: 0.0, LA: 0.0, RA: 0.02, INH: 0.0}[st[b][i]]
    lty[CH + 20:CH + 23, 2] = 10                       # stepType >= 10: double support whatever the heights say
    time = np.arange(lcap) * 0.005
    F = dict(B=B, lcap=lcap, lf=torch.from_numpy(lf).cuda(), rf=torch.from_numpy(rf).cuda(), lty=torch.from_numpy(lty).cuda(),
             ln=torch.from_numpy(np.array(lens, np.int32)).cuda(), time=torch.from_numpy(time).cuda())
    dev = queues_to_host(device_queues(F))
    want = [1, 2, 7]
    for b in range(B):
        L = lens[b]
        ref = oracle_fc(time[:L], lf[:L, :, b], lty[:L, b], rf[:L, :, b])
        assert ref[3] == want[b], (b, ref[3])          # the scenario is what the comments say
        assert_queue(dev, b, ref, what="chunk edges")


# ---- 3. capacity and errors --------------------------------------------------------------------------------------------------
@gpu
def test_capacity_and_bad_arguments(fleet1):
    zm = fleet1["fleet"][0]
    F = fleet1["F"]
    cap = 5
    dev = queues_to_host(device_queues(F, qcap=cap))
    full = fleet1["host"][3]
    assert (full > cap).any() and (dev[3] == full).all()                  # the full number, whatever the capacity
    for b in range(BF):
        L = F["lens"][b]
        ref = oracle_fc(times(L, zm.T), fleet1["lf"][:L, :, b], fleet1["lty"][:L, b], fleet1["rf"][:L, :, b], cap=cap)
        assert_queue(dev, b, ref, qcap=cap, what="capacity")              # exactly min(count, cap) entries, neighbours intact
    lib = wg.lib()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    Q = fleet1["Q"]
    args = (p(F["ln"]), p(F["time"]), p(F["lf"]), p(F["lty"]), p(F["rf"]), *SOLE)
    outs = (p(Q["queues"]), p(Q["ts"]), p(Q["te"]), p(Q["count"]))
    assert lib.wg_foot_constraints_batch_dev(0, F["lcap"], *args, QCAP, *outs, None) == 0
    assert lib.wg_foot_constraints_batch_dev(BF, F["lcap"], *args, QCAP, None, outs[1], outs[2], outs[3], None) == -2
    assert lib.wg_foot_constraints_batch_dev(BF, 0, *args, QCAP, *outs, None) == -2
    assert queues_to_host(Q)[0].tobytes() == fleet1["host"][0].tobytes()  # the refused calls wrote nothing


# ---- 4. selection against the reference's walk ---------------------------------------------------------------------------------
def ref_select(P, ts, te, k, t0, N, T):
    """what wg_mpc.h documents: _polytopes_for_tick while it stays inside the queue; the LAST polytope once it does not"""
    k = min(k, QCAP)
    if k <= 0:
        return None, 1
    try:
        sel = _polytopes_for_tick(P, ts, te, k, t0, N, T)
    except AssertionError:                             # t0 in no interval
        return [k - 1] * N, 1
    ran = int(max(sel) >= k)
    first = next((i for i, q in enumerate(sel) if q >= k), N)
    return sel[:first] + [k - 1] * (N - first), ran


def run_select(Q, t0, N, count=None):
    import torch
    B = Q["B"]
    polys = torch.full((B, N * PSZ), FILL_B, dtype=torch.uint8, device="cuda")
    ran = torch.full((B,), FILL_I, dtype=torch.int32, device="cuda")
    wg.dimitrov_select_polys_dev(B, Q["qcap"], Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(),
                                 (Q["count"] if count is None else count).data_ptr(), t0, polys.data_ptr(), ran.data_ptr(), _stream())
    return polys.cpu().numpy(), ran.cpu().numpy()


def _setup_dimitrov(solver=0):
    wg.init(0)
    model = wg.dimitrov_defaults()
    model.solver = solver
    wg.dimitrov_configure(model)
    return model


@gpu
def test_selection_matches_the_reference_walk():
    model = _setup_dimitrov()
    N, T = model.N, model.T
    Q = device_queues(device_feet(fleet70(0.7, 0.13)))
    qb, ts, te, cnt = queues_to_host(Q)
    assert (cnt >= 3).all() and (cnt <= QCAP).all()

    def check(t0, count=None, cnt=cnt):
        got, ran = run_select(Q, t0, N, count)
        n_in = 0
        for b in range(BF):
            sel, want_ran = ref_select(None, ts[b], te[b], int(cnt[b]), t0, N, T)
            want = bytes(N * PSZ) if sel is None else b"".join(qb[b, q * PSZ:(q + 1) * PSZ].tobytes() for q in sel)
            assert got[b].tobytes() == want, (t0, b, sel)
            assert ran[b] == want_ran, (t0, b)
            n_in += not want_ran
        return n_in, ran

    t0, inside = 0.0, 0
    for _ in range(40):                                # 40 values of t0 accumulated by += T
        inside += check(t0)[0]
        t0 += T
    assert inside > 0.9 * 40 * BF                      # nearly every walk stays inside its queue: _polytopes_for_tick's own answer
    # run-out cases: beyond the last interval; past the last entry at instant 5; a gait without polytopes
    _, ran = check(1e3)
    assert (ran == 1).all()
    b = 7
    t_edge = te[b, cnt[b] - 1] - 4.5 * T
    sel, want_ran = ref_select(None, ts[b], te[b], int(cnt[b]), t_edge, N, T)
    assert want_ran == 1 and ts[b, cnt[b] - 1] <= t_edge and t_edge + 4 * T <= te[b, cnt[b] - 1] < t_edge + 5 * T
    _, ran = check(t_edge)
    assert ran[b] == 1
    c0 = Q["count"].clone(); c0[3] = 0
    h0 = cnt.copy(); h0[3] = 0
    got, ran = check(0.0, count=c0, cnt=h0)
    assert ran[3] == 1 and ran.sum() == 1


# ---- 5. / 6. / 7. the walk ---------------------------------------------------------------------------------------------------
def fresh_states(B):
    st = (wg.DimitrovState * B)()
    for b in range(B):
        st[b].starting = 1
    return st


def to_dev(ct):
    import torch
    return torch.from_numpy(np.frombuffer(ct, dtype=np.uint8).copy()).cuda()


def device_walk(Q, n_ticks, B=None, sync=True):
    """ONE wg_dimitrov_walk_dev from fresh states at t0 = 0: (states, outs, ran_out) as device tensors"""
    import torch
    B = B or Q["B"]
    st = to_dev(fresh_states(B))
    outs = torch.zeros((n_ticks, B * OSZ), dtype=torch.uint8, device="cuda")      # zeroed, as the host-pointer tick hands them over
    ran = torch.full((B,), FILL_I, dtype=torch.int32, device="cuda")
    wg.dimitrov_walk_dev(B, Q["qcap"], Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(), Q["count"].data_ptr(), 0.0,
                         n_ticks, st.data_ptr(), outs.data_ptr(), ran.data_ptr(), 0, _stream())
    if sync:
        torch.cuda.synchronize()
    return st, outs, ran


def host_queues(F):
    """today's path: every gait's feet copied back, wg_foot_constraints on the host"""
    lf, rf, lty = F["lf"].cpu().numpy(), F["rf"].cpu().numpy(), F["lty"].cpu().numpy()
    res = []
    for b in range(F["B"]):
        L = F["lens"][b]
        res.append(wg.foot_constraints(times(L, F["zm"].T), lf[:L, :, b], lty[:L, b], rf[:L, :, b], *SOLE, cap=QCAP))
    return res


def host_select(queues, t0, N, T):
    B = len(queues)
    polys = (wg.ZmpPolytope * (B * N))()
    for b, (pq, ts, te, k) in enumerate(queues):
        for i, q in enumerate(_polytopes_for_tick(pq, ts, te, k, t0, N, T)):
            C.memmove(C.byref(polys[b * N + i]), C.byref(pq[q]), PSZ)
    return polys


@gpu
def test_walk_matches_the_oracle_tick():
    """test_step_sequences_to_com_through_zmpdisc_footconstraints_and_the_tick's scenario, everything from the step sequences on
    produced on the device and run as ONE wg_dimitrov_walk_dev; the oracle tick is fed by host-selected polytopes of host-built
    queues.  A gait is compared up to and including its first non-zero return code (the existing test re-seeds the GPU state from
    the oracle there, which a single launch cannot do): every out as bytes while the code is 0, code and solver counts at the tick
    that fails; the final state of a gait that never fails is the oracle's."""
    model = _setup_dimitrov()
    K = wg.dimitrov_constants(model.N)
    N, T = model.N, model.T
    M = ol.pldp_setup(N, K["iPu"], K["Px"], K["Pu"])
    lib = ol.oracle()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    zm = kajita_model()
    zm.t_single, zm.t_double = 0.7, 0.13
    B = 6
    steps, n_steps, init = random_fleet(np.random.default_rng(31), B, SMAX, zm, exotic=False)
    _align(zm, steps, init, range(B))
    F = device_feet((zm, steps, n_steps, init))
    Q = device_queues(F)
    hq = host_queues(F)
    n_ticks = int(min((q[2][-1] - N * T) / T for q in hq)) - 1
    assert n_ticks > 40
    st, outs, ran = device_walk(Q, n_ticks)
    st_h = st.cpu().numpy().tobytes(); outs_h = outs.cpu().numpy()
    assert not ran.cpu().numpy().any()
    so = fresh_states(B)
    lived = np.zeros(B, int); alive = np.ones(B, bool)
    t0 = 0.0
    for it in range(n_ticks):
        polys = host_select(hq, t0, N, T)
        for b in range(B):
            if not alive[b]:
                continue
            oo = wg.DimitrovOut()
            rc = lib.wgo_dimitrov_tick(C.byref(M), dp(K["OptB"]), dp(K["OptC"]), dp(K["iLQ"]), C.c_double(T), C.c_double(model.Tctrl),
                                       C.c_double(model.com_height), C.byref(polys, b * N * PSZ), C.byref(so[b]), C.byref(oo),
                                       C.c_int(0))
            got = wg.DimitrovOut.from_buffer_copy(outs_h[it, b * OSZ:(b + 1) * OSZ].tobytes())
            assert got.ret == rc, (it, b, got.ret, rc)
            same = bytes(got) == bytes(oo)
            if rc != 0:
                # PLDP's exit(0) path (-2): the oracle tick returns before its solver has written X, so its out holds whatever its
                # stack held there; the existing test compares these fields at that tick, and so does this one
                print("gait %d: first non-zero return code %d at tick %d; out bytes equal the oracle's: %s" % (b, rc, it, same))
                assert rc == -2 and (got.n_iter, got.n_active, got.m) == (oo.n_iter, oo.n_active, oo.m), (it, b)
                alive[b] = False
                continue
            assert same, (it, b)
            lived[b] = it + 1
        t0 += T
    assert lived.min() >= 30                              # the oracle alone keeps every gait alive for 30 ticks
    for b in range(B):
        if alive[b]:
            assert st_h[b * SSZ:(b + 1) * SSZ] == bytes(so[b]), b


def fnv1a(data):
    h = 1469598103934665603
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.fixture(scope="module")
def fleet6():
    """the 70-gait fleet, axis-aligned, on the device: feet and queues"""
    wg.init(0)
    fl = fleet70(0.7, 0.13, aligned=range(BF))
    F = device_feet(fl)
    return dict(fleet=fl, F=F, Q=device_queues(F))


@gpu
@pytest.mark.parametrize("solver", [0, 1, 2], ids=["PLDP", "QLD", "QLDANDLQ"])
def test_walk_equals_the_host_fed_loop(fleet6, solver):
    import torch
    model = _setup_dimitrov(solver)
    try:
        N, T, n_ticks = model.N, model.T, 25
        F, Q = fleet6["F"], fleet6["Q"]
        # (a) today's path: host queues, host selection, host-pointer tick
        hq = host_queues(F)
        sa = fresh_states(BF)
        outs_a = []
        t0 = 0.0
        for _ in range(n_ticks):
            outs_a.append(bytes(wg.dimitrov_tick_batch(host_select(hq, t0, N, T), sa)))
            t0 += T
        # (b) a loop of select + wg_dimitrov_tick_batch_dev
        sb = to_dev(fresh_states(BF))
        polys = torch.zeros(BF * N * PSZ, dtype=torch.uint8, device="cuda")
        outs_b = torch.zeros((n_ticks, BF * OSZ), dtype=torch.uint8, device="cuda")
        t0 = 0.0
        for k in range(n_ticks):
            wg.dimitrov_select_polys_dev(BF, QCAP, Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(), Q["count"].data_ptr(),
                                         t0, polys.data_ptr(), None, _stream())
            wg.dimitrov_tick_batch_dev(BF, polys.data_ptr(), sb.data_ptr(), outs_b[k].data_ptr(), 0, _stream())
            t0 += T
        # (c) one wg_dimitrov_walk_dev, and right behind it on the same stream a second, smaller one
        sc, outs_c, ran = device_walk(Q, n_ticks, sync=False)
        B2 = 20
        s2, outs_2, _ = device_walk(Q, n_ticks, B=B2, sync=False)
        torch.cuda.synchronize()
        assert not ran.cpu().numpy().any()
        rets = set()
        for k in range(n_ticks):
            assert outs_b[k].cpu().numpy().tobytes() == outs_a[k], (k, "select + tick loop")
            assert outs_c[k].cpu().numpy().tobytes() == outs_a[k], (k, "walk")
            rets |= {wg.DimitrovOut.from_buffer_copy(outs_a[k][b * OSZ:(b + 1) * OSZ]).ret for b in range(BF)}
        assert sb.cpu().numpy().tobytes() == bytes(sa) and sc.cpu().numpy().tobytes() == bytes(sa)
        assert (0 in rets) if solver != 1 else (2 in rets)            # mode QLD is the reference's: ifail = 2 on the first tick
        # the second walk alone: the same bytes (the context's polytope buffer is reused behind the first)
        s2a, outs_2a, _ = device_walk(Q, n_ticks, B=B2)
        assert s2.cpu().numpy().tobytes() == s2a.cpu().numpy().tobytes() and torch.equal(outs_2, outs_2a)
        for k in range(n_ticks):                                      # ... which are the first gaits of the fleet's walk
            assert outs_2[k].cpu().numpy().tobytes() == outs_a[k][:B2 * OSZ]
    finally:
        wg.dimitrov_configure(wg.dimitrov_defaults())


@gpu
def test_host_program_walks_the_same_fleet(fleet6, tmp_path):
    """host/dimitrov_fleet.cpp (plain C++ through the C ABI) on test 6's fleet: same checksum of the final states"""
    _setup_dimitrov()
    zm, steps, n_steps, init = fleet6["fleet"]
    path = tmp_path / "fleet.bin"
    with open(path, "wb") as f:
        f.write(np.array([BF, SMAX], np.int32).tobytes() + bytes(zm) + bytes(steps) + np.ascontiguousarray(n_steps, np.int32).tobytes()
                + np.ascontiguousarray(init, np.float64).tobytes())
    st, _, _ = device_walk(fleet6["Q"], 25)
    want = fnv1a(st.cpu().numpy().tobytes())
    exe = os.path.join(ROOT, "jrl-walkgen_amd", "bin", "dimitrov_fleet")
    r = subprocess.run([exe, "--fleet", str(path), "--ticks", "25"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d walks" % BF in r.stdout and r.stdout.strip().endswith("checksum %016x" % want), r.stdout
