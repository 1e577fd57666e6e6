"""wg_dimitrov_follow_dev, without a GPU: the entry points exist, and the follow rule replayed in Python on host arithmetic alone
(wg_zmpdisc_length_after, the shared time array, N = 16, T = 0.1) does on the 70-gait fleet what the GPU tests of
tests/test_dimitrov_follow_gpu.py rely on -- ragged tick counts, sit-outs beside advancers, gaits ahead of the lock-step walk.
`feeding` and `replay` are what those tests hold the device's tick counts to."""
import ctypes as C
import importlib
import inspect
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_zmpdisc_gpu import gait_steps  # noqa: E402
from test_dimitrov_walk_gpu import BF, SMAX, fleet70, times  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")

N_TICKS = 60
N_HORIZON, T_TICK = 16, 0.1                    # wg_dimitrov_defaults


def feeding(fleet, K):
    """the calls of an on-line walk fed K steps at a time, as tests/test_footcons_online_gpu.py feeds it: begin with two steps,
    end the gaits whose steps have run out, then { append min(K, steps left); end those out of steps } -- one entry per call that
    grows the queues: (what, counts or select [B], lengths [B] after it, ended [B] after it)"""
    zm, steps, n_steps, _ = fleet
    B = len(n_steps)
    n_steps = np.asarray(n_steps, np.int64)
    seqs = [gait_steps(steps, b, SMAX, int(n_steps[b])) for b in range(B)]
    given, ended = np.full(B, 2, np.int64), np.zeros(B, bool)
    lens = lambda: np.array([wg.zmpdisc_length_after(zm, seqs[b], int(given[b]), bool(ended[b])) for b in range(B)], np.int32)  # noqa: E731
    calls = [("begin", given.astype(np.int32), lens(), ended.copy())]

    def end_those_out_of_steps():
        out = (given == n_steps) & ~ended
        if out.any():
            ended[out] = True
            calls.append(("end", out.astype(np.int32), lens(), ended.copy()))

    end_those_out_of_steps()
    while not ended.all():
        counts = np.where(ended, 0, np.minimum(K, n_steps - given)).astype(np.int32)
        given += counts
        calls.append(("append", counts, lens(), ended.copy()))
        end_those_out_of_steps()
    return calls


def safe_ticks(t0, t_have, N=N_HORIZON, T=T_TICK):
    """wg_dimitrov_walk_safe_ticks, in Python: the same doubles"""
    n, t = 0, t0
    while t + (N - 1) * T <= t_have:
        n, t = n + 1, t + T
    return n


def replay(fleet, K, cap=N_TICKS, N=N_HORIZON, T=T_TICK):
    """per call: (ticks [B] of the follow rule after it, ticks of the lock-step walk after it)"""
    zm = fleet[0]
    calls = feeding(fleet, K)
    B = len(fleet[2])
    t_of = times(int(max(c[2].max() for c in calls)), zm.T)
    ticks, clock = np.zeros(B, np.int32), np.zeros(B)
    lock, t_lock = 0, 0.0
    res = []
    for _, _, lens, ended in calls:
        for b in range(B):
            while ticks[b] < cap and (ended[b] or clock[b] + (N - 1) * T <= t_of[lens[b] - 1]):
                ticks[b] += 1
                clock[b] += T
        n = cap - lock
        if not ended.all():
            n = min(n, safe_ticks(t_lock, float(t_of[lens[~ended].min() - 1]), N, T))
        for _ in range(n):
            t_lock += T
        lock += n
        res.append((ticks.copy(), lock))
    return res


def test_follow_entry_points_exist_and_the_abi_version_stays():
    lib = wg.lib()
    assert hasattr(lib, "wg_dimitrov_follow_dev") and hasattr(lib, "wg_dimitrov_follow_dev_ctx")
    assert callable(wg.dimitrov_follow_dev) and wg.DIMITROV_FOLLOW_ALL_FINAL == 1
    assert "ctx" in inspect.signature(wg.dimitrov_follow_dev).parameters       # the context form: ctx= a Context or a raw handle
    assert lib.wg_dimitrov_follow_dev_ctx.argtypes == [C.c_void_p] + lib.wg_dimitrov_follow_dev.argtypes
    assert len(lib.wg_dimitrov_follow_dev_ctx.argtypes) == len(lib.wg_dimitrov_follow_dev.argtypes) + 1 == 21
    assert lib.wg_abi_version() == 5


def test_follow_rule_meets_its_preconditions_on_host_arithmetic():
    fleet = fleet70(0.7, 0.13)
    for K in (1, 3):
        res = replay(fleet, K)
        prev = np.zeros(BF, np.int32)
        distinct, mixed, rounds, useful = [], [], [], []
        for ticks, _ in res:
            adv = ticks - prev
            distinct.append(len(set(adv[adv > 0])))
            mixed.append(((adv == 0).sum(), (adv > 0).sum()))
            rounds.append(int(adv.max()))
            useful.append(bool((adv > 0).any()))
            prev = ticks
        last_useful = max(i for i, u in enumerate(useful) if u)
        ahead = [int((ticks > lock).sum()) for ticks, lock in res]
        print("K = %d: %d calls; distinct advances per call %s; (sit-outs, advancers) %s; ahead of the lock-step walk %s; lock-step "
              "%s; most rounds %d" % (K, len(res), distinct, mixed, ahead, [lock for _, lock in res], max(rounds)))
        assert max(distinct) >= 4
        assert any(s > 0 and a > 0 for s, a in mixed)
        assert last_useful >= 4 and all(a >= 60 for a in ahead[2:last_useful])
        assert (res[-1][0] == N_TICKS).all() and res[-1][1] == N_TICKS
        assert max(rounds) <= N_TICKS
