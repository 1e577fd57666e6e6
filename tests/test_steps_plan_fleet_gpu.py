"""wg_steps_plan_fleet_dev: the step stack of B gaits with the support times of each gait (ss[b], ds[b] on the device).  Gait b's
rows, count and stack are the bytes of the host call wg_steps_plan(.., ss[b], ds[b], ..); a non-finite time refuses that gait
alone, and the refusal is sticky."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stepsplan as sp  # noqa: E402
from stepsplan import ADD, BAD, wg  # noqa: E402
from test_steps_plan_gpu import CANARY, DevStack  # noqa: E402

pytestmark = pytest.mark.gpu


def plan_fleet(d, lists, ccap, ss, ds):
    """one wg_steps_plan_fleet_dev over the gaits' lists on a DevStack; no synchronisation"""
    import torch
    raw, n = sp.cmd_bytes(lists, ccap)
    d_cmds, d_n = torch.from_numpy(raw).cuda(), torch.from_numpy(n).cuda()
    d_ss, d_ds = torch.from_numpy(np.asarray(ss, np.float64)).cuda(), torch.from_numpy(np.asarray(ds, np.float64)).cuda()
    d.keepalive.append((d_cmds, d_n, d_ss, d_ds))
    wg.steps_plan_fleet_dev(d.B, ccap, d_cmds.data_ptr(), d_n.data_ptr(), d_ss.data_ptr(), d_ds.data_ptr(), d.stack[1:].data_ptr(),
                            d.smax, d.steps[1:].data_ptr(), d.n[1:].data_ptr())


def test_times_per_gait_refusal_of_a_nan_time_and_its_stickiness():
    B, smax, ccap = 70, 64, 8
    fam = sp.family(6407, 70, ccap, smax)[:B]
    rng = np.random.default_rng(53)
    ss = rng.choice([0.6, 0.7, 0.78, 0.9], B) * rng.uniform(0.8, 1.2, B)
    ds = rng.choice([0.02, 0.05, 0.1], B) * rng.uniform(0.8, 1.2, B)
    ss[13], ds[66] = np.nan, np.inf                    # one in each wave group of four; 12, 14, 65, 67 are their neighbours
    keep0 = np.array([f[2] for f in fam], np.int32)
    d = DevStack(B, smax, keep0)
    plan_fleet(d, [f[0] for f in fam], ccap, ss, ds)
    rows, n, st = d.read()
    assert n.max() > 1
    for b, (cmds, _, k0, _) in enumerate(fam):
        if b in (13, 66):
            assert n[b] == 0 and (rows[b] == CANARY).all() and st[b].tolist() == [k0, BAD, 0, 0], b
            continue
        buf, hn, hs = sp.host_plan(cmds, k0, smax, ss=float(ss[b]), ds=float(ds[b]))
        assert hn == n[b] and np.array_equal(buf[1:-1], rows[b]), b
        assert [hs.keep, hs.error, hs.n_given, hs.pad_] == st[b].tolist(), b
    # a second call with good times: the refused gaits stay refused and keep their bytes, the others walk on
    ss2, ds2 = np.full(B, 0.7), np.full(B, 0.05)
    plan_fleet(d, [[(ADD, 0, 0.1, 0.2, 0.0)]] * B, ccap, ss2, ds2)
    rows2, n2, st2 = d.read()
    for b in range(B):
        if b in (13, 66):
            assert n2[b] == 0 and (rows2[b] == CANARY).all() and st2[b].tolist() == [keep0[b], BAD, 0, 0], b
            continue
        stack = wg.StepStack(*[int(v) for v in st[b]])
        buf, hn, hs = sp.host_plan([(ADD, 0, 0.1, 0.2, 0.0)], smax=smax, ss=0.7, ds=0.05, stack=stack)
        assert hn == n2[b] == 1 and np.array_equal(buf[1], rows2[b, 0]) and np.array_equal(rows2[b, 1:], rows[b, 1:]), b
        assert [hs.keep, hs.error, hs.n_given, hs.pad_] == st2[b].tolist(), b


def test_uniform_times_leave_the_bytes_of_the_one_time_call_and_bad_arguments():
    B, smax, ccap = 65, 7, 8
    fam = sp.family(707, 70, ccap, smax)[:B]
    keep0 = np.array([f[2] for f in fam], np.int32)
    lists = [f[0] for f in fam]
    one, fleet = DevStack(B, smax, keep0), DevStack(B, smax, keep0)
    one.plan(lists, ccap)
    plan_fleet(fleet, lists, ccap, np.full(B, sp.SS), np.full(B, sp.DS))
    for a, b in zip(one.read(), fleet.read()):
        assert np.array_equal(a, b)
    lib = wg.lib()
    p = fleet.keepalive[-1]
    args = lambda ss, ds: (B, ccap, p[0].data_ptr(), p[1].data_ptr(), ss, ds, fleet.stack[1:].data_ptr(), smax,  # noqa: E731
                           fleet.steps[1:].data_ptr(), fleet.n[1:].data_ptr(), None)
    assert lib.wg_steps_plan_fleet_dev(*args(None, p[3].data_ptr())) == -2
    assert lib.wg_steps_plan_fleet_dev(*args(p[2].data_ptr(), None)) == -2
    assert lib.wg_steps_plan_fleet_dev(0, *args(p[2].data_ptr(), p[3].data_ptr())[1:]) == 0
    for a, b in zip(one.read(), fleet.read()):         # nothing was launched
        assert np.array_equal(a, b)
