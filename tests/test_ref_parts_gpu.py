"""The kernels that compile csrc/wg_footcons_geom.hpp's fc_hull8 (wg_foot_constraints_batch_dev / _append_dev) and the feet
queue's polynomials (wg_zmpdisc_full_batch_dev), held to what the reference's own ConvexHull.cpp and PolynomeFoot.cpp gave when
compiled: tests/golden/ref_parts.npz, recorded by tests/golden/make_golden.py from oracle/_ref/libwalkgen_parts_ref.so.  Nothing
here opens the reference tree or oracle/_ref/, so nothing here can skip.

The expectations are built on the CPU by tests/refparts.py from the record and the wg_trig.h oracle's corner and polytope probes,
and tests/test_ref_parts_oracle.py holds them to the oracle and to the host call first.  Every comparison is byte equality.

The tick's polynomials (csrc/wg_tick_device.hpp: poly_eval, poly_d1, poly_d2, poly3/4/5_set) have no entry point of their own:
tests/test_ref_parts_oracle.py pins oracle/herdt_oracle.c's to the compiled classes, and the GPU == oracle tests of the tick
(tests/test_tick_gpu.py, test_models_gpu.py, test_fullsize_gpu.py) carry the pin to the kernel."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import refparts as rp  # noqa: E402
from test_zmpdisc_gpu import gait_steps  # noqa: E402
from test_dimitrov_walk_gpu import FILL_B, FILL_D, FILL_I, SOLE, _stream, device_queues, queues_to_host  # noqa: E402
from test_footcons_online_gpu import append, new_queues  # noqa: E402

wg = rp.wg
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fleet():
    """the recorded stances as B = 70 ragged feet trajectories on the device"""
    import torch
    wg.init(0)
    assert wg.foot_constraints_chunk() == rp.CH
    assert (FILL_B, FILL_D, FILL_I, SOLE) == (rp.FILL_B, rp.FILL_D, rp.FILL_I, rp.SOLE)
    gold = np.load(rp.GOLDEN)
    time, left, lty, right, lens = rp.fleet_trajectories(gold)
    assert left.shape == (rp.CH + 48, 6, rp.FLEET_B)
    F = dict(B=rp.FLEET_B, lcap=left.shape[0], lf=torch.from_numpy(left).cuda(), rf=torch.from_numpy(right).cuda(),
             lty=torch.from_numpy(lty).cuda(), ln=torch.from_numpy(lens).cuda(), time=torch.from_numpy(time).cuda())
    return dict(gold=gold, F=F, lens=lens)


def assert_queues(dev, want, what):
    for name, a, w in zip(("polytopes", "t_start", "t_end", "count"), dev, want):
        if a.tobytes() != w.tobytes():
            bad = [b for b in range(rp.FLEET_B) if a[b].tobytes() != w[b].tobytes()]
            raise AssertionError("%s: %s differ for gaits %s" % (what, name, bad[:10]))


def test_batch_queues_are_the_polytopes_of_the_recorded_reference_hulls(fleet):
    """wg_foot_constraints_batch_dev: queues, t_start, t_end and count, whole arrays with their untouched entries"""
    dev = queues_to_host(device_queues(fleet["F"], qcap=rp.FLEET_QCAP))
    assert_queues(dev, rp.fleet_expectation(fleet["gold"]), "batch")


def test_appended_queues_are_the_polytopes_of_the_recorded_reference_hulls(fleet):
    """the same fleet through wg_foot_constraints_append_dev, cut at a chunk edge and one sample after it; after every call
    the queues of the prefix"""
    Q = new_queues(rp.FLEET_B, rp.FLEET_QCAP)
    done = np.zeros(rp.FLEET_B, np.int32)
    for cut in (rp.CH, rp.CH + 1, int(fleet["lens"].max())):
        lens = np.minimum(fleet["lens"], cut)
        dev = append(fleet["F"], Q, lens, first_sample=int(done.min()))
        assert np.array_equal(dev[4], lens)
        assert_queues(dev[:4], rp.fleet_expectation(fleet["gold"], lens), "append to %d" % cut)
        done = lens
    assert np.array_equal(done, fleet["lens"])


@pytest.mark.parametrize("i", range(len(rp.SWING_MODELS)))
def test_swing_heights_are_the_recorded_polynomial(i):
    """wg_zmpdisc_full_batch_dev, B = 70 random step sequences, omega = 0: the z column of either foot is the recorded
    Polynome4(t_single, step_height).Compute(k T) wherever the foot is in the air and 0 elsewhere (rp.swing_expectation)"""
    import torch
    wg.init(0)
    want, airborne, _ = rp.swing_expectation(np.load(rp.GOLDEN), i)
    assert airborne > 10000
    zm, steps, n_steps, init = rp.swing_fleet(i)
    B, smax = rp.FLEET_B, rp.SWING_SMAX
    lens = [wg.zmpdisc_length(zm, gait_steps(steps, b, smax, int(n_steps[b]))) for b in range(B)]
    assert lens == [w[0] for w in want]
    lcap = max(lens)
    d_steps = torch.from_numpy(np.frombuffer(steps, dtype=np.uint8).copy()).cuda()
    d_ns = torch.from_numpy(np.ascontiguousarray(n_steps)).cuda()
    d_init = torch.from_numpy(np.ascontiguousarray(init)).cuda()
    lf = torch.full((lcap, 6, B), float("nan"), dtype=torch.float64, device="cuda")
    rf = torch.full_like(lf, float("nan"))
    ln = torch.zeros(B, dtype=torch.int32, device="cuda")
    rc = wg.lib().wg_zmpdisc_full_batch_dev(C.byref(zm), B, smax, d_steps.data_ptr(), d_ns.data_ptr(), d_init.data_ptr(), lcap, None,
                                            None, None, None, lf.data_ptr(), None, rf.data_ptr(), None, ln.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert ln.cpu().numpy().tolist() == lens
    lz, rz = lf[:, 2, :].cpu().numpy(), rf[:, 2, :].cpu().numpy()
    for b in range(B):
        L, wl, wr = want[b]
        assert lz[:L, b].tobytes() == wl.tobytes() and rz[:L, b].tobytes() == wr.tobytes(), (i, b)
