"""The N = 16 solver's guarded sums on the device (jrl-walkgen_amd/csrc/wg_ql_guard.hpp): whichever way the four
decision-only sums are formed, the tick computes the oracle's bytes.

The sample of tests/test_iteration_paths_gpu.py (B = 64 gaits x 48 ticks of the benchmark's recipe, velocity references x 1, 3
and 7: drops, dependent normals, reduced steps, resets, failed QPs) runs under each setting of WG_QL_SUMS, read when the model is
configured:
  unset     tree sums under the certificates; a doubt at the dependence test forms that iteration's sums in the reference's order,
            a doubt at the magnitude test runs the solve again in the reference's order;
  ordered   the reference's order throughout (the parent's behaviour);
  doubt     the dependence certificate doubts in every iteration and every finished solve is doubted as a whole: the local
            fallback everywhere, and a second pass that starts from the dirtiest state a first pass can leave.
Each through one wg_mpc_tick_batch_dev launch per tick with EVERY tick's add / drop history, and through the staged multi-tick
launch (wg_mpc_run_sched_dev; the last tick with its history).  Diag rows, histories and final states must equal the oracle's
(computed once per scale by that module and shared) byte for byte -- and so each other's."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import herdt_replay as hr
import test_iteration_paths_gpu as ip
import workload as w

pytestmark = pytest.mark.gpu

MODES = (None, "ordered", "doubt")


@pytest.fixture
def sums_mode():
    """Sets WG_QL_SUMS for the configuration the test makes; afterwards the context is configured again without it."""
    old = os.environ.get("WG_QL_SUMS")

    def set_mode(mode):
        if mode is None:
            os.environ.pop("WG_QL_SUMS", None)
        else:
            os.environ["WG_QL_SUMS"] = mode
    yield set_mode
    set_mode(old)
    wg = ip._wg()
    wg.mpc_configure(wg.model_defaults())


def _per_tick_with_histories(scale):
    """ip._gpu's per-tick form, but every launch returns its history."""
    import torch
    wg = ip._wg()
    model = wg.model_defaults()
    wg.mpc_configure(model)
    B, T = ip.B, ip.T
    states = w.to_device(w.start_bytes(wg.gait_init, model), B)
    vt = torch.from_numpy(np.ascontiguousarray(ip._table(scale))).cuda()
    diag = torch.zeros(T, B, 6, dtype=torch.int32, device="cuda")
    hist = torch.zeros(T, B, hr.HIST_CAP, dtype=torch.int32, device="cuda")
    hlen = torch.zeros(T, B, dtype=torch.int32, device="cuda")
    sp = states.data_ptr()
    wg.mpc_set_velref_dev(B, sp, vt[0].data_ptr())
    for t in range(T):
        wg.mpc_tick_batch_dev(B, sp, None, diag[t].data_ptr(), w.advance_calls(t), hist[t].data_ptr(), hr.HIST_CAP, hlen[t].data_ptr())
    torch.cuda.synchronize()
    return states.cpu().numpy().tobytes(), diag.cpu().numpy(), hist.cpu().numpy(), hlen.cpu().numpy()


@pytest.mark.parametrize("scale", ip.SCALES)
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m or "unset")
def test_one_launch_per_tick_every_history(mode, scale, sums_mode):
    import fleet_oracle as fo
    wg = ip._binding()
    sums_mode(mode)
    ref = ip._oracle(scale)
    final, diag, hist, hlen = _per_tick_with_histories(scale)
    what = "WG_QL_SUMS=%s, scale %g, wg_mpc_tick_batch_dev" % (mode, scale)
    fo.assert_diag_equal(ref["diag"], diag, what)
    for t in range(ip.T):
        for g in range(ip.B):
            h = ref["hists"][t][g]
            assert int(hlen[t, g]) == len(h) and tuple(int(v) for v in hist[t, g, :len(h)]) == h, (what, "history", t, g)
    fo.assert_records_equal(ref["final"], final, C.sizeof(wg.GaitState), what + ": final states", names=fo.word_names(wg.GaitState))
    assert final == ref["final"], what


@pytest.mark.parametrize("scale", ip.SCALES)
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m or "unset")
def test_staged_multi_tick_launch(mode, scale, sums_mode):
    sums_mode(mode)
    ip._compare(scale, True)


def test_an_unknown_setting_is_refused(sums_mode):
    wg = ip._wg()
    sums_mode("sometimes")
    with pytest.raises(Exception):
        wg.mpc_configure(wg.model_defaults())
