"""The lane-parallel phases of the N = 16 active-set iteration outside its two serial chains -- the violation scan and its
selection among the lanes' candidates, Z^T a of the new normal with its chunk skip and its step-column tail, the sweep's
phases 2 and 3, the x / lambda update, the drop, the residual refresh -- held to the CPU oracle on the sample
tests/test_iteration_paths_gpu.py defines and shares: B = 64 gaits x 48 ticks of the benchmark's recipe at 1, 3 and 7 times
its velocity references.  The oracle's run of a scale is computed once (that module's cache) and used by both files.

What this file adds to that module's comparison (diag rows of every tick, final states against wgo_mpc_run, the last tick's
add / drop history):
  * the run through one wg_mpc_tick_batch_dev launch per tick asks for the add / drop history of EVERY tick and holds all
    48 x 64 of them to the oracle's, event by event: the selections of the scan and of the ratio test leave their choice
    there, iteration by iteration, where the diag row only has the counts;
  * the staged multi-tick run (wg_mpc_run_sched_dev) and the per-tick run must agree with each other byte for byte as well;
  * test_sample_exercises_the_lane_phases asserts, from the oracle alone, that the sample reaches the forms those phases
    have:
      - QPs of n = 34 and n = 36, i.e. Z^T a's step-column tail of two and of four columns.  n = 32 -- no tail -- is NOT
        reachable on this recipe, at this size or any other: n = 2 N + 2 ns, and ns = 0 needs a tick whose whole horizon
        (16 x 0.1 s) lies inside the current support phase, which lasts 0.8 s; every tick of a walking gait previews one
        step or two (832 ticks with one, 2240 with two, at each of the three scales).  The tail of no column is the same
        code with neither of its two tests taken; the assert below states what the sample has and fails if that changes;
      - an iteration that adds a CoP row of instant 0 (only the first chunk of each half of Z's column is walked) and one
        of instant 15 (every chunk is);
      - a drop inside the step loop, which is followed by a second sweep over the shortened factor (the oracle's
        `step = ratio * sumy` site, counted by the instrumented solve of tests/test_iteration_paths_gpu.py);
      - a residual refresh after the first one of a solve (an add with itref > 0 goes to the refresh again: that module's
        third counter), once in the sample, at seven times the references."""
import ctypes as C

import numpy as np
import pytest

import herdt_replay as hr
import test_iteration_paths_gpu as ip
import workload as w

pytestmark = pytest.mark.gpu

B, T, SCALES = ip.B, ip.T, ip.SCALES
N = 16
COP_FIRST, COP_LAST = 2, 1 + 4 * N                              # history codes of the CoP rows: row k (1 .. 4 N) is logged as k + 1


def _instant(code):
    return (code - COP_FIRST) >> 2


def _gpu_every_history(scale):
    """One wg_mpc_tick_batch_dev launch per tick, each with its history."""
    import torch
    wg = ip._wg()
    model = wg.model_defaults()
    wg.mpc_configure(model)
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


@pytest.mark.parametrize("scale", SCALES)
def test_both_entry_points_follow_the_oracle_with_every_ticks_history(scale):
    import fleet_oracle as fo
    wg = ip._binding()
    ref = ip._oracle(scale)
    final, diag, hist, hlen = _gpu_every_history(scale)
    what = "scale %g, wg_mpc_tick_batch_dev" % scale
    fo.assert_diag_equal(ref["diag"], diag, what)
    fo.assert_records_equal(ref["final"], final, C.sizeof(wg.GaitState), what + ": final states", names=fo.word_names(wg.GaitState))
    assert final == ref["final"], what
    for t in range(T):
        for g in range(B):
            h = ref["hists"][t][g]
            assert int(hlen[t, g]) == len(h), (what, "history length", t, g, int(hlen[t, g]), len(h))
            got = tuple(int(v) for v in hist[t, g, :len(h)])
            if got != h:
                first = next(i for i in range(len(h)) if got[i] != h[i])
                raise AssertionError((what, "history", t, g, "event", first, got[first], h[first]))
    final_run, diag_run, _, _ = ip._gpu(scale, True)
    what = "scale %g, wg_mpc_run_sched_dev" % scale
    fo.assert_diag_equal(ref["diag"], diag_run, what)
    fo.assert_records_equal(ref["final"], final_run, C.sizeof(wg.GaitState), what + ": final states", names=fo.word_names(wg.GaitState))
    assert final_run == ref["final"], what
    assert final_run == final and (diag_run == diag).all(), "the two entry points disagree at scale %g" % scale


def test_sample_exercises_the_lane_phases():
    n_ticks = {32: 0, 34: 0, 36: 0}
    adds_at = {0: 0, N - 1: 0}
    step_drops = later_refresh = 0
    for scale in SCALES:
        ref = ip._oracle(scale)
        d = ref["diag"]
        for n in n_ticks:
            n_ticks[n] += int((d[:, :, 3] == n).sum())
        for row in ref["hists"]:
            for h in row:
                for e in h:
                    if COP_FIRST <= e <= COP_LAST and _instant(e) in adds_at:
                        adds_at[_instant(e)] += 1
        step_drops += int((ref["paths"][:, :, ip.PATHS.index("reduced_step")] > 0).sum())
        later_refresh += int((ref["paths"][:, :, ip.PATHS.index("add_after_refresh")] > 0).sum())
    print("ticks by n:", n_ticks, "adds of CoP rows by instant:", adds_at, "ticks with a drop in the step loop:", step_drops,
          "ticks with a second refresh:", later_refresh)
    assert n_ticks[34] > 0 and n_ticks[36] > 0, n_ticks
    assert n_ticks[32] == 0, ("the recipe now has ticks without a previewed step: the docstring's statement on n = 32 no longer "
                              "holds, assert their presence instead", n_ticks)
    assert n_ticks[34] + n_ticks[36] == len(SCALES) * T * B, n_ticks
    assert adds_at[0] > 0 and adds_at[N - 1] > 0, adds_at
    assert step_drops > 0 and later_refresh > 0, (step_drops, later_refresh)
