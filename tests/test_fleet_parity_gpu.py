"""Every gait of the timed fleets against the CPU oracle, at the sizes bench.py times.

The oracle (oracle/libwg_oracle_ptrig.so, the kernels' bit-exact partner) runs on a pool of spawned host processes
(tests/fleet_oracle.py).  The module queues the oracle side of every selected test first, so that it works while the GPU
runs; each test then collects its own part.  Inputs are bench.py's own (velocity_table, start_states, launch_plan,
table_segments), never a copy of the recipe:

  a. bench.py --gpus 1 --steps 20 --warmup 5 --outs-on --dump-outputs, the command of record, as a subprocess: its dumped
     states, last diag row and last tick's wg_tick_out_t for all 4096 gaits;
  b. bench.py's default run (pre-roll + warm-up to tick 150, then the 200-tick wg_mpc_run_sched_dev launch), 4096 gaits:
     every tick's diag and the final states;
  c. config 5 (N = 32, 8192 gaits) through the plan bench.config5_leg issues: every tick's diag and the final states;
  d. an overdriven slice (the references times 3, as SOAK_VSCALE=3) through one 200-tick wg_mpc_run_sched_dev launch, where
     gaits are lost to NaN solves: states and the last tick's outs NaN-aware, every tick's diag exact.

tests/test_fullsize_gpu.py and tests/test_configs45_gpu.py keep their sampled checks of the host-pointer path."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_oracle as fo  # noqa: E402
import workload as w  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# a: bench.py --steps 20 --warmup 5 (its pre-roll of 100 ticks comes first): ticks [0, 125), the last one timed
A_K, A_W0 = 20, 5
# b: bench.py's defaults, K = 200, W = 50 + 100
B_K, B_W = 200, 150
# c: bench.config5_leg's plan, ticks [0, 10) warm-up, [10, 50) timed
C_T, C_WARM = 50, 10
# d: gaits [0, 512) with the references times 3; launches of ticks 0 | 1 | 2-49 | 50-249 (one wg_mpc_run_sched_dev), then
# one wg_mpc_tick_batch_dev at tick 250 (the stretch that starts there is the table's sixth) that stores the outs
D_B, D_T, D_SCALE = 512, 250, 3.0


def _workloads(bench):
    """test name -> (N, B, n_ticks, velocity table, ticks whose outs are kept, NaN-aware)"""
    R = bench.REDRAW_TICKS
    a_t = A_K + A_W0 + bench.PREROLL_TICKS
    return {
        "test_a_bench_command_of_record_every_gait": (16, bench.BATCH_PER_GPU, a_t,
                                                      lambda: bench.velocity_table(0, bench.BATCH_PER_GPU,
                                                                                   bench.table_segments(A_K, A_W0 + bench.PREROLL_TICKS)),
                                                      (a_t - 1,), False),
        "test_b_bench_default_run_every_gait_every_tick": (16, bench.BATCH_PER_GPU, B_K + B_W,
                                                           lambda: bench.velocity_table(0, bench.BATCH_PER_GPU,
                                                                                        bench.table_segments(B_K, B_W)), (), False),
        "test_c_config5_every_gait_every_tick": (32, bench.CONFIG5_BATCH, C_T,
                                                 lambda: bench.velocity_table(0, bench.CONFIG5_BATCH, (C_T + R - 1) // R), (), False),
        "test_d_overdriven_slice_through_the_multi_tick_launch": (16, D_B, D_T + 1,
                                                                  lambda: bench.velocity_table(0, D_B, D_T // R + 1) * D_SCALE,
                                                                  (D_T,), True),
    }


@pytest.fixture(scope="module")
def fleet(request):
    """bench.py as a module, and the oracle runs of the selected tests, queued in test order on one pool"""
    bench = w.bench_module()
    wg.init(0)
    work = _workloads(bench)
    wanted = [it.name for it in request.session.items if it.module is request.module and it.name in work]
    fo.build_oracle()
    layout = fo.layout_of(wg)
    workers = fo.pool_size(bench)
    jobs = {}
    with fo.make_pool(workers) as pool:
        for name in wanted:
            N, B, T, table, keep, nan_aware = work[name]
            model = wg.model_defaults()
            model.N = N
            start = bench.start_states(model, B).numpy().tobytes()
            jobs[name] = (fo.submit(pool, layout, bytes(model), start, table(), bench.REDRAW_TICKS, T, keep_ticks=keep,
                                    nan_aware=nan_aware), table)
        print("\noracle for %s queued on %d processes" % (", ".join(n.split("_")[1] for n in wanted), workers))
        yield bench, layout, jobs
        wg.mpc_configure(wg.model_defaults())


def _collect(job):
    return job.result(timeout=900)


def _live(diag, n_set, what):
    """no vacuous pass: every tick the oracle ran solved a QP of an expected size, with iterations"""
    sizes = set(np.unique(diag[..., 3]).tolist())
    assert sizes <= n_set and len(sizes) > 1, (what, sizes)
    assert int(diag[..., 1].min()) > 0, what


def _tick_counts(states, B, T):
    st = (wg.GaitState * B).from_buffer_copy(states)
    assert all(s.tick_count == T for s in st)


def test_a_bench_command_of_record_every_gait(fleet, tmp_path):
    """bench.py's command of record with the deliverable stored: what it dumps after its last timed step -- every gait's state,
    that tick's diag row and its wg_tick_out_t -- equals, field by field, what the oracle holds after the same 125 ticks of
    the same table (bench.dump_outputs on both sides)."""
    bench, layout, jobs = fleet
    job, _ = jobs["test_a_bench_command_of_record_every_gait"]
    B, T = bench.BATCH_PER_GPU, A_K + A_W0 + bench.PREROLL_TICKS
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(A_K), "--warmup", str(A_W0),
                        "--outs-on", "--dump-outputs", str(tmp_path / "gpu")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = _collect(job)
    _live(res["diag"], {34, 36}, "a")
    _tick_counts(res["states"], B, T)
    bench.dump_outputs(str(tmp_path / "cpu"), {"states": np.frombuffer(res["states"], dtype=np.uint8),
                                               "diag": np.ascontiguousarray(res["diag"][T - 1]),
                                               "outs": np.frombuffer(res["outs"][T - 1], dtype=np.uint8)}, 0)
    names = sorted(os.listdir(tmp_path / "gpu"))
    assert names == sorted(os.listdir(tmp_path / "cpu"))
    assert {"diag.npy", "gait_index.npy", "state_clock.npy", "outs_jerk_x.npy", "outs_lf_x.npy"} <= set(names)
    assert np.array_equal(np.load(tmp_path / "gpu" / "gait_index.npy"), np.arange(B))      # the dump holds every gait
    gpu_diag = np.load(tmp_path / "gpu" / "diag.npy")
    assert gpu_diag.shape == (B, 6) and (gpu_diag[:, 0] == 0).all()
    bad = {}
    for f in names:
        a, b = np.load(tmp_path / "cpu" / f), np.load(tmp_path / "gpu" / f)
        assert a.shape == b.shape and a.dtype == b.dtype == np.float64, f
        ne = (a.view(np.uint64) != b.view(np.uint64)).reshape(B, -1).any(axis=1)
        for g in np.flatnonzero(ne)[:8]:
            bad.setdefault(int(g), []).append(f[:-4])
    assert not bad, "gaits whose dumped fields differ from the oracle: %s" % "; ".join(
        "gait %d: %s" % (g, ", ".join(fs[:6])) for g, fs in sorted(bad.items())[:8])
    print("a: %d of %d gaits, ticks [0, %d): states, diag and outs of tick %d equal the oracle's (%d fields)"
          % (B, B, T, T - 1, len(names)))


def test_b_bench_default_run_every_gait_every_tick(fleet):
    """bench.py's default run (K = 200, W = 150, its table of table_segments(200, 150) stretches): the pre-roll + warm-up
    launches and the 200-tick wg_mpc_run_sched_dev launch it times.  Every gait's diag at every one of the 350 ticks, and its
    final state, equal the oracle's."""
    bench, layout, jobs = fleet
    job, _ = jobs["test_b_bench_default_run_every_gait_every_tick"]
    B, T = bench.BATCH_PER_GPU, B_K + B_W
    model = wg.model_defaults()
    wg.mpc_configure(model)
    fin, diag, names = w.bench_plan_run(wg, model, B, T, B_W, bench, n_seg=bench.table_segments(B_K, B_W))
    assert names == ["wg_mpc_tick_batch_dev", "wg_mpc_tick_batch_dev", "wg_mpc_run_batch_dev", "wg_mpc_run_sched_dev",
                     "wg_mpc_run_sched_dev"]                      # ticks 0 | 1 | 2-49 | 50-149 | 150-349 (timed)
    res = _collect(job)
    _live(res["diag"], {34, 36}, "b")
    _tick_counts(res["states"], B, T)
    fo.assert_diag_equal(res["diag"], diag, "b: diag")
    fo.assert_records_equal(res["states"], b"".join(fin), layout["state_size"], "b: final states",
                            names=fo.word_names(wg.GaitState))
    print("b: %d of %d gaits x %d ticks: every diag row and every final state equal the oracle's" % (B, B, T))


def test_c_config5_every_gait_every_tick(fleet):
    """config 5 (N = 32, B = 8192) through the plan bench.config5_leg issues (warm-up [0, 10), one wg_mpc_run_batch_dev
    launch of ticks [10, 50), a one-stretch table): every diag row of the 50 ticks and every final state equal the oracle's."""
    bench, layout, jobs = fleet
    job, _ = jobs["test_c_config5_every_gait_every_tick"]
    B, T = bench.CONFIG5_BATCH, C_T
    model = wg.model_defaults()
    model.N = 32
    wg.mpc_configure(model)
    try:
        fin, diag, names = w.bench_plan_run(wg, model, B, T, C_WARM, bench)
    finally:
        wg.mpc_configure(wg.model_defaults())
    assert names == ["wg_mpc_tick_batch_dev", "wg_mpc_tick_batch_dev", "wg_mpc_run_batch_dev", "wg_mpc_run_batch_dev"]
    res = _collect(job)
    _live(res["diag"], {70, 72}, "c")
    _tick_counts(res["states"], B, T)
    fo.assert_diag_equal(res["diag"], diag, "c: diag")
    fo.assert_records_equal(res["states"], b"".join(fin), layout["state_size"], "c: final states",
                            names=fo.word_names(wg.GaitState))
    print("c: %d of %d gaits x %d ticks at N = 32: every diag row and every final state equal the oracle's" % (B, B, T))


def test_d_overdriven_slice_through_the_multi_tick_launch(fleet):
    """Gaits [0, 512) of the benchmark workload with the references times 3 (0.9 m/s asked of a 0.7 m robot), the same table on
    both sides: ticks 50-249 are one wg_mpc_run_sched_dev launch, inside which QPs go inconsistent (ifail > 10), iterates go NaN
    and solves run to maxit (ifail = 1): gaits are lost.  The first 512 gaits meet the liveness counts below (round 5's soak:
    2 680 of 4 096 lost by tick 250).  Every diag row exact; the final states (after one more tick, 250, through
    wg_mpc_tick_batch_dev with the outs stored) and that tick's outs NaN-aware: a NaN matches a NaN whatever its sign bit."""
    import torch
    bench, layout, jobs = fleet
    job, table = jobs["test_d_overdriven_slice_through_the_multi_tick_launch"]
    B, T, R = D_B, D_T, bench.REDRAW_TICKS
    n_seg = T // R + 1
    model = wg.model_defaults()
    wg.mpc_configure(model)
    fin, diag, names = w.bench_plan_run(wg, model, B, T, T, bench, n_seg=n_seg, vel_scale=D_SCALE)
    assert names == ["wg_mpc_tick_batch_dev", "wg_mpc_tick_batch_dev", "wg_mpc_run_batch_dev", "wg_mpc_run_sched_dev"]
    states = w.to_device(b"".join(fin))
    vlast = torch.from_numpy(np.ascontiguousarray(table()[T // R])).cuda()
    outs = torch.zeros(B * layout["out_size"], dtype=torch.uint8, device="cuda")
    dlast = torch.zeros(B, 6, dtype=torch.int32, device="cuda")
    wg.mpc_set_velref_dev(B, states.data_ptr(), vlast.data_ptr())
    wg.mpc_tick_batch_dev(B, states.data_ptr(), outs.data_ptr(), dlast.data_ptr(), w.advance_calls(T))
    torch.cuda.synchronize()
    gpu_diag = np.concatenate([diag, dlast.cpu().numpy()[None]])
    res = _collect(job)
    d = res["diag"]
    lost = fo.nan_gaits(res["states"], layout["state_size"])
    n_maxit = int((d[R:T, :, 0] == 1).sum())
    n_incons = int((d[..., 0] > 10).sum())
    print("d: %d of %d gaits x %d ticks (references x %g): %d maxit exits inside the multi-tick launch, %d inconsistent QPs, "
          "%d gaits end with NaNs in their state" % (B, B, T + 1, D_SCALE, n_maxit, n_incons, lost))
    assert n_maxit > 0 and n_incons > 0 and lost >= 0.2 * B
    fo.assert_diag_equal(d, gpu_diag, "d: diag")
    fo.assert_records_equal(res["states"], states.cpu().numpy().tobytes(), layout["state_size"], "d: final states",
                            nan_aware=True, names=fo.word_names(wg.GaitState))
    fo.assert_records_equal(res["outs"][T], outs.cpu().numpy().tobytes(), layout["out_size"], "d: outs of tick %d" % T,
                            nan_aware=True, names=fo.word_names(wg.TickOut))
