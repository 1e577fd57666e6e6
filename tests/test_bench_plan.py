"""bench.py's host-side bookkeeping (no GPU): the launch plan covers exactly the timed ticks, never crosses a change of the
velocity references, keeps the control loop's first two ticks apart; the algorithmic-bytes formula is SURVEY 8(d)'s; the
synthetic references are the same for a gait whatever shard it lands in.  And the pins that hold tests/workload.py -- the
workload as the suite and the tools state it -- to bench.py's own copy: either side drifting fails here."""
import os

import numpy as np

import workload as w
from workload import bench_module as _bench


def test_launch_plan_covers_ticks_and_respects_redraws():
    b = _bench()
    for t0, t1 in ((0, 50), (50, 250), (20, 220), (0, 3), (7, 8), (49, 51), (100, 100)):
        for per_tick in (False, True):
            for staged in (False, True):
                plan = b.launch_plan(t0, t1, per_tick, staged=staged)
                ticks = [t for s, n in plan for t in range(s, s + n)]
                assert ticks == list(range(t0, t1))
                for s, n in plan:
                    one_segment = s // b.REDRAW_TICKS == (s + n - 1) // b.REDRAW_TICKS
                    # a launch crosses a change of the references only if it starts on one (then they are staged on the device)
                    assert n >= 1 and (one_segment or (staged and s % b.REDRAW_TICKS == 0))
                    assert n == 1 or (s >= 2 and not per_tick)
    assert b.launch_plan(50, 250, staged=False) == [(50, 50), (100, 50), (150, 50), (200, 50)]
    assert b.launch_plan(50, 250) == [(50, 200)]
    assert b.launch_plan(20, 220) == [(20, 30), (50, 170)]
    assert b.launch_plan(0, 50)[:3] == [(0, 1), (1, 1), (2, 48)]


def test_algorithmic_bytes_is_the_ql0001_boundary():
    b = _bench()
    # n = 36, m = 75 (mmax = 76): 8 (n^2 + n + mmax n + mmax + 2n) read + 8 (n + m + 2n) written = 33 728 + 1 464
    assert b.algorithmic_bytes(36, 75) == 33728 + 1464
    assert b.algorithmic_bytes(32, 65) == 8 * (32 * 32 + 32 + 66 * 32 + 66 + 64) + 8 * (32 + 65 + 64)     # no previewed step


def test_velocity_table_is_per_gait_deterministic():
    b = _bench()
    a = b.velocity_table(0, 8, 3)
    c = b.velocity_table(4, 12, 3)
    assert np.array_equal(a[:, 4:8], c[:, 0:4])                   # gait g draws the same references in any shard
    assert (a[..., 0] >= -0.1).all() and (a[..., 0] <= 0.3).all() and (np.abs(a[..., 1]) <= 0.1).all() and (np.abs(a[..., 2]) <= 0.2).all()


def test_cpu_baseline_worker_count_is_what_the_process_may_use(monkeypatch):
    """"1 core and all host cores; the harness prints the core count" -- the count is the affinity mask
    cut down by the cgroup quota (or, with no limit visible on a many-core host, one GPU lease's share), never os.cpu_count()
    of a shared host; the line reports what was seen, what was used and the parallel efficiency."""
    b = _bench()
    used, seen = b.usable_cores()
    assert 1 <= used <= len(os.sched_getaffinity(0)) <= seen["os_cpu_count"]
    assert used <= max(b.BOX_CPU_SHARE, int(seen["cgroup_quota"] or 0)) or seen["affinity"] < seen["os_cpu_count"]
    monkeypatch.setenv("WG_BENCH_CPU_CORES", "2")
    assert b.usable_cores()[0] == min(2, used)
    one, allc = b.cpu_baseline(8, 4)                                # a token sample: the bookkeeping, not a measurement
    assert allc["cores_used"] == min(2, used) and allc["value"] > 0 and 0 < allc["parallel_efficiency"]
    assert allc["worker_rate_min"] <= allc["worker_rate_max"] and allc["cores_visible"] == seen["os_cpu_count"]


def test_dump_outputs_writes_every_field_as_float64_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: one float64 array per field of the gaits' states, the last tick's diag row and (with --outs-on) its outs,
    gait-major; over the size limit a fixed sample of gaits, the same on every run, with the gaits it kept."""
    import ctypes as C
    b = _bench()
    wg = b.wg
    B = 40
    states = (wg.GaitState * B)()
    for g in range(B):
        states[g].clock = 0.005 * g
        states[g].lf[1].x = -g
    snap = {"states": np.frombuffer(bytes(states), dtype=np.uint8), "diag": np.arange(B * 6, dtype=np.int32),
            "outs": np.zeros(B * C.sizeof(wg.TickOut), dtype=np.uint8)}
    b.dump_outputs(str(tmp_path / "all"), snap, 4096)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert all(a.dtype == np.float64 and len(a) == B for a in got.values())
    assert np.array_equal(got["gait_index"], 4096 + np.arange(B)) and np.array_equal(got["state_clock"], 0.005 * np.arange(B))
    assert np.array_equal(got["state_lf_x"][:, 1], -np.arange(B)) and got["diag"].shape == (B, 6) and got["diag"][1, 0] == 6
    assert "outs_zmp_x" in got and got["outs_com_x"].shape == (B, wg.SAMPLES, 3) and not any("pad" in k for k in got)
    monkeypatch.setattr(b, "DUMP_LIMIT_BYTES", 100000)               # bench.py is loaded once per process: put the limit back
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), snap, 0)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= b.DUMP_LIMIT_BYTES
    kept = np.load(tmp_path / "s1" / "gait_index.npy")
    assert 0 < len(kept) < B and np.array_equal(kept, np.load(tmp_path / "s2" / "gait_index.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "state_clock.npy"), 0.005 * kept)


# ------------------------------------------------------------------------------- tests/workload.py pinned to bench.py
def test_workload_references_are_bench_pys_table():
    b = _bench()
    assert w.REDRAW == b.REDRAW_TICKS
    for lo, hi, n in ((0, 8, 3), (4, 12, 7), (7 * 4096, 7 * 4096 + 5, 9), (4095, 4096, 1)):
        tab = b.velocity_table(lo, hi, n)
        got = w.velocity_table(lo, hi, n)
        assert got.dtype == tab.dtype and got.shape == tab.shape == (n, hi - lo, 3) and np.array_equal(got, tab)
        for k, g in enumerate(range(lo, hi)):
            assert np.array_equal(w.velocity(g, n), tab[:, k])
    assert not np.array_equal(w.velocity(0, 4), w.velocity(1, 4))


def test_workload_start_state_is_bench_pys():
    b = _bench()
    wg = b.wg
    for N, B in ((16, 3), (32, 2)):
        model = wg.model_defaults()
        model.N = N
        want = b.start_states(model, B).numpy().tobytes()
        assert w.start_bytes(wg.gait_init, model, B) == want == w.state_bytes(w.start_array(wg.gait_init, model, B))
        s = w.start_state(wg.gait_init, model)
        assert s.nb_steps_left == w.STEPS_BEFORE_STOP == 2 and (s.com_x[0], s.com_y[0]) == w.START_COM[:2]
        assert (s.lf[2].y, s.rf[2].y) == (w.START_LEFT[1], w.START_RIGHT[1]) == (0.09, -0.09)


def test_workload_clock_schedule():
    """The clock advances by 1, 19, 20, 20, ... control periods, by repeated addition of Tctrl.  That is not clock + n * Tctrl:
    over the first 400 ticks of the default model the two differ in the last bits on nearly every tick (398 of 400 when this
    was written), and a checker that multiplied would leave the kernels' bytes at once."""
    wg = _bench().wg
    model = wg.model_defaults()
    per_tick = int(round(model.T / model.Tctrl))
    assert per_tick == 20
    assert [w.advance_calls(t) for t in range(5)] == [1, 19, 20, 20, 20] == [w.advance_calls(t, per_tick) for t in range(5)]
    assert [w.advance_calls(t, 10) for t in range(4)] == [1, 9, 10, 10]
    s = w.start_state(wg.gait_init, model)
    literal = s.clock
    differs = 0
    for t in range(400):
        n = 1 if t == 0 else (19 if t == 1 else 20)
        multiplied = s.clock + n * model.Tctrl
        for _ in range(n):
            literal += model.Tctrl
        w.advance_clock(s, model, n)
        assert s.clock.hex() == literal.hex(), t
        differs += s.clock != multiplied
    assert abs(s.clock - 7980 * model.Tctrl) < 1e-9 and differs > 0
