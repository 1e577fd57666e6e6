"""BASELINE configs 4 and 5 at their stated sizes, on one GPU, through the C ABI's device entry points (the path bench.py
times): wg_mpc_set_velref_dev + wg_mpc_tick_batch_dev / wg_mpc_run_batch_dev on resident states.

  config 4  "Herdt2010 N=16 fp64, batch=32768 sharded across 8 GPUs": ALL EIGHT shards, one after the other on this GPU, each
            run exactly as bench.py's rank r would run it (global gaits 4096 r .. 4096 r + 4095, seeds 20100 + global index,
            200 ticks, references redrawn every 50), a seeded sample of every shard followed bit for bit by the CPU oracle; the
            same job split four ways gives the same bytes; the shard boundaries and references are bench.py's own.  (RCCL with
            >= 2 ranks is unmeasured on hardware here: the 8-GPU launch itself needs the 8-GPU node.)
  config 5  "Herdt2010 N=32 with foot-placement decision vars, batch=8192": the full batch through the element view, 50
            ticks, as properties -- every QP solves, determinism (two runs, same bytes), batch-composition invariance
            (a permuted sub-batch reproduces its gaits' bytes), multi-tick launch == one launch per tick -- plus a seeded
            sample followed bit for bit by the oracle.  The solve is fp64 (an fp32 solver would be
            narrower than the reference's arithmetic); the fp32 part of the config is the MFMA Gramian as Hessian source,
            run here at full size as a tolerance mode."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import workload as w  # noqa: E402
from workload import REDRAW  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu


def _run_dev(model, gaits, n_ticks, **kw):
    return w.run_dev(wg, model, gaits, n_ticks, **kw)


def _oracle_follow(pt, model, g, n_ticks):
    return w.oracle_follow(pt, model, w.start_state(wg.gait_init, model), w.velocity(g, (n_ticks + REDRAW - 1) // REDRAW), n_ticks,
                           per_tick=int(round(model.T / model.Tctrl)))


# ---------------------------------------------------------------------------------------------------------- config 4
# "Herdt2010 N=16 fp64, batch=32768 sharded across 8 GPUs": ALL eight shards, one after the other on this one GPU, each run
# exactly as bench.py's rank r would run it (global gaits [4096 r, 4096 (r + 1)), seeds 20100 + global index, 200 ticks,
# references redrawn every 50).  What one GPU cannot show is the RCCL launch itself: RCCL with >= 2 ranks is UNMEASURED ON
# HARDWARE in this repository (tests/test_shard_gloo.py covers the rank bookkeeping on gloo; the driver's SCALE run is the
# only place the 8-GPU job can happen).
C4_B, C4_T, C4_WORLD = 4096, 200, 8


@pytest.fixture(scope="module")
def config4_shards():
    wg.init(0)
    model = wg.model_defaults()
    wg.mpc_configure(model)
    shard = importlib.import_module("jrl-walkgen_amd.shard")
    runs = []
    for rank in range(C4_WORLD):
        lo, hi = shard.shard_range(C4_WORLD * C4_B, rank, C4_WORLD)
        assert (lo, hi) == (rank * C4_B, (rank + 1) * C4_B)
        fin, diag = _run_dev(model, list(range(lo, hi)), C4_T)
        runs.append((lo, hi, fin, diag))
    return model, runs


def test_config4_all_eight_shards_full_size(config4_shards):
    """every one of the 32 768 gaits x 200 ticks = 6 553 600 QPs solves; each shard holds different problems; a seeded sample
    of EVERY shard is followed tick by tick by the CPU oracle to the same bytes"""
    model, runs = config4_shards
    pt = w.ptrig()
    seen = set()
    for rank, (lo, hi, fin, diag) in enumerate(runs):
        assert int((diag[:, :, 0] != 0).sum()) == 0, rank
        assert set(np.unique(diag[:, :, 3]).tolist()) <= {32, 34, 36} and diag[:, :, 1].max() < 200
        st = (wg.GaitState * C4_B).from_buffer_copy(fin.tobytes())
        assert all(s.tick_count == C4_T and s.running == 1 for s in st)
        com = np.array([[s.com_x[0], s.com_y[0]] for s in st]); feet = np.array([[s.lf[2].x, s.lf[2].y, s.rf[2].x, s.rf[2].y] for s in st])
        assert np.isfinite(com).all() and np.abs(com - 0.5 * (feet[:, :2] + feet[:, 2:])).max() < 0.35
        rows = {r.tobytes() for r in fin}
        assert len(rows) > 4000 and not (rows & seen), rank        # different problems, and different from every other shard's
        seen |= rows
        rng = np.random.default_rng(32768 + rank)
        for k in sorted(set(rng.choice(C4_B, 6, replace=False).tolist()) | {0, C4_B - 1}):
            assert _oracle_follow(pt, model, lo + k, C4_T) == fin[k].tobytes(), lo + k


def test_config4_results_do_not_depend_on_the_split(config4_shards):
    """the same 32 768 gaits split over FOUR ranks (8192 per GPU: other batch sizes, other wave placement, other queue
    traffic): rank q's bytes are shards 2q and 2q + 1 of the eight-way job, byte for byte"""
    model, runs = config4_shards
    shard = importlib.import_module("jrl-walkgen_amd.shard")
    for q in range(4):
        lo, hi = shard.shard_range(C4_WORLD * C4_B, q, 4)
        assert (lo, hi) == (2 * q * C4_B, (2 * q + 2) * C4_B)
        fin, diag = _run_dev(model, list(range(lo, hi)), C4_T, want_diag=(q == 0))
        assert np.array_equal(fin[:C4_B], runs[2 * q][2]) and np.array_equal(fin[C4_B:], runs[2 * q + 1][2]), q
        if q == 0:
            assert np.array_equal(diag[:, :C4_B], runs[0][3]) and np.array_equal(diag[:, C4_B:], runs[1][3])


def test_config4_last_shard_of_eight_full_size(config4_shards):
    """rank 7 of world 8, 4096 gaits per GPU: global gaits [28672, 32768)"""
    bench = w.bench_module()
    model, runs = config4_shards
    B, T, rank = C4_B, C4_T, 7
    lo, hi, fin, diag = runs[rank]
    assert (lo, hi) == (28672, 32768)
    # the references this shard gets are bench.py's table for those global indices (not a re-seeded local table)
    tab = bench.velocity_table(lo, lo + 3, 4)
    for k in range(3):
        assert np.array_equal(tab[:, k, :], w.velocity(lo + k, 4))
    assert not np.array_equal(w.velocity(lo, 4), w.velocity(0, 4))
    # a larger seeded sample of this shard on the CPU oracle: same bytes
    pt = w.ptrig()
    rng = np.random.default_rng(32768)
    sample = sorted(set(rng.choice(B, 38, replace=False).tolist()) | {0, B - 1})
    for k in sample:
        assert _oracle_follow(pt, model, lo + k, T) == fin[k].tobytes(), lo + k
    # one launch per tick on a slice of the shard: same bytes as the multi-tick launches
    sl = list(range(lo + 1000, lo + 1300))
    fin2, _ = _run_dev(model, sl, T, multi_tick=False, want_diag=False)
    assert np.array_equal(fin2, fin[1000:1300])


# ---------------------------------------------------------------------------------------------------------- config 5
@pytest.fixture(scope="module")
def config5_run():
    wg.init(0)
    model = wg.model_defaults()
    model.N = 32
    wg.mpc_configure(model)
    B, T = 8192, 50
    fin, diag = _run_dev(model, list(range(B)), T)
    yield model, B, T, fin, diag
    wg.mpc_configure(wg.model_defaults())


def test_config5_full_size_solves_and_uses_all_previewed_steps(config5_run):
    model, B, T, fin, diag = config5_run
    assert int((diag[:, :, 0] != 0).sum()) == 0                    # 409 600 QPs, none failed
    sizes = set(np.unique(diag[:, :, 3]).tolist())
    assert max(sizes) == 72 and min(sizes) >= 64                    # n = 2N + 2s, s up to 4: foot-placement variables kept
    assert int(diag[:, :, 4].max()) == 1 + 4 * 32 + 5 * 4           # m = 149
    st = (wg.GaitState * B).from_buffer_copy(fin.tobytes())
    assert all(s.tick_count == T and s.running == 1 for s in st)
    com = np.array([[s.com_x[0], s.com_y[0]] for s in st]); feet = np.array([[s.lf[2].x, s.lf[2].y, s.rf[2].x, s.rf[2].y] for s in st])
    assert np.isfinite(com).all() and np.abs(com - 0.5 * (feet[:, :2] + feet[:, 2:])).max() < 0.35
    assert len({r.tobytes() for r in fin}) > 8000


def test_config5_full_size_sample_followed_by_the_oracle(config5_run):
    model, B, T, fin, diag = config5_run
    pt = w.ptrig()
    rng = np.random.default_rng(8192)
    sample = sorted(set(rng.choice(B, 14, replace=False).tolist()) | {0, B - 1})
    for g in sample:
        assert _oracle_follow(pt, model, g, T) == fin[g].tobytes(), g


def test_config5_bench_plan_at_the_timed_size(config5_run):
    """bench.py's config5 leg as it issues it (B = 8192, N = 32: warm-up = ticks [0, 10), timed = ONE launch of ticks
    [10, 50) through wg_mpc_run_batch_dev): same bytes and the same ifail / iterations / n / m per QP as the fixture's run."""
    model, B, T, fin, diag = config5_run
    bench = w.bench_module()
    assert B == bench.CONFIG5_BATCH and T == 50
    fin2, diag2, names = w.bench_plan_run(wg, model, B, T, 10, bench)
    assert names == ["wg_mpc_tick_batch_dev", "wg_mpc_tick_batch_dev", "wg_mpc_run_batch_dev", "wg_mpc_run_batch_dev"]
    assert np.array_equal(diag2, diag)
    assert b"".join(fin2) == fin.tobytes()


def test_config5_determinism_and_batch_composition_invariance(config5_run):
    model, B, T, fin, diag = config5_run
    fin_again, diag_again = _run_dev(model, list(range(B)), T)
    assert np.array_equal(fin_again, fin) and np.array_equal(diag_again, diag)
    perm = np.random.default_rng(5).permutation(B)[:700].tolist()    # other order, other batch size, other neighbours
    fin_p, _ = _run_dev(model, perm, T, want_diag=False)
    assert np.array_equal(fin_p, fin[perm])
    sl = list(range(4000, 4400))                                   # one launch per tick == multi-tick launches
    fin_s, _ = _run_dev(model, sl, T, multi_tick=False, want_diag=False)
    assert np.array_equal(fin_s, fin[4000:4400])


def test_config5_full_size_with_the_fp32_matrix_core_gramian(config5_run):
    """the config as BASELINE words it: Q_b from the fp32 MFMA Gramian.  A tolerance mode: every QP still
    solves at full size, iteration counts stay where they were, and the closed loop stays within 1 mm of the fp64 run
    over these 5 s of walking."""
    model, B, T, fin, diag = config5_run
    m = wg.model_defaults(); m.N = 32; m.flags = 4                   # WG_FLAG_GRAMIAN_MFMA_F32
    try:
        wg.mpc_configure(m)
        fin32, diag32 = _run_dev(m, list(range(B)), T)
    finally:
        wg.mpc_configure(model)
    assert int((diag32[:, :, 0] != 0).sum()) == 0
    assert abs(diag32[:, :, 1].mean() - diag[:, :, 1].mean()) < 0.5
    a = (wg.GaitState * B).from_buffer_copy(fin.tobytes()); b = (wg.GaitState * B).from_buffer_copy(fin32.tobytes())
    dev = max(max(abs(x.com_x[0] - y.com_x[0]), abs(x.com_y[0] - y.com_y[0])) for x, y in zip(a, b))
    assert 0.0 < dev < 1e-3, dev
