"""The CPU checker pool of the fleet parity tests (tests/fleet_oracle.py) checked on the host: its pool equals the oracle's
own C loop, its per-tick diagnostics equal a plain wgo_mpc_tick loop, its comparator names the gait that differs and
takes NaNs as NaNs but nothing else, its digest sees every word, and its workers never hold torch or the HIP runtime."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fleet_oracle as fo  # noqa: E402
import workload as w  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")                 # POD layouts only: no library load
B, T, REDRAW = 16, 60, 25                                       # redraws at ticks 0, 25 and 50


def _lib():
    lib = C.CDLL(fo.build_oracle())
    lib.wgo_mpc_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _model(lib):
    m = wg.Model()
    lib.wgo_model_defaults(C.byref(m))
    return m


def _start(lib, model):
    s = wg.GaitState()
    lib.wgo_gait_init(C.byref(model), C.byref(s), *((C.c_double * 3)(*v) for v in (w.START_COM, w.START_LEFT, w.START_RIGHT)))
    s.nb_steps_left = w.STEPS_BEFORE_STOP
    return s


def _vel(n_seg, n):
    r = np.random.default_rng(60)
    return np.stack([r.uniform(-0.1, 0.3, (n_seg, n)), r.uniform(-0.1, 0.1, (n_seg, n)), r.uniform(-0.2, 0.2, (n_seg, n))], 2)


@pytest.fixture(scope="module")
def pooled():
    lib = _lib()
    model = _model(lib)
    s0 = _start(lib, model)
    vel = _vel((T + REDRAW - 1) // REDRAW, B)
    with fo.make_pool(3) as pool:
        job = fo.submit(pool, fo.layout_of(wg), bytes(model), bytes(s0), vel, REDRAW, T, keep_ticks=(0, 37, T - 1),
                        chunks=[5, 2, 9])
        dig = fo.submit(pool, fo.layout_of(wg), bytes(model), bytes(s0), vel, REDRAW, T, keep_ticks=(37,), outs="digest",
                        chunks=[7, 9])
        res, res_dig = job.result(300), dig.result(300)
    return lib, model, s0, vel, res, res_dig


def test_pool_equals_the_oracles_own_run_loop(pooled):
    lib, model, s0, vel, res, _ = pooled
    states = (wg.GaitState * B)(*([s0] * B))
    assert lib.wgo_mpc_run(C.byref(model), states, B, T, vel.ctypes.data_as(C.c_void_p), REDRAW) == 0
    assert res["states"] == bytes(states)
    st = (wg.GaitState * B).from_buffer_copy(res["states"])
    assert all(s.tick_count == T for s in st)
    assert len({bytes(s) for s in st}) == B                    # every gait its own references
    assert all(tuple(s.vref) == tuple(vel[2, g]) for g, s in enumerate(st))   # the third stretch's references were set


def test_pool_diag_and_outs_equal_a_plain_tick_loop(pooled):
    lib, model, s0, vel, res, res_dig = pooled
    diag = np.zeros((T, B, 6), dtype=np.int32)
    outs = {}
    o = wg.TickOut()

    def on_tick(t, s):
        diag[t, g] = o.ifail, o.n_iter, o.nact, o.n, o.m, o.nb_prw_steps
        outs.setdefault(t, []).append(bytes(o))
        C.memset(C.byref(o), 0, C.sizeof(o))                   # every tick writes into a zeroed struct, as in the pool
    for g in range(B):
        w.oracle_follow(lib, model, s0, vel[:, g], T, redraw=REDRAW, out=o, on_tick=on_tick)
    assert np.array_equal(res["diag"], diag)
    assert (diag[..., 0] == 0).all() and (diag[..., 1] > 0).all() and set(np.unique(diag[..., 3])) <= {32, 34, 36}
    for t in (0, 37, T - 1):
        assert res["outs"][t] == b"".join(outs[t]), t
    osz = C.sizeof(wg.TickOut)
    want = fo.digest(np.frombuffer(b"".join(outs[37]), dtype=np.uint64).reshape(B, osz // 8))
    assert np.array_equal(res_dig["outs"][37], want)


def test_pool_workers_hold_neither_torch_nor_the_hip_runtime(pooled):
    res, res_dig = pooled[4], pooled[5]
    reports = res["workers"] + res_dig["workers"]
    assert len(reports) == 5 and os.getpid() not in {r["pid"] for r in reports}
    for r in reports:
        assert not r["torch"] and r["libs"] == [], r


def _states(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, C.sizeof(wg.GaitState) // 8)).view(np.uint64)


def test_comparator_names_the_gait_with_one_flipped_bit():
    sz = C.sizeof(wg.GaitState)
    names = fo.word_names(wg.GaitState)
    a = _states(64, 1)
    b = a.copy()
    w = wg.GaitState.com_y.offset // 8 + 1
    b[41, w] ^= np.uint64(1)
    assert fo.record_mismatches(a, a.copy(), sz) == []
    bad = fo.record_mismatches(a, b, sz, nan_aware=True, names=names)
    assert [(r, f) for r, f, _, _ in bad] == [(41, "com_y[1]")]
    with pytest.raises(AssertionError, match=r"1 of 64 gaits differ .* gait 1041 field com_y\[1\]"):
        fo.assert_records_equal(a, b, sz, "states", names=names, first=1000)
    d = np.zeros((5, 64, 6), dtype=np.int32)
    d2 = d.copy()
    d2[3, 17, 1] = 1
    with pytest.raises(AssertionError, match="gait 17 tick 3 n_iter"):
        fo.assert_diag_equal(d, d2, "diag")
    assert fo.word_names(wg.TickOut)[2] == "ifail|n_iter" and fo.word_names(wg.TickOut)[-1] == "pad_[14]"


_NAN_X86, _NAN_GFX = np.uint64(0xFFF8000000000000), np.uint64(0x7FF8000000000000)
_NAN_PAYLOAD = np.uint64(0x7FF0000000000001)
_PINF, _NINF = np.uint64(0x7FF0000000000000), np.uint64(0xFFF0000000000000)
_ONE = np.float64(1.0).view(np.uint64)


@pytest.mark.parametrize("x,y,same", [(_NAN_X86, _NAN_GFX, True), (_NAN_PAYLOAD, _NAN_X86, True),
                                      (_NAN_GFX, _PINF, False), (_NINF, _NAN_X86, False), (_NAN_GFX, _ONE, False),
                                      (_PINF, _NINF, False), (_PINF, _PINF, True)])
def test_comparator_takes_nans_as_nans_and_nothing_else(x, y, same):
    sz = C.sizeof(wg.GaitState)
    a = _states(4, 2)
    b = a.copy()
    a[2, 7], b[2, 7] = x, y
    assert fo.record_mismatches(a, b, sz) == ([] if x == y else [(2, 7, "0x%016x" % int(x), "0x%016x" % int(y))])
    assert (fo.record_mismatches(a, b, sz, nan_aware=True) == []) == same


def test_digest_sees_every_word_and_only_a_nans_sign_is_forgiven():
    osz = C.sizeof(wg.TickOut) // 8
    base = np.random.default_rng(3).uniform(-1, 1, osz).view(np.uint64)
    for nan_aware in (False, True):
        d0 = fo.digest(base, nan_aware)
        flip = np.repeat(base[None], osz, 0)
        flip[np.arange(osz), np.arange(osz)] ^= np.uint64(1 << 63)   # the sign bit, one word per row
        assert (fo.digest(flip, nan_aware) != d0).all()
        low = np.repeat(base[None], osz, 0)
        low[np.arange(osz), np.arange(osz)] ^= np.uint64(1)
        assert (fo.digest(low, nan_aware) != d0).all()
    n = base.copy()
    n[100] = _NAN_GFX
    m = n.copy()
    m[100] = _NAN_X86
    assert fo.digest(n, True) == fo.digest(m, True) and fo.digest(n) != fo.digest(m)
    m[100] = _PINF
    assert fo.digest(n, True) != fo.digest(m, True)
