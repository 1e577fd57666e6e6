"""Morisawa-2007 analytic walks on the device, through the C ABI (wg_morisawa_solve_dev, _sample_dev, _walk_dev, their fleet forms and
_ctx twins) against the host twins (wg_morisawa_solve, _solve_fleet, _sample: the same arithmetic compiled for the host, held to the
restatement and to the reference's golden files in tests/test_morisawa_host.py and tests/test_morisawa_golden.py): the same BYTES --
blocks, statuses, every output for k < length and the last sample repeated past it -- with canaries before and behind every array.
B = 67: one wave-group of gaits and three, at smax 3, 7 and 14 (n = 64: every lane a row); the fleets of tests/morisawa_fleets.py.
Each fleet is solved and sampled on the host once and shared."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import morisawa_fleets as mf

wg = mf.wg()
pytestmark = pytest.mark.gpu

B = 67
SENT_D, SENT_I = -7.25, -77
OUT_I = ("left_type", "right_type")
TOL = 2e-7


def to_dev(a):
    import torch
    if not isinstance(a, np.ndarray):
        a = np.frombuffer(bytes(memoryview(a).cast("B")), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


@functools.lru_cache(maxsize=None)
def case(smax):
    """the fleet, and what the host twins make of it with one model ("one") and with a model per gait ("per"); never modified"""
    f = mf.Fleet(B, smax, 500 + smax, golden_first=smax == 7)
    t0 = mf.t_start_of(f.model)
    out = dict(fleet=f, t0=t0, words=wg.morisawa_block_bytes(smax) // 8)
    for key, model in (("one", f.model), ("per", f.models)):
        blocks, status = wg.morisawa_solve(model, f.steps, f.n_steps, f.init_feet, f.com0, smax)
        assert list(status) == [0] * B
        lcap = mf.lcap_for(f, key == "per")
        out[key] = dict(blocks=blocks, status=status, lcap=lcap, samples=wg.morisawa_sample(blocks, status, smax, t0, f.model.T, lcap))
        assert (out[key]["samples"]["length"] > 100).all() and len(set(out[key]["samples"]["length"])) > 1
    return out


class Dev:
    """the fleet's inputs on the device, and sentinel-filled outputs with a canary row (block, entry) before and behind each"""

    def __init__(self, f, words, lcap, outputs=wg.MORISAWA_OUTPUTS):
        import torch
        self.f, self.words, self.lcap = f, words, lcap
        self.steps, self.n_steps = to_dev(f.steps), to_dev(f.n_steps)
        self.feet, self.com0, self.models = to_dev(f.init_feet), to_dev(f.com0), to_dev(f.models)
        self.blocks = torch.full((f.B + 2, words), SENT_D, dtype=torch.float64, device="cuda")
        self.status = torch.full((f.B + 2,), SENT_I, dtype=torch.int32, device="cuda")
        self.length = torch.full((f.B + 2,), SENT_I, dtype=torch.int32, device="cuda")
        shape = dict(zmp_x=(f.B,), zmp_y=(f.B,), com=(4, f.B), left=(6, f.B), right=(6, f.B), left_type=(f.B,), right_type=(f.B,))
        self.outs = {k: torch.full((lcap + 2,) + shape[k], SENT_I if k in OUT_I else SENT_D,
                                   dtype=torch.int32 if k in OUT_I else torch.float64, device="cuda") for k in outputs}

    def solve_args(self, model=None):
        m = self.models.data_ptr() if model is None else model
        return (m, self.f.B, self.f.smax, self.steps.data_ptr(), self.n_steps.data_ptr(), self.feet.data_ptr(), self.com0.data_ptr(),
                self.blocks[1:].data_ptr(), self.status[1:].data_ptr())

    def out_ptrs(self):
        return {k: v[1:].data_ptr() for k, v in self.outs.items()}

    def check_blocks(self, blocks, status, refused=()):
        import torch
        torch.cuda.synchronize()
        got, st = self.blocks.cpu().numpy(), self.status.cpu().numpy()
        assert (got[0] == SENT_D).all() and (got[-1] == SENT_D).all() and st[0] == SENT_I and st[-1] == SENT_I
        assert list(st[1:-1]) == list(status)
        for b in range(self.f.B):
            if b in refused:
                assert (got[1 + b] == SENT_D).all(), b
            else:
                assert got[1 + b].tobytes() == blocks[b].tobytes(), b

    def check_outs(self, samples, refused=()):
        import torch
        torch.cuda.synchronize()
        ln = self.length.cpu().numpy()
        assert ln[0] == SENT_I and ln[-1] == SENT_I and list(ln[1:-1]) == list(samples["length"])
        keep = [b for b in range(self.f.B) if b not in refused]
        for k, t in self.outs.items():
            got, sent = t.cpu().numpy(), (SENT_I if k in OUT_I else SENT_D)
            assert (got[0] == sent).all() and (got[-1] == sent).all(), k
            assert got[1:-1][..., keep].tobytes() == np.ascontiguousarray(samples[k][..., keep]).tobytes(), k
            for b in refused:
                assert (got[..., b] == sent).all(), (k, b)


@pytest.mark.parametrize("smax", (3, 7, 14))
def test_solve_sample_and_walk_give_the_host_twins_bytes(smax):
    c = case(smax)
    f, h = c["fleet"], c["one"]
    d = Dev(f, c["words"], h["lcap"])
    wg.morisawa_solve_dev(*d.solve_args(f.model))
    d.check_blocks(h["blocks"], h["status"])
    wg.morisawa_sample_dev(f.B, smax, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), c["t0"], f.model.T, h["lcap"], d.out_ptrs(),
                           d.length[1:].data_ptr())
    d.check_outs(h["samples"])
    lens = h["samples"]["length"]
    got = d.outs["zmp_x"].cpu().numpy()[1:-1]
    for b in (0, 1, 66):                                                   # past a gait's length: its last sample again
        assert lens[b] < h["lcap"] and (got[lens[b]:, b] == got[lens[b] - 1, b]).all()
    w = Dev(f, c["words"], h["lcap"])
    wg.morisawa_walk_dev(f.model, f.B, smax, *w.solve_args(f.model)[3:], c["t0"], h["lcap"], w.out_ptrs(), w.length[1:].data_ptr())
    w.check_blocks(h["blocks"], h["status"])
    w.check_outs(h["samples"])


@pytest.mark.parametrize("smax", (3, 7, 14))
def test_model_per_gait_and_broadcast(smax):
    """a model per gait: gait b has the bytes of the one-model call with model b (the host's fleet twin, shown equal to exactly that in
    tests/test_morisawa_host.py; three gaits once more here on the device); one model broadcast: the one-model call"""
    import torch
    c = case(smax)
    f, h = c["fleet"], c["per"]
    d = Dev(f, c["words"], h["lcap"])
    wg.morisawa_walk_dev(d.models.data_ptr(), f.B, smax, *d.solve_args()[3:], c["t0"], h["lcap"], d.out_ptrs(), d.length[1:].data_ptr(),
                         T=f.model.T)
    d.check_blocks(h["blocks"], h["status"])
    d.check_outs(h["samples"])
    for b in (2, 33, 66):
        o = Dev(f, c["words"], 1)
        wg.morisawa_solve_dev(*o.solve_args(f.models[b]))
        torch.cuda.synchronize()
        assert torch.equal(o.blocks[1 + b].view(torch.int64), d.blocks[1 + b].view(torch.int64))      # as bits: packed ints may spell a NaN
    same = Dev(f, c["words"], c["one"]["lcap"])
    same.models = to_dev((wg.MorisawaModel * f.B)(*[f.model] * f.B))
    wg.morisawa_solve_dev(*same.solve_args())
    same.check_blocks(c["one"]["blocks"], c["one"]["status"])


def test_every_combination_of_null_outputs():
    import torch
    c = case(3)
    f, h = c["fleet"], c["one"]
    blocks, status = to_dev(h["blocks"]), to_dev(h["status"])
    ref = {k: to_dev(h["samples"][k]) for k in wg.MORISAWA_OUTPUTS}
    ref_len = to_dev(h["samples"]["length"])
    for n in range(len(wg.MORISAWA_OUTPUTS) + 1):
        for keys in itertools.combinations(wg.MORISAWA_OUTPUTS, n):
            for with_length in ((True, False) if n in (0, 7) else (True,)):
                d = Dev(f, 1, h["lcap"], outputs=keys)
                wg.morisawa_sample_dev(f.B, 3, blocks.data_ptr(), status.data_ptr(), c["t0"], f.model.T, h["lcap"], d.out_ptrs(),
                                       d.length[1:].data_ptr() if with_length else None)
                torch.cuda.synchronize()
                for k in keys:
                    sent = SENT_I if k in OUT_I else SENT_D
                    assert torch.equal(d.outs[k][1:-1], ref[k]) and (d.outs[k][0] == sent).all() and (d.outs[k][-1] == sent).all(), (keys, k)
                assert torch.equal(d.length[1:-1], ref_len) if with_length else (d.length == SENT_I).all()


def test_second_context_and_stream():
    import torch
    c = case(7)
    f, h = c["fleet"], c["one"]
    st = torch.cuda.Stream()
    d = Dev(f, c["words"], h["lcap"])
    torch.cuda.synchronize()
    with wg.Context(0) as ctx:
        outs = d.out_ptrs()
        rc = ctx.call("wg_morisawa_walk_dev", C.addressof(f.model), f.B, 7, *d.solve_args()[3:], c["t0"], h["lcap"],
                      *[outs[k] for k in wg.MORISAWA_OUTPUTS], d.length[1:].data_ptr(), st.cuda_stream)
        assert rc == 0, wg.lib().wg_last_error()
        rc = ctx.call("wg_morisawa_sample_dev", f.B, 7, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), c["t0"], f.model.T, h["lcap"],
                      *[outs[k] for k in wg.MORISAWA_OUTPUTS], d.length[1:].data_ptr(), st.cuda_stream)       # a second clock, behind the first
        assert rc == 0, wg.lib().wg_last_error()
        st.synchronize()
        d.check_blocks(h["blocks"], h["status"])
        d.check_outs(h["samples"])


def test_refusals_on_the_device():
    """S = 1, S = 15 at smax = 14, t_double = 0, a NaN height, omega dT > 40 -- one gait each, in one fleet with a model per gait: the
    host's codes, blocks and outputs of the refused gaits byte-identical to their canaries, every other gait as if nothing had happened"""
    f = mf.Fleet(B, 14, 514)
    t0, lcap = mf.t_start_of(f.model), mf.lcap_for(f, True)
    good, st0 = wg.morisawa_solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, 14)
    assert list(st0) == [0] * B
    bad = (1, 20, 40, 63, 66)
    f.n_steps[1] = 1
    f.n_steps[20] = 15
    f.models[40].t_double = 0.0
    f.com0[63, 2] = float("nan")
    f.com0[66, 2] = 0.01
    blocks, status = wg.morisawa_solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, 14, blocks=np.full_like(good, SENT_D))
    assert all(status[b] == wg.MORISAWA_BAD_INPUT for b in bad) and sum(status != 0) == len(bad)
    assert all(blocks[b].tobytes() == good[b].tobytes() for b in range(B) if b not in bad)
    samples = wg.morisawa_sample(blocks, status, 14, t0, f.model.T, lcap)
    d = Dev(f, blocks.shape[1], lcap)
    wg.morisawa_walk_dev(d.models.data_ptr(), B, 14, *d.solve_args()[3:], t0, lcap, d.out_ptrs(), d.length[1:].data_ptr(), T=f.model.T)
    d.check_blocks(blocks, status, refused=bad)
    d.check_outs(samples, refused=bad)
    # a walk that does not fit its rows: WG_MORISAWA_CAPACITY for that gait alone
    lens = samples["length"]
    short = int(np.median(lens[lens > 0]))
    s2 = wg.morisawa_sample(blocks, status, 14, t0, f.model.T, short)
    over = tuple(int(b) for b in np.nonzero(s2["length"] == wg.MORISAWA_CAPACITY)[0])
    assert over and len(over) < B - len(bad)
    e = Dev(f, blocks.shape[1], short)
    wg.morisawa_sample_dev(B, 14, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), t0, f.model.T, short, e.out_ptrs(), e.length[1:].data_ptr())
    e.check_outs(s2, refused=bad + over)


def test_host_side_errors_launch_nothing():
    c = case(3)
    f = c["fleet"]
    d = Dev(f, c["words"], 8)
    lib, a = wg.lib(), d.solve_args(C.addressof(f.model))
    assert lib.wg_morisawa_solve_dev(*a[:2], 15, *a[3:], None) == -2
    assert lib.wg_morisawa_solve_dev(None, *a[1:], None) == -2
    assert lib.wg_morisawa_solve_dev(*a[:8], None, None) == -2
    o = [d.out_ptrs()[k] for k in wg.MORISAWA_OUTPUTS]
    for t0, T, lcap in ((-1.0, 0.005, 8), (0.0, 0.0, 8), (0.0, float("nan"), 8), (0.0, 0.005, 0)):
        assert lib.wg_morisawa_sample_dev(f.B, 3, d.blocks[1:].data_ptr(), None, t0, T, lcap, *o, None, None) == -2
    assert lib.wg_morisawa_solve_dev(a[0], 0, *a[2:], None) == 0
    d.check_blocks(np.zeros((f.B, 0)), [SENT_I] * f.B, refused=range(f.B))


def test_golden_walk_as_gait_0_of_a_mixed_fleet():
    """the reference's short walk is gait 0 of the smax = 7 fleet whose 66 other gaits differ in everything: within 2e-7 of every
    recorded column of the 32-bit golden file (tests/test_morisawa_golden.py says why the older file's foot x, y are another curve)"""
    import torch
    c = case(7)
    f, h = c["fleet"], c["per"]
    g = np.load(mf.GOLDEN)
    names, K = [str(n) for n in g["names"]], len(g["data32"])
    d = Dev(f, c["words"], h["lcap"])
    wg.morisawa_walk_dev(d.models.data_ptr(), f.B, 7, *d.solve_args()[3:], c["t0"], h["lcap"], d.out_ptrs(), d.length[1:].data_ptr(), T=f.model.T)
    torch.cuda.synchronize()
    assert int(d.length[1]) == K == 1588
    o = {k: v.cpu().numpy()[1:1 + K] for k, v in d.outs.items()}
    col = lambda n: g["data32"][:, names.index(n)]  # noqa: E731
    worst = 0.0
    for i, n in enumerate(("com_x", "dcom_x", "com_y", "dcom_y")):
        worst = max(worst, np.abs(o["com"][:, i, 0] - col(n)).max())
    worst = max(worst, np.abs(o["zmp_x"][:, 0] - col("zmp_x")).max(), np.abs(o["zmp_y"][:, 0] - col("zmp_y")).max())
    for foot in ("left", "right"):
        for i, a in enumerate(("x", "y", "z", "theta", "omega", "omega2")):
            worst = max(worst, np.abs(o[foot][:, i, 0] - col("%s_%s" % (foot, a))).max())
    print("device walk vs the 32-bit golden file: %.3g" % worst)
    assert worst <= TOL
