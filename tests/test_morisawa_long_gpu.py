"""The long Morisawa family on the device, through the C ABI (wg_morisawa_long_solve_dev, _long_sample_dev, _long_walk_dev, their fleet
forms and _ctx twins) against its host twins (wg_morisawa_long_solve, _long_solve_fleet, _long_sample: the same arithmetic compiled
for the host, held to the short family, the restatement and the 50-digit truth in tests/test_morisawa_long_host.py): the same BYTES
-- blocks, statuses, every output for k < length and the last sample repeated past it -- with canaries before and behind every
array.  B = 67 at smax = 2 (n = 16: every window of the elimination is clipped by the matrix edge), 15, 33 and 64 (gait 0 has 64
steps, gait 1 two).  At smax = 14 the device band is held to the device's dense elimination by value.  Each fleet is solved and
sampled on the host once and shared."""
import ctypes as C
import functools

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


def fleet_for(smax):
    f = mf.Fleet(B, smax, 600 + smax, golden_first=smax == 15)
    f.n_steps[2] = smax                             # a walk of the full length whatever gait 0 is
    if smax == 64:                                  # the shortest support times of the tables: lcap stays below about 8000
        for b in range(B):
            f.models[b].t_single = min(mf.SINGLE_TICKS) * f.model.T
            f.models[b].t_double = min(mf.DOUBLE_TICKS) * f.model.T
        f.model.t_single, f.model.t_double = f.models[0].t_single, f.models[0].t_double
    return f


def lcap_of(f, per_gait, pad=3):
    t0 = mf.t_start_of(f.model)
    return max(wg.morisawa_long_length(f.model_of(b, per_gait), int(f.n_steps[b]), t0) for b in range(f.B)) + pad


@functools.lru_cache(maxsize=None)
def case(smax, sampled=True):
    """the fleet, and what the host twins make of it with one model ("one") and with a model per gait ("per"); never modified"""
    f = fleet_for(smax)
    t0 = mf.t_start_of(f.model)
    out = dict(fleet=f, t0=t0, words=wg.morisawa_long_block_bytes(smax) // 8)
    for key, model in (("one", f.model), ("per", f.models)):
        blocks, status = wg.morisawa_long_solve(model, f.steps, f.n_steps, f.init_feet, f.com0, smax)
        assert list(status) == [0] * B
        out[key] = dict(blocks=blocks, status=status)
        if sampled:
            lcap = lcap_of(f, key == "per")
            out[key].update(lcap=lcap, samples=wg.morisawa_long_sample(blocks, status, smax, t0, f.model.T, lcap))
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


@pytest.mark.parametrize("smax", (2, 15, 33, 64))
def test_long_solve_gives_the_host_twins_bytes(smax):
    """one-model and fleet forms; three gaits of the fleet form once more as one-model calls handed the gait's model"""
    import torch
    c = case(smax) if smax in (15, 64) else case(smax, sampled=False)
    f = c["fleet"]
    d = Dev(f, c["words"], 1)
    wg.morisawa_long_solve_dev(*d.solve_args(f.model))
    d.check_blocks(c["one"]["blocks"], c["one"]["status"])
    p = Dev(f, c["words"], 1)
    wg.morisawa_long_solve_dev(*p.solve_args())
    p.check_blocks(c["per"]["blocks"], c["per"]["status"])
    for b in (2, 66):
        o = Dev(f, c["words"], 1)
        wg.morisawa_long_solve_dev(*o.solve_args(f.models[b]))
        torch.cuda.synchronize()
        assert torch.equal(o.blocks[1 + b].view(torch.int64), p.blocks[1 + b].view(torch.int64))


@pytest.mark.parametrize("smax", (15, 64))
def test_long_sample_and_walk_give_the_host_twins_bytes(smax):
    c = case(smax)
    f, h = c["fleet"], c["one"]
    assert h["lcap"] < 8200
    d = Dev(f, c["words"], h["lcap"])
    wg.morisawa_long_solve_dev(*d.solve_args(f.model))
    wg.morisawa_long_sample_dev(f.B, smax, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), c["t0"], f.model.T, h["lcap"], d.out_ptrs(),
                                d.length[1:].data_ptr())
    d.check_blocks(h["blocks"], h["status"])
    d.check_outs(h["samples"])
    lens = h["samples"]["length"]
    got = d.outs["zmp_x"].cpu().numpy()[1:-1]
    for b in (0, 1, 66):                                                   # past a gait's length: its last sample again
        assert lens[b] < h["lcap"] and (got[lens[b]:, b] == got[lens[b] - 1, b]).all()
    del d
    g = c["per"]
    w = Dev(f, c["words"], g["lcap"])
    wg.morisawa_long_walk_dev(w.models.data_ptr(), f.B, smax, *w.solve_args()[3:], c["t0"], g["lcap"], w.out_ptrs(), w.length[1:].data_ptr(),
                              T=f.model.T)
    w.check_blocks(g["blocks"], g["status"])
    w.check_outs(g["samples"])


def test_long_walk_one_model_form():
    c = case(15)
    f, h = c["fleet"], c["one"]
    w = Dev(f, c["words"], h["lcap"])
    wg.morisawa_long_walk_dev(f.model, f.B, 15, *w.solve_args(f.model)[3:], c["t0"], h["lcap"], w.out_ptrs(), w.length[1:].data_ptr())
    w.check_blocks(h["blocks"], h["status"])
    w.check_outs(h["samples"])


def test_each_output_null_alone_and_resident_alone():
    """smax = 15: each of the seven outputs absent with the others resident, and each alone resident: 14 launches"""
    import torch
    c = case(15)
    f, h = c["fleet"], c["one"]
    blocks, status = to_dev(h["blocks"]), to_dev(h["status"])
    ref = {k: to_dev(h["samples"][k]) for k in wg.MORISAWA_OUTPUTS}
    ref_len = to_dev(h["samples"]["length"])
    sets = [tuple(k for k in wg.MORISAWA_OUTPUTS if k != out) for out in wg.MORISAWA_OUTPUTS] + [(k,) for k in wg.MORISAWA_OUTPUTS]
    assert len(sets) == 14
    for keys in sets:
        d = Dev(f, 1, h["lcap"], outputs=keys)
        wg.morisawa_long_sample_dev(f.B, 15, blocks.data_ptr(), status.data_ptr(), c["t0"], f.model.T, h["lcap"], d.out_ptrs(),
                                    d.length[1:].data_ptr())
        torch.cuda.synchronize()
        for k in keys:
            sent = SENT_I if k in OUT_I else SENT_D
            assert torch.equal(d.outs[k][1:-1], ref[k]) and (d.outs[k][0] == sent).all() and (d.outs[k][-1] == sent).all(), (keys, k)
        assert torch.equal(d.length[1:-1], ref_len)


def test_device_band_is_device_dense():
    """smax = 14: one fleet through wg_morisawa_walk_dev and wg_morisawa_long_walk_dev; every output equal by value, the pivots equal"""
    import torch
    f = mf.Fleet(B, 14, 614)
    t0, lcap = mf.t_start_of(f.model), mf.lcap_for(f, True)
    s = Dev(f, wg.morisawa_block_bytes(14) // 8, lcap)
    wg.morisawa_walk_dev(s.models.data_ptr(), B, 14, *s.solve_args()[3:], t0, lcap, s.out_ptrs(), s.length[1:].data_ptr(), T=f.model.T)
    l = Dev(f, wg.morisawa_long_block_bytes(14) // 8, lcap)
    wg.morisawa_long_walk_dev(l.models.data_ptr(), B, 14, *l.solve_args()[3:], t0, lcap, l.out_ptrs(), l.length[1:].data_ptr(), T=f.model.T)
    torch.cuda.synchronize()
    assert torch.equal(s.status, l.status) and (s.status[1:-1] == 0).all()
    assert torch.equal(s.length, l.length) and (s.length[1:-1] > 100).all()
    for k in wg.MORISAWA_OUTPUTS:
        a, b_ = s.outs[k].cpu().numpy(), l.outs[k].cpu().numpy()
        assert np.array_equal(a, b_), k                                       # by value: +0 == -0
    sb, lb = s.blocks.cpu().numpy(), l.blocks.cpu().numpy()
    for b in range(B):
        vs, vl = wg.morisawa_view(sb[1 + b], 14), wg.morisawa_long_view(lb[1 + b], 14)
        assert list(vs["piv"]) == list(vl["piv"]), b
        assert np.array_equal(vs["yx"], vl["yx"]) and np.array_equal(vs["yy"], vl["yy"]), b


def test_long_golden_walk_as_gait_0_of_a_mixed_fleet():
    """the reference's short walk is gait 0 of the smax = 15 fleet whose 66 other gaits differ in everything: within 2e-7 of every
    recorded column of the 32-bit golden file, as tests/test_morisawa_gpu.py holds the short family"""
    import torch
    c = case(15)
    f, h = c["fleet"], c["per"]
    g = np.load(mf.GOLDEN)
    names, K = [str(n) for n in g["names"]], len(g["data32"])
    d = Dev(f, c["words"], h["lcap"])
    wg.morisawa_long_walk_dev(d.models.data_ptr(), f.B, 15, *d.solve_args()[3:], c["t0"], h["lcap"], d.out_ptrs(), d.length[1:].data_ptr(),
                              T=f.model.T)
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
    print("device long walk vs the 32-bit golden file: %.3g" % worst)
    assert worst <= TOL


def test_long_second_context_and_stream():
    import torch
    c = case(15)
    f, h = c["fleet"], c["one"]
    st = torch.cuda.Stream()
    d = Dev(f, c["words"], h["lcap"])
    e = Dev(f, c["words"], h["lcap"])
    torch.cuda.synchronize()
    with wg.Context(0) as ctx:
        outs = d.out_ptrs()
        rc = ctx.call("wg_morisawa_long_walk_dev", C.addressof(f.model), f.B, 15, *d.solve_args()[3:], c["t0"], h["lcap"],
                      *[outs[k] for k in wg.MORISAWA_OUTPUTS], d.length[1:].data_ptr(), st.cuda_stream)
        assert rc == 0, wg.lib().wg_last_error()
        # the default context on the default stream next to it
        wg.morisawa_long_walk_dev(f.model, f.B, 15, *e.solve_args(f.model)[3:], c["t0"], h["lcap"], e.out_ptrs(), e.length[1:].data_ptr())
        rc = ctx.call("wg_morisawa_long_sample_dev", f.B, 15, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), c["t0"], f.model.T, h["lcap"],
                      *[outs[k] for k in wg.MORISAWA_OUTPUTS], d.length[1:].data_ptr(), st.cuda_stream)       # a second clock, behind the first
        assert rc == 0, wg.lib().wg_last_error()
        st.synchronize()
        d.check_blocks(h["blocks"], h["status"])
        d.check_outs(h["samples"])
    e.check_blocks(h["blocks"], h["status"])
    e.check_outs(h["samples"])


def test_long_refusals_on_the_device():
    """S = 1, S = 16 at smax = 15, t_double = 0, a NaN height, omega dT > 40 -- one gait each, in one fleet with a model per gait: the
    host's codes, blocks and outputs of the refused gaits byte-identical to their canaries, every other gait as if nothing had happened;
    then a short block handed to the long sampler"""
    f = mf.Fleet(B, 15, 615)
    t0, lcap = mf.t_start_of(f.model), lcap_of(f, True)
    good, st0 = wg.morisawa_long_solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, 15)
    assert list(st0) == [0] * B
    bad = (1, 20, 40, 63, 66)
    f.n_steps[1] = 1
    f.n_steps[20] = 16
    f.models[40].t_double = 0.0
    f.com0[63, 2] = float("nan")
    f.com0[66, 2] = 0.01
    blocks, status = wg.morisawa_long_solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, 15, blocks=np.full_like(good, SENT_D))
    assert all(status[b] == wg.MORISAWA_BAD_INPUT for b in bad) and sum(status != 0) == len(bad)
    assert all(blocks[b].tobytes() == good[b].tobytes() for b in range(B) if b not in bad)
    samples = wg.morisawa_long_sample(blocks, status, 15, t0, f.model.T, lcap)
    d = Dev(f, blocks.shape[1], lcap)
    wg.morisawa_long_walk_dev(d.models.data_ptr(), B, 15, *d.solve_args()[3:], t0, lcap, d.out_ptrs(), d.length[1:].data_ptr(), T=f.model.T)
    d.check_blocks(blocks, status, refused=bad)
    d.check_outs(samples, refused=bad)
    # a walk that does not fit its rows: WG_MORISAWA_CAPACITY for that gait alone
    lens = samples["length"]
    short = int(np.median(lens[lens > 0]))
    s2 = wg.morisawa_long_sample(blocks, status, 15, t0, f.model.T, short)
    over = tuple(int(b) for b in np.nonzero(s2["length"] == wg.MORISAWA_CAPACITY)[0])
    assert over and len(over) < B - len(bad)
    e = Dev(f, blocks.shape[1], short)
    wg.morisawa_long_sample_dev(B, 15, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), t0, f.model.T, short, e.out_ptrs(), e.length[1:].data_ptr())
    e.check_outs(s2, refused=bad + over)


def test_a_short_block_is_refused_by_the_long_sampler():
    f = mf.Fleet(B, 14, 714)
    t0 = mf.t_start_of(f.model)
    short, st = wg.morisawa_solve(f.model, f.steps, f.n_steps, f.init_feet, f.com0, 14)
    words = wg.morisawa_long_block_bytes(14) // 8
    assert list(st) == [0] * B and short.shape[1] > words
    heads = to_dev(np.ascontiguousarray(short[:, :words]))                    # where long blocks of smax = 14 are expected
    d = Dev(f, 1, 40)
    wg.morisawa_long_sample_dev(B, 14, heads.data_ptr(), None, t0, f.model.T, 40, d.out_ptrs(), d.length[1:].data_ptr())
    nothing = {k: np.zeros((40,) + tuple(v.shape[1:])) for k, v in d.outs.items()}      # no gait is kept: only the shapes matter
    d.check_outs(dict(nothing, length=[wg.MORISAWA_BAD_INPUT] * B), refused=range(B))


def test_long_host_side_errors_launch_nothing():
    c = case(2, sampled=False)
    f = c["fleet"]
    d = Dev(f, c["words"], 8)
    lib, a = wg.lib(), d.solve_args(C.addressof(f.model))
    assert lib.wg_morisawa_long_solve_dev(*a[:2], 65, *a[3:], None) == -2
    assert lib.wg_morisawa_long_solve_dev(*a[:2], 1, *a[3:], None) == -2
    assert lib.wg_morisawa_long_solve_dev(None, *a[1:], None) == -2
    assert lib.wg_morisawa_long_solve_dev(*a[:8], None, None) == -2
    o = [d.out_ptrs()[k] for k in wg.MORISAWA_OUTPUTS]
    assert lib.wg_morisawa_long_sample_dev(f.B, 65, d.blocks[1:].data_ptr(), None, 0.0, 0.005, 8, *o, None, None) == -2
    assert lib.wg_morisawa_long_walk_dev(*a[:2], 65, *a[3:], 0.0, 8, *o, None, None) == -2
    for t0, T, lcap in ((-1.0, 0.005, 8), (0.0, 0.0, 8), (0.0, float("nan"), 8), (0.0, 0.005, 0)):
        assert lib.wg_morisawa_long_sample_dev(f.B, 2, d.blocks[1:].data_ptr(), None, t0, T, lcap, *o, None, None) == -2
    assert lib.wg_morisawa_long_solve_dev(a[0], 0, *a[2:], None) == 0
    d.check_blocks(np.zeros((f.B, 0)), [SENT_I] * f.B, refused=range(f.B))
