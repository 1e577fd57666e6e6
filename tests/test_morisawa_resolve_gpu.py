"""The Morisawa re-plan on the device (wg_morisawa_resolve_dev, _resolve_fleet_dev, their wg_morisawa_long_ forms and _ctx twins):
the bytes of the host twins (tests/test_morisawa_resolve_host.py), which are the bytes of the device's own full solve of the same
plans.  The factor block is made by wg_morisawa[_long]_solve_dev on the same stream and the re-plan follows it without a
synchronisation.  Short family at (smax, S) = (3, 2) and (14, 14) -- n = 64: every lane a row, the c % 64 owner of the back
substitution --, long family at (15, 15) -- n = 68, the first size past a row per lane -- and (64, 64), the LDS cap; B = 3 and 70.
Every comparison is equality of bytes; the sampled one is equality by value.  No tolerance."""
import functools

import numpy as np
import pytest

import morisawa_fleets as mf
import morisawa_replan as rp

wg = mf.wg()
pytestmark = pytest.mark.gpu

SENT_D, SENT_I = -7.25, -77
CASES = ((False, 3, 2), (False, 14, 14), (True, 15, 15), (True, 64, 64))


def to_dev(a):
    import torch
    if not isinstance(a, np.ndarray):
        a = np.frombuffer(bytes(memoryview(a).cast("B")), dtype=np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


@functools.lru_cache(maxsize=None)
def case(long_, smax, S, B):
    """the plans and what the host twins make of them: the full solve with one model and with a model per gait; never modified"""
    fam = rp.Family(long_)
    f = rp.plans(B, smax, S, 1500 + 10 * smax + B)
    one, st = fam.solve(f.model, f.steps, f.n_steps, f.init_feet, f.com0, smax)
    assert list(st) == [0] * B
    per, st = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, smax)
    assert list(st) == [0] * B and rp.swaps(fam.view(one[0], smax)) >= 1
    return dict(fam=fam, fleet=f, one=one, per=per, words=fam.words(smax))


class Dev:
    """the plans on the device; sentinel-filled blocks and statuses with a canary entry before and behind"""

    def __init__(self, f, words):
        import torch
        self.f, self.words = f, words
        self.steps, self.n_steps = to_dev(f.steps), to_dev(f.n_steps)
        self.feet, self.com0, self.models = to_dev(f.init_feet), to_dev(f.com0), to_dev(f.models)
        self.blocks = torch.full((f.B + 2, words), SENT_D, dtype=torch.float64, device="cuda")
        self.status = torch.full((f.B + 2,), SENT_I, dtype=torch.int32, device="cuda")

    def plan_args(self):
        return (self.steps.data_ptr(), self.feet.data_ptr(), self.com0.data_ptr(), self.blocks[1:].data_ptr(), self.status[1:].data_ptr())

    def solve_args(self, B=None):
        return (self.f.B if B is None else B, self.f.smax, self.steps.data_ptr(), self.n_steps.data_ptr(), self.feet.data_ptr(),
                self.com0.data_ptr(), self.blocks[1:].data_ptr(), self.status[1:].data_ptr())

    def check(self, blocks, refused=()):
        import torch
        torch.cuda.synchronize()
        got, st = self.blocks.cpu().numpy(), self.status.cpu().numpy()
        assert (got[0] == SENT_D).all() and (got[-1] == SENT_D).all() and st[0] == SENT_I and st[-1] == SENT_I
        for b in range(self.f.B):
            if b in refused:
                assert st[1 + b] == wg.MORISAWA_BAD_INPUT and (got[1 + b] == SENT_D).all(), b
            else:
                assert st[1 + b] == 0 and got[1 + b].tobytes() == blocks[b].tobytes(), b
        return got[1:-1]


@pytest.mark.parametrize("B", (3, 70))
@pytest.mark.parametrize("long_,smax,S", CASES)
def test_device_replan_is_host_twin_is_device_solve(long_, smax, S, B):
    import torch
    c = case(long_, smax, S, B)
    fam, f = c["fam"], c["fleet"]
    twin, st = fam.resolve(f.model, c["one"][0:1], None, f.steps, f.init_feet, f.com0, smax)
    assert list(st) == [0] * B and twin.tobytes() == c["one"].tobytes()
    full = Dev(f, c["words"])                       # the device's full solve of every plan
    fam.solve_dev(f.model, *full.solve_args())
    fac = Dev(f, c["words"])                        # gait 0's plan alone: the factor block, then the re-plan behind it on the stream
    d = Dev(f, c["words"])
    fam.solve_dev(f.model, *fac.solve_args(B=1))
    fam.resolve_dev(f.model, B, smax, fac.blocks[1:].data_ptr(), 1, None, *d.plan_args())
    got = d.check(twin)
    assert got.tobytes() == full.check(c["one"]).tobytes()
    assert torch.equal(fac.blocks[1].view(torch.int64), d.blocks[1].view(torch.int64)) and (fac.blocks[2:] == SENT_D).all()


@pytest.mark.parametrize("long_,smax,S", ((False, 14, 14), (True, 15, 15)))
def test_two_factors_and_the_fleet_form(long_, smax, S):
    """factor blocks at two CoM heights made by one wg_morisawa[_long]_solve_fleet_dev launch, gaits with a step height of their own
    re-planned from them under a mixed factor_of: each the full fleet solve at its factor's height"""
    B = 70
    c = case(long_, smax, S, B)
    fam = c["fam"]
    heights = (0.6, 0.8143)
    factor_of = np.array([(1, 1, 0, 0, 1)[b % 5] for b in range(B)], np.int32)
    f = rp.plans(B, smax, S, 1500 + 10 * smax + B)
    f.com0[:, 2] = [heights[k] for k in factor_of]
    assert len({m.step_height for m in f.models}) > 10
    want, st = fam.solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, smax)
    assert list(st) == [0] * B
    g = rp.plans(2, smax, S, 77)                     # two other plans at the two heights: the factor blocks
    g.com0[:, 2] = heights
    fac, d = Dev(g, c["words"]), Dev(f, c["words"])
    fam.solve_dev(fac.models.data_ptr(), *fac.solve_args())
    fo = to_dev(factor_of)
    fam.resolve_dev(d.models.data_ptr(), B, smax, fac.blocks[1:].data_ptr(), 2, fo.data_ptr(), *d.plan_args())
    d.check(want)
    twin, st = fam.resolve(f.models, fac.blocks[1:3].cpu().numpy(), factor_of, f.steps, f.init_feet, f.com0, smax)
    assert list(st) == [0] * B and twin.tobytes() == want.tobytes()


@pytest.mark.parametrize("long_,smax,S", ((False, 14, 14), (True, 15, 15)))
def test_refusals_inside_a_launch(long_, smax, S):
    """gait 1 of 3 has a NaN step, gait 2 a height that is not the factor's: status -1 and the caller's bytes; gait 0 is right"""
    c = case(long_, smax, S, 3)
    fam, src = c["fam"], c["fleet"]
    f = rp.plans(3, smax, S, 1500 + 10 * smax + 3)
    f.steps[1 * smax + S // 2].sy = float("nan")
    f.com0[2, 2] = rp.ulp_up(f.com0[2, 2])
    fac, d = Dev(src, c["words"]), Dev(f, c["words"])
    fam.solve_dev(src.model, *fac.solve_args(B=1))
    fam.resolve_dev(f.model, 3, smax, fac.blocks[1:].data_ptr(), 1, None, *d.plan_args())
    d.check(c["one"], refused=(1, 2))
    # factor_of out of range on both sides, in the same way
    e = Dev(src, c["words"])
    fo = to_dev(np.array([-1, 0, 1], np.int32))
    fam.resolve_dev(src.model, 3, smax, fac.blocks[1:].data_ptr(), 1, fo.data_ptr(), *e.plan_args())
    e.check(c["one"], refused=(0, 2))


@pytest.mark.parametrize("long_", (False, True))
def test_replan_then_sample_is_the_walk(long_):
    """smax = 3: wg_morisawa[_long]_resolve_dev, then _sample_dev on the same stream; every output equals by value
    wg_morisawa[_long]_walk_dev of the same plans"""
    import torch
    B, smax, S = 70, 3, 3
    c = case(long_, smax, S, B)
    fam, f = c["fam"], c["fleet"]
    t0 = mf.t_start_of(f.model)
    lcap = fam.length(f.model, S, t0) + 3
    shape = dict(zmp_x=(B,), zmp_y=(B,), com=(4, B), left=(6, B), right=(6, B), left_type=(B,), right_type=(B,))
    outs = [{k: torch.full((lcap,) + shape[k], SENT_I if k.endswith("type") else SENT_D,
                           dtype=torch.int32 if k.endswith("type") else torch.float64, device="cuda") for k in wg.MORISAWA_OUTPUTS}
            for _ in range(2)]
    length = torch.full((2, B), SENT_I, dtype=torch.int32, device="cuda")
    w = Dev(f, c["words"])
    fam.walk_dev(f.model, *w.solve_args(), t0, lcap, {k: v.data_ptr() for k, v in outs[0].items()}, length[0].data_ptr())
    fac, d = Dev(f, c["words"]), Dev(f, c["words"])
    fam.solve_dev(f.model, *fac.solve_args(B=1))
    fam.resolve_dev(f.model, B, smax, fac.blocks[1:].data_ptr(), 1, None, *d.plan_args())
    fam.sample_dev(B, smax, d.blocks[1:].data_ptr(), d.status[1:].data_ptr(), t0, f.model.T, lcap, {k: v.data_ptr() for k, v in outs[1].items()},
                   length[1].data_ptr())
    d.check(c["one"])
    assert torch.equal(length[0], length[1]) and (length[0] > 100).all()
    for k in wg.MORISAWA_OUTPUTS:
        a, b_ = outs[0][k].cpu().numpy(), outs[1][k].cpu().numpy()
        assert np.array_equal(a, b_) and not (a == (SENT_I if k.endswith("type") else SENT_D)).any(), k


@pytest.mark.parametrize("long_,smax,S", ((False, 3, 2), (True, 15, 15)))
def test_context_forms_give_the_same_bytes(long_, smax, S):
    import torch
    B = 3
    c = case(long_, smax, S, B)
    fam, f = c["fam"], c["fleet"]
    st = torch.cuda.Stream()
    fac, one, per = Dev(f, c["words"]), Dev(f, c["words"]), Dev(f, c["words"])
    torch.cuda.synchronize()
    with wg.Context(0) as ctx:
        fam.solve_dev(f.model, *fac.solve_args(B=1), stream=st.cuda_stream, ctx=ctx)
        fam.resolve_dev(f.model, B, smax, fac.blocks[1:].data_ptr(), 1, None, *one.plan_args(), stream=st.cuda_stream, ctx=ctx)
        fam.resolve_dev(per.models.data_ptr(), B, smax, fac.blocks[1:].data_ptr(), 1, None, *per.plan_args(), stream=st.cuda_stream, ctx=ctx)
        st.synchronize()
        one.check(c["one"])
        per.check(c["per"])


def test_host_side_errors_launch_nothing():
    import ctypes as C
    c = case(False, 3, 2, 3)
    f = c["fleet"]
    lib = wg.lib()
    for name, cap in (("wg_morisawa_", wg.MORISAWA_MAX_STEPS), ("wg_morisawa_long_", wg.MORISAWA_LONG_MAX_STEPS)):
        d, fac = Dev(f, c["words"]), Dev(f, c["words"])
        for form, model in (("resolve_dev", C.addressof(f.model)), ("resolve_fleet_dev", d.models.data_ptr())):
            fn = getattr(lib, name + form)
            args = [model, 3, 3, fac.blocks.data_ptr(), 1, None, *d.plan_args(), None]
            for i in (0, 3, 6, 7, 8, 9, 10):
                assert fn(*[None if k == i else a for k, a in enumerate(args)]) == -2, (form, i)
            for i, bad in ((1, -1), (2, 1), (2, cap + 1), (4, 0)):
                assert fn(*[bad if k == i else a for k, a in enumerate(args)]) == -2, (form, i, bad)
            assert fn(*[0 if k == 1 else a for k, a in enumerate(args)]) == 0
        import torch
        torch.cuda.synchronize()
        assert (d.blocks == SENT_D).all() and (d.status == SENT_I).all()
