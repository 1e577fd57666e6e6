"""The producers' fleet forms in their chains, on one stream, nothing leaving the device in between:

  Dimitrov   wg_steps_plan_fleet_dev -> wg_zmpdisc_begin / append / end_fleet_dev -> wg_foot_constraints_append_fleet_dev ->
             wg_dimitrov_follow_fleet_dev on blocks of wg_dimitrov_constants_batch_dev: 8 gaits of 3 robot types, every gait's final
             state and queue equal to the same chain run per robot type through the one-model entry points;
  Kajita     wg_zmpdisc_full_fleet_dev -> wg_riccati_gains_batch_dev -> wg_preview_run_fleet_dev on the queue of the mixed fleet
             (tests/test_zmpdisc_fleet_gpu.py): CoM equal to wgo_zmpdisc -> wgo_preview_run with the gait's own model and gains."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stepsplan as sp  # noqa: E402
from stepsplan import ADD, LS, SF  # noqa: E402
from test_preview_fleet_gpu import gains_of  # noqa: E402
from test_preview_oracle import oracle_run  # noqa: E402
from test_zmpdisc_fleet_gpu import DevFleet, copy_model, mixed_case, models_dev, to_dev  # noqa: E402
from test_zmpdisc_gpu import kajita_model  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu

PSZ, SSZ = C.sizeof(wg.ZmpPolytope), C.sizeof(wg.DimitrovState)
SCALES = (0.8, 1.0, 1.2)                          # three robot types: everything of a robot scales with its size
B8, SMAX, CCAP, QCAP, TICKS = 8, 8, 8, 32, 64    # 64 ticks: past the rest phase, into the steps
TYPE_OF = np.array([g % 3 for g in range(B8)], np.int32)


def robot(r):
    """(zmpdisc model, sole, CoM height) of type r; the single support is a multiple of T that grows with the robot"""
    s = SCALES[r]
    m = copy_model(kajita_model(), t_single=(0.6, 0.7, 0.8)[r], t_double=(0.1, 0.13, 0.15)[r], step_height=0.07 * s, omega=2.0,
                   foot_b=0.1 * s, foot_h=0.105 * s, foot_f=0.13 * s)
    return m, (0.24 * s, 0.138 * s, 0.02 * s, 0.02 * s), 0.814 * s


def commands(g):
    """gait g's walk as two lists: what the begin call takes (the support foot and a first step), and the rest"""
    s = SCALES[TYPE_OF[g]]
    n_add = 3 + 2 * (g % 2)                            # odd: the last support foot closes the alternation
    adds = [(ADD, 0, (0.1 + 0.01 * g) * s, (-0.19 if i % 2 == 0 else 0.19) * s, 0.0) for i in range(n_add)]
    return [(SF, 1, 0.0, 0.0, 0.0), adds[0]], adds[1:] + [(LS, 0, 0.0, 0.0, 0.0)]


class Chain:
    """the device arrays of one run of the chain over the gaits `idx`"""

    def __init__(self, idx, lcap):
        import torch
        self.t, self.idx, self.B, self.lcap = torch, idx, len(idx), lcap
        B = self.B
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda")  # noqa: E731
        self.steps = z(B * SMAX * sp.STEP_BYTES, dt=torch.uint8)
        self.n_steps, self.length, self.done, self.count = (z(B, dt=torch.int32) for _ in range(4))
        self.stack = to_dev(np.tile(np.array([1, 0, 0, 0], np.int32), (B, 1)))
        self.walk = z(B * wg.ZMPDISC_STATE_BYTES, dt=torch.uint8)
        self.feet = to_dev(np.tile([0.0, 0.095, 0.0, 0.0, -0.095, 0.0], (B, 1)) * np.array([SCALES[TYPE_OF[g]] for g in idx])[:, None])
        self.outs = dict(left=z(lcap, 6, B), left_type=z(lcap, B, dt=torch.int32), right=z(lcap, 6, B))
        self.time = to_dev(np.arange(lcap) * 0.005)
        self.queues = torch.full((B, QCAP, PSZ), 0xA5, dtype=torch.uint8, device="cuda")
        self.ts, self.te = torch.full((B, QCAP), -1.0, dtype=torch.float64, device="cuda"), torch.full((B, QCAP), -1.0, dtype=torch.float64, device="cuda")
        st = (wg.DimitrovState * B)()
        for b in range(B):
            st[b].starting = 1
        self.states, self.clock, self.ticks, self.ran = to_dev(st), z(B), z(B, dt=torch.int32), z(B, dt=torch.int32)
        self.cmds = []
        for part in (0, 1):
            raw, n = sp.cmd_bytes([commands(g)[part] for g in idx], CCAP)
            self.cmds.append((to_dev(raw), to_dev(n)))

    def out_ptrs(self):
        return {k: v.data_ptr() for k, v in self.outs.items()}

    def result(self):
        self.t.cuda.synchronize()
        h = lambda x: x.cpu().numpy()  # noqa: E731
        return dict(states=h(self.states).reshape(self.B, SSZ), queues=h(self.queues), ts=h(self.ts), te=h(self.te), count=h(self.count),
                    length=h(self.length), ticks=h(self.ticks), clock=h(self.clock), n_given=h(self.stack)[:, 2], ran=h(self.ran),
                    left=h(self.outs["left"]))


def chain_lcap():
    """rows for the longest walk: every gait's own model and step count (the times are the models')"""
    L = 0
    for g in range(B8):
        m = robot(TYPE_OF[g])[0]
        first, rest = commands(g)
        n = len(first) + len(rest)
        steps = wg.rel_steps([[0.0, 0.1, 0.0]] * n, m.t_single, m.t_double)
        L = max(L, wg.zmpdisc_length(m, steps))
    return L


def run_fleet_chain(lcap):
    wg.init(0)
    c = Chain(list(range(B8)), lcap)
    robots = [robot(r) for r in range(3)]
    B = B8
    ss = to_dev(np.array([robots[r][0].t_single for r in TYPE_OF])); ds = to_dev(np.array([robots[r][0].t_double for r in TYPE_OF]))
    soles = to_dev(np.array([robots[r][1] for r in TYPE_OF]))
    d_models, d_of = models_dev([m for m, _, _ in robots]), to_dev(TYPE_OF)
    zfl = wg.zmpdisc_fleet(kajita_model(), 3, d_models.data_ptr(), d_of.data_ptr())
    base = wg.dimitrov_defaults()
    heights = to_dev(np.array([h for _, _, h in robots]))
    blocks = c.t.zeros((3, wg.dimitrov_constants_bytes()), dtype=c.t.uint8, device="cuda")
    status = c.t.full((3,), -7, dtype=c.t.int32, device="cuda")
    wg.dimitrov_constants_batch_dev(3, base, heights.data_ptr(), None, None, blocks.data_ptr(), status.data_ptr())
    dfl = wg.dimitrov_fleet(base, 3, blocks.data_ptr(), d_of.data_ptr())

    def grow_and_follow():
        wg.foot_constraints_append_fleet_dev(B, lcap, 0, c.done.data_ptr(), c.length.data_ptr(), c.time.data_ptr(), c.outs["left"].data_ptr(),
                                             c.outs["left_type"].data_ptr(), c.outs["right"].data_ptr(), soles.data_ptr(), QCAP,
                                             c.queues.data_ptr(), c.ts.data_ptr(), c.te.data_ptr(), c.count.data_ptr())
        wg.dimitrov_follow_fleet_dev(B, dfl, QCAP, c.queues.data_ptr(), c.ts.data_ptr(), c.te.data_ptr(), c.count.data_ptr(), lcap,
                                     c.time.data_ptr(), c.done.data_ptr(), c.walk.data_ptr(), 0, c.clock.data_ptr(), c.ticks.data_ptr(),
                                     TICKS, TICKS, c.states.data_ptr(), None, c.ran.data_ptr(), 0)
    plan = lambda part: wg.steps_plan_fleet_dev(B, CCAP, c.cmds[part][0].data_ptr(), c.cmds[part][1].data_ptr(), ss.data_ptr(),  # noqa: E731
                                                ds.data_ptr(), c.stack.data_ptr(), SMAX, c.steps.data_ptr(), c.n_steps.data_ptr())
    plan(0)
    wg.zmpdisc_begin_fleet_dev(zfl, B, SMAX, c.steps.data_ptr(), c.n_steps.data_ptr(), c.feet.data_ptr(), lcap, c.out_ptrs(),
                               c.walk.data_ptr(), c.length.data_ptr())
    grow_and_follow()
    plan(1)
    wg.zmpdisc_append_fleet_dev(zfl, B, SMAX, c.steps.data_ptr(), c.n_steps.data_ptr(), lcap, c.out_ptrs(), c.walk.data_ptr(),
                                c.length.data_ptr())
    grow_and_follow()
    wg.zmpdisc_end_fleet_dev(zfl, B, lcap, c.out_ptrs(), c.walk.data_ptr(), c.length.data_ptr())
    grow_and_follow()
    r = c.result()
    assert (status.cpu().numpy() == 0).all()
    return r


def run_type_chain(r, lcap):
    """the same chain for the gaits of robot type r alone, through the one-model entry points and a context configured for it"""
    idx = [g for g in range(B8) if TYPE_OF[g] == r]
    c = Chain(idx, lcap)
    B = c.B
    m, sole, height = robot(r)
    dm = wg.dimitrov_defaults()
    dm.com_height = height
    wg.dimitrov_configure(dm)

    def grow_and_follow():
        wg.foot_constraints_append_dev(B, lcap, 0, c.done.data_ptr(), c.length.data_ptr(), c.time.data_ptr(), c.outs["left"].data_ptr(),
                                       c.outs["left_type"].data_ptr(), c.outs["right"].data_ptr(), *sole, QCAP, c.queues.data_ptr(),
                                       c.ts.data_ptr(), c.te.data_ptr(), c.count.data_ptr())
        wg.dimitrov_follow_dev(B, QCAP, c.queues.data_ptr(), c.ts.data_ptr(), c.te.data_ptr(), c.count.data_ptr(), lcap, c.time.data_ptr(),
                               c.done.data_ptr(), c.walk.data_ptr(), 0, c.clock.data_ptr(), c.ticks.data_ptr(), TICKS, TICKS,
                               c.states.data_ptr(), None, c.ran.data_ptr(), 0)
    plan = lambda part: wg.steps_plan_dev(B, CCAP, c.cmds[part][0].data_ptr(), c.cmds[part][1].data_ptr(), m.t_single, m.t_double,  # noqa: E731
                                          c.stack.data_ptr(), SMAX, c.steps.data_ptr(), c.n_steps.data_ptr())
    plan(0)
    wg.zmpdisc_begin_dev(m, B, SMAX, c.steps.data_ptr(), c.n_steps.data_ptr(), c.feet.data_ptr(), lcap, c.out_ptrs(), c.walk.data_ptr(),
                         c.length.data_ptr())
    grow_and_follow()
    plan(1)
    wg.zmpdisc_append_dev(m, B, SMAX, c.steps.data_ptr(), c.n_steps.data_ptr(), lcap, c.out_ptrs(), c.walk.data_ptr(), c.length.data_ptr())
    grow_and_follow()
    wg.zmpdisc_end_dev(m, B, lcap, c.out_ptrs(), c.walk.data_ptr(), c.length.data_ptr())
    grow_and_follow()
    return idx, c.result()


def test_dimitrov_chain_of_three_robot_types_equals_the_chain_per_type():
    lcap = chain_lcap()
    fleet = run_fleet_chain(lcap)
    assert (fleet["length"] > 0).all() and (fleet["count"] > 4).all() and (fleet["ticks"] == TICKS).all()
    assert len({fleet["states"][g].tobytes() for g in range(B8)}) == B8
    for r in range(3):
        idx, one = run_type_chain(r, lcap)
        for k in ("length", "count", "ticks", "clock", "n_given", "ran", "states", "queues", "ts", "te"):
            assert np.array_equal(fleet[k][idx], one[k]), (r, k)
        assert np.array_equal(fleet["left"][:, :, idx], one["left"]), r


def test_kajita_chain_on_the_mixed_fleet_equals_the_oracle_chain():
    import torch
    wg.init(0)
    c = mixed_case()
    B, smax, lcap, nl, T = 6, c["smax"], c["lcap"], 160, 0.005
    steps = (wg.RelStep * (B * smax))(*[c["steps"][i] for i in range(B * smax)])
    d = DevFleet(kajita_model(), c["models"], c["model_of"][:B], steps, c["n_steps"][:B], c["init"][:B])
    zc = np.array([0.6, 0.7, 0.814, 0.9, 0.65, 0.95])
    zx = torch.full((lcap, B), -7.25, dtype=torch.float64, device="cuda"); zy = torch.full_like(zx, -7.25)
    ln = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_zc = to_dev(zc)
    K = torch.zeros(4, B, dtype=torch.float64, device="cuda"); F = torch.zeros(nl, B, dtype=torch.float64, device="cuda")
    status = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    Lrun = lcap - nl + 1
    st = torch.zeros(B, 8, dtype=torch.float64, device="cuda")
    com = torch.zeros(Lrun, 6, B, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    wg.zmpdisc_full_fleet_dev(d.fleet, B, smax, d.steps.data_ptr(), d.n_steps.data_ptr(), d.init.data_ptr(), lcap,
                              dict(zmp_x=zx.data_ptr(), zmp_y=zy.data_ptr()), ln.data_ptr(), stream)
    wg.riccati_gains_batch_dev(B, T, d_zc.data_ptr(), 1.0, 1e-6, nl, wg.RICCATI_WITHOUT_INITIALPOS, K.data_ptr(), F.data_ptr(),
                               status.data_ptr(), stream)
    pf = wg.preview_fleet(T, nl, d_zc.data_ptr(), K.data_ptr(), F.data_ptr())
    wg.preview_run_fleet_dev(B, Lrun, pf, zx.data_ptr(), zy.data_ptr(), st.data_ptr(), com.data_ptr(), None, True, stream)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all() and np.array_equal(ln.cpu().numpy(), c["lens"][:B])
    com_h = com.cpu().numpy()
    for b in range(B):
        o = c["orc"][b]                                # wgo_zmpdisc with the gait's own model
        L = o["length"]
        ZX = np.full((1, lcap), o["zmp"][-1, 0]); ZY = np.full((1, lcap), o["zmp"][-1, 1])      # at rest after its last sample
        ZX[0, :L], ZY[0, :L] = o["zmp"][:, 0], o["zmp"][:, 1]
        g, Fh = gains_of(zc[b], nl)
        com_o, _ = oracle_run(g, Fh, ZX, ZY, np.zeros((1, 8)), Lrun)
        assert np.array_equal(com_h[:, :, b], com_o[0]), b
