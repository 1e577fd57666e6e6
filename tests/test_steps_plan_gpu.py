"""The step stack on the device (wg_steps_plan_dev): rows, counts and stacks byte for byte against the host twin and the oracle's
generators (tests/stepsplan.py), canaries around every array; the capacity edge, refusals and their stickiness; cutting a command
list into calls; and the chains plan -> wg_zmpdisc_full_batch_dev and plan -> begin -> (plan -> append) x 3 -> end on one stream
with no host synchronisation in between, held to the oracle's ZMP discretisation over the oracle's steps."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oraclelib as ol  # noqa: E402
import stepsplan as sp  # noqa: E402
from stepsplan import ADD, ARC, BAD, CAPACITY, LS, ONLINE, SF, wg  # noqa: E402
from test_zmpdisc_oracle import GOLD, golden_case, kajita_model  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = 0xA5
OUTS = wg.ZMPDISC_OUTPUTS
ZD_BAD = -1                                  # WG_ZMPDISC_BAD_INPUT


class DevStack:
    """B gaits' rows, counts and stacks on the device, one guard gait either side of every array"""

    def __init__(self, B, smax, keep):
        import torch
        self.t = torch
        wg.init(0)
        self.B, self.smax = B, smax
        self.steps = torch.full((B + 2, smax, sp.STEP_BYTES), CANARY, dtype=torch.uint8, device="cuda")
        self.n = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
        st = np.full((B + 2, 4), -7, np.int32)
        st[1:B + 1] = 0
        st[1:B + 1, 0] = keep
        self.stack = torch.from_numpy(st).cuda()
        self.keepalive = []

    def plan(self, lists, ccap, n_cmds=None, smax=None, steps_ptr=None, ss=sp.SS, ds=sp.DS):
        """one wg_steps_plan_dev over the gaits' lists; no synchronisation"""
        raw, n = sp.cmd_bytes(lists, ccap)
        n = n if n_cmds is None else np.asarray(n_cmds, np.int32)
        guard = np.full((1, ccap, sp.CMD_BYTES), CANARY, np.uint8)
        d_cmds = self.t.from_numpy(np.concatenate([guard, raw, guard])).cuda()
        d_n = self.t.from_numpy(np.concatenate([[-7], n, [-7]]).astype(np.int32)).cuda()
        self.keepalive.append((d_cmds, d_n))
        wg.steps_plan_dev(self.B, ccap, d_cmds[1:].data_ptr(), d_n[1:].data_ptr(), ss, ds, self.stack[1:].data_ptr(),
                          smax or self.smax, steps_ptr or self.steps[1:].data_ptr(), self.n[1:].data_ptr())

    def read(self):
        """(rows [B, smax, STEP_BYTES], n_steps [B], stack [B, 4]) after checking the guards"""
        rows, n, st = self.steps.cpu().numpy(), self.n.cpu().numpy(), self.stack.cpu().numpy()
        assert (rows[0] == CANARY).all() and (rows[-1] == CANARY).all()
        assert n[0] == n[-1] == -7 and (st[0] == -7).all() and (st[-1] == -7).all()
        return rows[1:-1].copy(), n[1:-1].copy(), st[1:-1].copy()


@pytest.mark.parametrize("smax", [1, 7, 64])
@pytest.mark.parametrize("B", [1, 63, 65, 70])
def test_rows_counts_and_stacks_equal_host_and_oracle(B, smax):
    fam = sp.family(100 * smax + 7, 70, 8, smax)[:B]
    if B > 1:
        fam = fam[:-1] + [(sp.CIRCLE, *sp.oracle_list(sp.CIRCLE, 1)[:1], 1, 1)] if smax >= 5 else fam
    keep0 = np.array([f[2] for f in fam], np.int32)
    d = DevStack(B, smax, keep0)
    d.plan([f[0] for f in fam], 8)
    rows, n, st = d.read()
    for b, (cmds, want, k0, k1) in enumerate(fam):
        assert n[b] == len(want) and np.array_equal(rows[b, :n[b]], want), b          # the oracle
        assert (rows[b, n[b]:] == CANARY).all(), b                                     # the row past n_steps
        assert st[b].tolist() == [k1, 0, len(want), 0], b
        buf, hn, hs = sp.host_plan(cmds, k0, smax)                                     # the host twin
        assert hn == n[b] and np.array_equal(buf[1:-1], rows[b]) and [hs.keep, hs.error, hs.n_given, hs.pad_] == st[b].tolist()
    assert n.max() > 0


EDGE = {1: (ARC, 1, 0.0, 0.75, 5.0), 7: (ARC, -1, 0.0, -0.75, 75.0), 64: (ARC, 1, -3.0, 0.0, 182.0)}
OVER = {1: (ARC, 1, 0.0, 0.75, 15.0), 7: (ARC, -1, 0.0, -0.75, 85.0), 64: (ARC, 1, -3.0, 0.0, 185.0)}


@pytest.mark.parametrize("smax", [1, 7, 64])
def test_capacity_edge_refusals_and_their_neighbours(smax):
    """an arc of exactly smax steps passes, one of smax + 1 is refused: sticky, its row untouched, and the neighbours' bytes are
    those of a run without that gait's commands.  The other refusals ride along."""
    B = 65
    assert len(sp.oracle_list([EDGE[smax]])[0]) == smax and len(sp.oracle_list([OVER[smax]])[0]) == smax + 1
    fam = sp.family(100 * smax + 7, 70, 8, smax)[:B]
    lists = [f[0] for f in fam]
    lists[5], lists[6] = [EDGE[smax]], [OVER[smax]]
    bad = {6: CAPACITY, 9: BAD, 20: BAD, 33: BAD, 40: BAD, 41: BAD, 63: BAD, 64: CAPACITY}
    lists[9] = [(ADD, 0, 0.1, 0.2, 0.0), (7, 1, 0.0, 0.0, 0.0)][-min(smax, 2):]      # unknown op
    lists[20] = [(SF, 0, 0.0, 0.0, 0.0)]                                               # foot not +-1
    lists[33] = [(ONLINE, 0, 0.0, float("nan"), 0.0)]                                  # non-finite
    lists[40] = [(ARC, 1, 0.0, 0.75, -30.0)]                                           # negative arc
    lists[41] = [(ADD, 0, 0.1, 0.2, 0.0)]                                              # n_cmds out of range, below
    lists[63] = [(ADD, 0, 0.1, 0.2, 0.0)]
    lists[64] = [(ADD, 0, 0.1, 0.2, 0.0)] * min(smax + 1, 8) if smax < 8 else [(ARC, 1, 1e150, 0.0, 1e150)]
    n_cmds = np.array([len(c) for c in lists], np.int32)
    n_cmds[41], n_cmds[63] = 9, -1
    keep0 = np.array([f[2] for f in fam], np.int32)
    d = DevStack(B, smax, keep0)
    d.plan(lists, 8, n_cmds)
    rows, n, st = d.read()
    assert n[5] == smax and st[5, 1] == 0
    for b, code in bad.items():
        assert n[b] == 0 and (rows[b] == CANARY).all() and st[b].tolist() == [keep0[b], code, 0, 0], b
    calm = DevStack(B, smax, keep0)                                                    # the same fleet with those gaits idle
    idle = n_cmds.copy()
    idle[list(bad)] = 0
    calm.plan(lists, 8, idle)
    rows2, n2, st2 = calm.read()
    ok = np.array([b not in bad for b in range(B)])
    assert np.array_equal(rows[ok], rows2[ok]) and np.array_equal(n[ok], n2[ok]) and np.array_equal(st[ok], st2[ok])
    for b in bad:                                                                      # idle: nothing but n_steps = 0
        assert n2[b] == 0 and (rows2[b] == CANARY).all() and st2[b].tolist() == [keep0[b], 0, 0, 0]
    d.plan([[(ADD, 0, 0.1, 0.2, 0.0)]] * B, 8)                                        # sticky: a good call later is refused too
    rows3, n3, st3 = d.read()
    for b, code in bad.items():
        assert n3[b] == 0 and (rows3[b] == CANARY).all() and st3[b].tolist() == [keep0[b], code, 0, 0], b
    assert (n3[ok] == 1).all() and (st3[ok, 2] == st[ok, 2] + 1).all()


def test_cutting_a_command_list_into_calls():
    """one call, one command per call, uneven cuts: the same concatenated steps and the same final stack; a gait with no command
    in a call is untouched by it"""
    B, smax = 70, 64
    fam = sp.family(6407, 70, 8, smax)
    keep0 = np.array([f[2] for f in fam], np.int32)
    rng = np.random.default_rng(3)
    uneven = []
    for f in fam:
        cuts, left = [], len(f[0])
        while left:
            cuts.append(int(rng.integers(0, left + 1)))
            left -= cuts[-1]
        uneven.append(cuts)
    for cuts in ([[len(f[0])] for f in fam], [[1] * len(f[0]) for f in fam], uneven):
        d = DevStack(B, smax, keep0)
        got = [[] for _ in range(B)]
        at = [0] * B
        for call in range(max(len(c) for c in cuts)):
            k = [c[call] if call < len(c) else 0 for c in cuts]
            before = d.read()
            d.steps.fill_(CANARY)
            d.plan([fam[b][0][at[b]:at[b] + k[b]] for b in range(B)], 8)
            rows, n, st = d.read()
            for b in range(B):
                at[b] += k[b]
                got[b].append(rows[b, :n[b]])
                assert (rows[b, n[b]:] == CANARY).all()
                if k[b] == 0:
                    assert n[b] == 0 and np.array_equal(st[b], before[2][b]), b
        for b, (cmds, want, k0, k1) in enumerate(fam):
            assert np.array_equal(np.concatenate(got[b]), want) and st[b].tolist() == [k1, 0, len(want), 0], b


# ---- the chains: steps planned on the device walk straight into the ZMP discretisation ----
def chain_fleet():
    """70 gaits: gait 0 turns on TestKajita2003's circle, the others on arcs of their own; then three rounds of on-line steps, 0..3
    per gait and round"""
    rng = np.random.default_rng(70)
    B = 70
    first, rounds = [], [[], [], []]
    for b in range(B):
        if b == 0:
            arc = sp.CIRCLE[1]
        else:
            while True:
                arc = sp.random_arc(rng, 9)
                if 1 <= len(sp.oracle_list([arc])[0]):
                    break
        first.append([(SF, -arc[1], 0.0, 0.0, 0.0), arc])
        for r in rounds:
            k = int(rng.integers(0, 4)) if b else 1
            r.append([(ONLINE, 0, float(rng.uniform(0.0, 0.2)), 0.0, float(rng.uniform(-5, 5))) for _ in range(k)])
    _, _, init = golden_case("Circle")
    return first, rounds, np.tile(np.asarray(init, np.float64), (B, 1))


def oracle_walk(m, cmds, init):
    rows, _ = sp.oracle_list(cmds, 1, m.t_single, m.t_double)
    steps = (wg.RelStep * len(rows)).from_buffer_copy(rows.tobytes())
    return ol.zmpdisc(m, steps, init, lib=sp.ptrig()), len(rows)


def out_buffers(t, B, lcap):
    shape = {"left": (lcap, 6, B), "right": (lcap, 6, B)}
    r = {k: t.zeros(*shape.get(k, (lcap, B)), dtype=t.int32 if k.endswith("type") else t.float64, device="cuda") for k in OUTS}
    r["length"] = t.full((B,), -9, dtype=t.int32, device="cuda")
    return r


def assert_walk(h, b, o):
    L = o["length"]
    assert h["length"][b] == L, b
    assert np.array_equal(h["zmp_x"][:L, b], o["zmp"][:, 0]) and np.array_equal(h["zmp_y"][:L, b], o["zmp"][:, 1]), b
    assert np.array_equal(h["zmp_theta"][:L, b], o["zmp_theta"]) and np.array_equal(h["zmp_type"][:L, b], o["zmp_type"]), b
    for k in ("left", "right"):
        assert np.array_equal(h[k][:L, :, b], o[k]) and np.array_equal(h[k + "_type"][:L, b], o[k + "_type"]), (b, k)


_chain = {}


def online_chain(spoil=None):
    """plan -> begin, 3 x (plan -> append), end, nothing but launches in between; `spoil`: a gait whose first list is refused"""
    if spoil in _chain:
        return _chain[spoil]
    import torch
    m = kajita_model()
    first, rounds, init = chain_fleet()
    B, smax, K = len(first), 16, 3
    whole = [first[b] + [c for r in rounds for c in r[b]] for b in range(B)]
    want = [oracle_walk(m, whole[b], init[b]) for b in range(B)]
    lcap = max(o["length"] for o, _ in want) + 2
    if spoil is not None:
        first = [list(f) for f in first]
        first[spoil] = [first[spoil][0], (ARC, 2, 0.0, 0.75, 30.0)]
    d = DevStack(B, smax, 1)
    buf = out_buffers(torch, B, lcap)
    outs = {k: buf[k].data_ptr() for k in OUTS}
    state = torch.zeros(B * wg.ZMPDISC_STATE_BYTES, dtype=torch.uint8, device="cuda")
    d_init = torch.from_numpy(init).cuda()
    chunk = torch.full((B, K, sp.STEP_BYTES), CANARY, dtype=torch.uint8, device="cuda")
    d.plan(first, 2, ss=m.t_single, ds=m.t_double)
    wg.zmpdisc_begin_dev(m, B, smax, d.steps[1:].data_ptr(), d.n[1:].data_ptr(), d_init.data_ptr(), lcap, outs, state.data_ptr(),
                         buf["length"].data_ptr())
    lens = []
    for r in rounds:
        d.plan(r, K, smax=K, steps_ptr=chunk.data_ptr(), ss=m.t_single, ds=m.t_double)
        wg.zmpdisc_append_dev(m, B, K, chunk.data_ptr(), d.n[1:].data_ptr(), lcap, outs, state.data_ptr(), buf["length"].data_ptr())
        lens.append(buf["length"].clone())                       # a device copy on the same stream: no synchronisation
    wg.zmpdisc_end_dev(m, B, lcap, outs, state.data_ptr(), buf["length"].data_ptr())
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in buf.items()}
    _chain[spoil] = (h, want, d.read(), [x.cpu().numpy() for x in lens], whole)
    return _chain[spoil]


def test_plan_then_full_batch_on_one_stream():
    import torch
    m = kajita_model()
    first, _, init = chain_fleet()
    B, smax = len(first), 16
    lists = [f + [sp.CIRCLE[2]] for f in first]                  # support foot, arc, last support
    assert lists[0] == sp.CIRCLE
    want = [oracle_walk(m, lists[b], init[b]) for b in range(B)]
    assert len({n for _, n in want}) > 4                         # ragged
    lcap = max(o["length"] for o, _ in want) + 2
    d = DevStack(B, smax, 1)
    buf = out_buffers(torch, B, lcap)
    d_init = torch.from_numpy(init).cuda()
    d.plan(lists, 3, ss=m.t_single, ds=m.t_double)
    rc = wg.lib().wg_zmpdisc_full_batch_dev(C.byref(m), B, smax, d.steps[1:].data_ptr(), d.n[1:].data_ptr(), d_init.data_ptr(), lcap,
                                            *[buf[k].data_ptr() for k in OUTS], buf["length"].data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in buf.items()}
    _, n, _ = d.read()
    for b in range(B):
        assert n[b] == want[b][1]
        assert_walk(h, b, want[b][0])
    # gait 0 is TurningOnTheCircle: the reference's golden file, to its print precision (as tests/test_zmpdisc_gpu.py pins it)
    rows = GOLD["Circle_rows"]
    k = rows.shape[0]
    assert h["length"][0] == k + 2 * int(m.preview_time / m.T)
    assert np.abs(rows[:, 13] - h["zmp_x"][:k, 0]).max() < 2e-7 and np.abs(rows[:, 14] - h["zmp_y"][:k, 0]).max() < 2e-7
    for c0, key in ((1, "left"), (7, "right")):
        assert np.abs(rows[:, c0:c0 + 6] - h[key][:k, :, 0]).max() < 2e-7


def test_plan_begin_three_appends_end_on_one_stream():
    h, want, (rows, n, st), lens, whole = online_chain()
    m = kajita_model()
    given = np.array([w for _, w in want])
    assert np.array_equal(st[:, 2], given) and (st[:, 1] == 0).all() and len(set(given.tolist())) > 6
    for b, (o, _) in enumerate(want):
        assert_walk(h, b, o)
    # the lengths each append left on the device are the prefix sums over the steps given so far
    first, rounds, _ = chain_fleet()
    for b in (0, 1, 17, 69):
        have = len(sp.oracle_list(first[b], 1)[0])
        steps = (wg.RelStep * int(given[b])).from_buffer_copy(sp.oracle_list(whole[b], 1, m.t_single, m.t_double)[0].tobytes())
        for r, ln in zip(rounds, lens):
            have += len(r[b])
            assert ln[b] == wg.zmpdisc_length_after(m, steps, have)


def test_a_refused_plan_in_the_chain():
    """gait 11's first list is refused: begin gives it its own WG_ZMPDISC_BAD_INPUT, the appends let it sit out, and the other 69
    are bit-equal to the clean chain"""
    clean = online_chain()[0]
    h, want, (rows, n, st), lens, _ = online_chain(spoil=11)
    assert st[11].tolist() == [1, BAD, 0, 0] and h["length"][11] == ZD_BAD
    assert all(ln[11] == ZD_BAD for ln in lens)
    others = [b for b in range(len(want)) if b != 11]
    for k in OUTS + ("length",):
        assert np.array_equal(h[k][..., others], clean[k][..., others]), k
        if k != "length":
            assert not h[k][..., 11].any(), k                     # nothing of the refused gait was written
    assert (st[others, 1] == 0).all()


def test_empty_batches_and_bad_arguments():
    wg.init(0)
    lib = wg.lib()
    one = C.c_void_p(8)                                            # never dereferenced: B = 0, or refused before the launch
    ok = (4, 8, one, one, 0.7, 0.1, one, 16, one, one, None)
    assert lib.wg_steps_plan_dev(0, *ok[1:]) == 0
    for i, v in ((0, -1), (1, 0), (2, None), (3, None), (4, float("nan")), (5, float("inf")), (6, None), (7, 0), (7, 65), (8, None), (9, None)):
        args = list(ok)
        args[i] = v
        assert lib.wg_steps_plan_dev(*args) == -2, (i, v)
    with wg.Context(0) as ctx:
        assert ctx.call("wg_steps_plan_dev", 0, *ok[1:]) == 0
        d = DevStack(3, 8, 1)
        raw, n = sp.cmd_bytes([sp.CIRCLE] * 3, 3)
        d_cmds, d_n = d.t.from_numpy(raw).cuda(), d.t.from_numpy(n).cuda()
        wg.steps_plan_dev(3, 3, d_cmds.data_ptr(), d_n.data_ptr(), sp.SS, sp.DS, d.stack[1:].data_ptr(), 8, d.steps[1:].data_ptr(),
                          d.n[1:].data_ptr(), ctx=ctx)
        rows, n, st = d.read()
        assert (n == 5).all() and np.array_equal(rows[2, :5], sp.oracle_list(sp.CIRCLE)[0])


@pytest.mark.parametrize("exe,extra", [("kajita_fleet", []), ("kajita_fleet", ["--online", "3"]),
                                       ("dimitrov_fleet", ["--online", "3", "--follow"])])
def test_fleet_programs_print_the_checksum_of_their_host_fed_twins(exe, extra):
    """--plan: the command lists are the only step input uploaded; --plan-host: the same lists through wg_steps_plan and the
    existing upload path"""
    path = os.path.join(ROOT, "jrl-walkgen_amd", "bin", exe)
    assert os.path.exists(path)
    sums = []
    for mode in ("--plan", "--plan-host"):
        r = subprocess.run([path, "--batch", "70", mode] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "FAILED" not in r.stderr, r.stdout + r.stderr
        sums.append(re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1))
    assert sums[0] == sums[1]
