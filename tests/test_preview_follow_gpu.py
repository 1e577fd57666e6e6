"""wg_preview_follow_dev (through the C ABI): the stage-1 preview in which every gait advances over exactly the rows its own queue
has made safe, steps [done[b], length[b] - nl + 1), driven by the `length` array of the wg_zmpdisc on-line calls.  Contract: however
the growth of the queues is cut into calls, state[b] and rows [0, done[b]) of com / zmp2 are the bytes of ONE preview over the
gait's final queue (the oracle's wgo_preview_run per gait, and wg_preview_run_batch_dev), rows >= done[b] are untouched.

The synthetic queues are NaN wherever a gait holds no sample yet: any read at or past length[b] poisons the result.

One departure from the wording of the checks: "in every call at least one gait sits out, at least one advances by exactly 1 and
one wave holds step counts 0, 1 and > 8 together" cannot hold for a fleet of ONE gait.  B = 1 asserts the three kinds of call
over its six calls instead; B = 5 and B = 70 assert them in every call."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zmpref  # noqa: E402
from test_preview_oracle import ini_gains, oracle_run  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu

BAD_ARG = -2
CANARY = -1.2345e300
PER_WAVE = 4                      # gaits of a wave in the split form (four gaits x two axes x eight lanes)


def gains(nl):
    if nl == 320:
        return ini_gains()
    g, F = wg.preview_gains(0.005, 0.814, nl * 0.005 + 1e-9)
    assert g.nl == nl
    return g, F


def scripted_lengths(rng, B, nl, n_calls):
    """[n_calls][B] lengths after each feeding, non-decreasing per gait, the last in [nl - 5, nl + 60].  Gaits 0, 1, 2 take turns:
    in call c gait j runs 9 or 10 steps, exactly 1, or none ((c + j) % 3 = 0, 1, 2) -- together in the first wave; the gait that
    runs none in call 0 holds fewer than nl samples then.  Gait 4 never gets a safe row.  The others grow at random, with calls
    that bring them nothing."""
    ln = np.zeros((n_calls, B), np.int64)
    for b in range(B):
        if b < 3:
            safe = 0
            for c in range(n_calls):
                safe += (int(rng.integers(9, 11)), 1, 0)[(c + b) % 3]
                ln[c, b] = nl - 1 + safe if safe else nl - 3
        elif b == 4:
            ln[:, b] = np.sort(rng.integers(0, nl, n_calls))
            ln[-1, b] = nl - 2
        else:
            fin = int(rng.integers(nl, nl + 61)) if b % 7 else int(rng.integers(nl - 5, nl))
            cuts = np.sort(rng.integers(max(fin - 66, 0), fin + 1, n_calls))
            cuts[-1] = fin
            for c in range(1, n_calls - 1):
                if rng.random() < 0.3:
                    cuts[c] = cuts[c - 1]                     # a call that brings the gait nothing
                elif rng.random() < 0.2 and cuts[c - 1] >= nl:
                    cuts[c] = cuts[c - 1] + 1                 # ... or one sample
            ln[:, b] = np.maximum.accumulate(np.minimum(cuts, fin))
            ln[-1, b] = fin
    assert (np.diff(ln, axis=0) >= 0).all() and (ln[-1] >= nl - 5).all() and (ln[-1] <= nl + 60).all()
    return ln


class Synth:
    """a fleet of synthetic queues on the device, NaN where a gait holds no sample yet"""

    def __init__(self, B, nl, g, F, seed, simulation=True, want_com=True, want_zmp2=True, slack=3, lcap=None):
        import torch
        self.t = torch
        wg.init(0)
        wg.preview_configure(g, F)
        rng = np.random.default_rng(seed)
        self.B, self.nl, self.g, self.F, self.sim = B, nl, g, F, simulation
        self.lcap = lcap or nl + 60 + slack
        self.rows = self.lcap - nl + 1
        zx, zy = zmpref.random_batch(rng, B, self.rows, nl)
        self.Z = (np.ascontiguousarray(zx), np.ascontiguousarray(zy))          # [B][lcap]
        self.s0 = rng.normal(0, 0.01, (B, 8))
        self.have = np.zeros(B, np.int64)
        self.hq = [np.full((self.lcap, B), np.nan) for _ in range(2)]
        self.q = [torch.from_numpy(h.copy()).cuda() for h in self.hq]
        self.state = torch.from_numpy(self.s0.copy()).cuda()
        new = lambda *s: torch.full(s, CANARY, dtype=torch.float64, device="cuda")  # noqa: E731
        self.com = new(self.rows, 6, B) if want_com else None
        self.z2 = new(self.rows, 2, B) if want_zmp2 else None
        self.length = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.done = torch.zeros(B, dtype=torch.int32, device="cuda")

    def feed(self, new_len, report=None):
        """rows [have[b], new_len[b]) of every gait reach the device queue; `report` is what `length` is told (default: the same)"""
        for b in range(self.B):
            lo, hi = int(self.have[b]), int(new_len[b])
            for a in range(2):
                self.hq[a][lo:hi, b] = self.Z[a][b, lo:hi]
        self.have = np.maximum(self.have, np.asarray(new_len, np.int64))
        for a in range(2):
            self.q[a].copy_(self.t.from_numpy(self.hq[a]))
        self.length.copy_(self.t.from_numpy(np.asarray(new_len if report is None else report, np.int32)))

    def follow(self, lcap=None, B=None):
        p = lambda x: x.data_ptr() if x is not None else None  # noqa: E731
        rc = wg.lib().wg_preview_follow_dev(self.B if B is None else B, lcap or self.lcap, p(self.length), p(self.done), p(self.q[0]),
                                            p(self.q[1]), p(self.state), p(self.com), p(self.z2), int(self.sim), None)
        self.t.cuda.synchronize()
        return rc

    def snapshot(self):
        return [x.clone() for x in (self.state, self.com, self.z2, self.done, self.length, *self.q) if x is not None]

    def assert_unchanged(self, snap, gaits=None):
        for a, b in zip(snap, self.snapshot()):
            ix = Ellipsis if gaits is None else ((gaits, slice(None)) if a.shape == (self.B, 8) else (Ellipsis, gaits))
            assert a.cpu().numpy()[ix].tobytes() == b.cpu().numpy()[ix].tobytes()

    def expected(self, b, L):
        """the oracle's whole preview of gait b over L steps: com [L][6], zmp2 [L][2], state [8]"""
        s = self.s0[b:b + 1].copy()
        if L == 0:
            return np.zeros((0, 6)), np.zeros((0, 2)), s[0]
        n = L + self.nl - 1
        com, z2 = oracle_run(self.g, self.F, self.Z[0][b:b + 1, :n], self.Z[1][b:b + 1, :n], s, L, simulation=self.sim)
        return com[0], z2[0], s[0]

    def fresh_rows(self):
        """per output column, the number of rows that no longer hold the canary: com x, com y, zmp2 x, zmp2 y -> [4][B]"""
        com, z2 = self.com.cpu().numpy(), self.z2.cpu().numpy()
        cols = [com[:, 0:3], com[:, 3:6], z2[:, 0:1], z2[:, 1:2]]
        return np.array([(c != CANARY).all(axis=1).sum(axis=0) for c in cols]), np.array([(c != CANARY).any(axis=1).sum(axis=0) for c in cols])

    def assert_equals_oracle(self, done, gaits=None):
        st = self.state.cpu().numpy()
        com = self.com.cpu().numpy() if self.com is not None else None
        z2 = self.z2.cpu().numpy() if self.z2 is not None else None
        for b in (range(self.B) if gaits is None else gaits):
            L = int(done[b])
            c, p, s = self.expected(b, L)
            assert np.array_equal(st[b], s), b
            if com is not None:
                assert np.array_equal(com[:L, :, b], c), b
                assert (com[L:, :, b] == CANARY).all(), b                  # rows >= done[b] are untouched
            if z2 is not None:
                assert np.array_equal(z2[:L, :, b], p), b
                assert (z2[L:, :, b] == CANARY).all(), b


def safe_rows(ln, nl):
    return np.maximum(0, np.asarray(ln, np.int64) - nl + 1)


@pytest.mark.parametrize("B", [1, 5, 70])
def test_ragged_growth_equals_the_whole_preview(B):
    """checks 1, 2 and 3: six ragged calls against the whole preview, both axes in step after every call, and a call that
    brings nothing touches nothing"""
    nl = 320
    g, F = gains(nl)
    rng = np.random.default_rng(500 + B)
    plan = scripted_lengths(rng, B, nl, 6)
    assert (plan[-1] < nl).any() or B < 5                           # some gaits never get a safe row
    f = Synth(B, nl, g, F, seed=B)
    done = np.zeros(B, np.int64)
    kinds = set()
    for c in range(6):
        f.feed(plan[c])
        n = safe_rows(plan[c], nl) - done
        sits, one = (n == 0).any(), (n == 1).any()
        mixed = any({0, 1} <= set(n[w:w + PER_WAVE]) and (n[w:w + PER_WAVE] > 8).any() for w in range(0, B, PER_WAVE))
        if B >= 5:
            assert sits and one and mixed, c
        kinds |= {k for k, v in (("sits", sits), ("one", one), ("long", (n > 8).any())) if v}
        assert f.follow() == 0
        done += n
        assert np.array_equal(f.done.cpu().numpy(), done), c
        all_fresh, any_fresh = f.fresh_rows()                       # the two axes of a gait advance together
        assert np.array_equal(all_fresh, any_fresh)
        for col in all_fresh:
            assert np.array_equal(col, done), c
    assert kinds == {"sits", "one", "long"}
    assert np.array_equal(done, safe_rows(plan[-1], nl))
    f.assert_equals_oracle(done)
    assert f.state.cpu().numpy()[done > 0].any()
    snap = f.snapshot()                                             # no length changed: every gait sits out
    assert f.follow() == 0
    f.assert_unchanged(snap)


SHAPES = [(64, "split"), (100, "split"), (200, "split"), (320, "split"), (350, "split"), (40, None), (400, None), (320, "l2"),
          (144, "split"), (150, "split"), (224, "split"), (300, "split"), (336, "split")]


@pytest.mark.parametrize("sim", [0, 1])
@pytest.mark.parametrize("nl,kernel", SHAPES)
def test_every_kernel_shape(nl, kernel, sim, monkeypatch):
    """check 4: T = 16 full, 16 part, 32 part, 40 full, 48 part of the split form; the plain form below and above the split's
    windows and forced at nl = 320; second row of SHAPES: T = 24 full, 24 part, 32 full, 40 part, 48 full, so that every
    instantiation of the follow form is launched"""
    if kernel:
        monkeypatch.setenv("WG_PREVIEW_KERNEL", kernel)
    else:
        monkeypatch.delenv("WG_PREVIEW_KERNEL", raising=False)
    g, F = gains(nl)
    B = 37
    plan = scripted_lengths(np.random.default_rng(nl), B, nl, 3)
    f = Synth(B, nl, g, F, seed=nl + sim, simulation=bool(sim))
    for c in range(3):
        f.feed(plan[c])
        assert f.follow() == 0
    done = safe_rows(plan[-1], nl)
    assert np.array_equal(f.done.cpu().numpy(), done) and (done > 0).any() and (done == 0).any()
    f.assert_equals_oracle(done)
    if not sim:
        assert np.array_equal(f.state.cpu().numpy()[:, 6:], f.s0[:, 6:])


@pytest.mark.parametrize("kernel", ["split", "l2"])
def test_null_output_forms(kernel, monkeypatch):
    monkeypatch.setenv("WG_PREVIEW_KERNEL", kernel)
    g, F = gains(320)
    plan = scripted_lengths(np.random.default_rng(9), 37, 320, 3)
    for com, z2 in ((False, True), (True, False), (False, False)):
        f = Synth(37, 320, g, F, seed=3, want_com=com, want_zmp2=z2)
        for c in range(3):
            f.feed(plan[c])
            assert f.follow() == 0
        f.assert_equals_oracle(safe_rows(plan[-1], 320))


@pytest.mark.parametrize("kernel", ["split", "l2"])
def test_refusals_and_sitting_out(kernel, monkeypatch):
    """check 5, on the device: length > lcap and done > safe are refused for good, length < 0 and done < 0 sit out, and none
    of their bytes but the refused gaits' done is written; their neighbours -- in the same wave -- equal the oracle"""
    monkeypatch.setenv("WG_PREVIEW_KERNEL", kernel)
    nl, B = 320, 10
    g, F = gains(nl)
    f = Synth(B, nl, g, F, seed=17)
    OVER, AHEAD, NOLEN, NODONE = 1, 3, 5, 6
    odd = [OVER, AHEAD, NOLEN, NODONE]
    others = [b for b in range(B) if b not in odd]
    ln = np.full(B, nl + 20, np.int64)
    ln[0], ln[9] = nl + 1, nl - 1
    report = ln.copy()
    report[OVER], report[NOLEN] = f.lcap + 1, -1                    # gait AHEAD: 5 steps behind it, of which its queue allows 3
    ln[AHEAD] = report[AHEAD] = nl + 2
    d0 = np.zeros(B, np.int32)
    d0[AHEAD], d0[NODONE] = 5, -7
    f.done.copy_(f.t.from_numpy(d0))
    f.feed(ln, report)
    snap = f.snapshot()
    assert f.follow() == 0
    want = safe_rows(ln, nl)
    want[OVER] = want[AHEAD] = BAD_ARG
    want[NOLEN], want[NODONE] = 0, -7
    assert np.array_equal(f.done.cpu().numpy(), want)
    f.assert_unchanged(snap[:3], gaits=odd)                         # state, com, zmp2
    f.assert_equals_oracle(want, gaits=others)
    # every later call leaves them alone, although their arguments are in order now
    ln2 = ln + 7
    f.feed(ln2)
    assert f.follow() == 0
    want2 = safe_rows(ln2, nl)                                      # gait NOLEN has a length now and done = 0: it starts its walk
    keep = [OVER, AHEAD, NODONE]                                    # ... the three others keep their codes
    want2[keep] = want[keep]
    assert np.array_equal(f.done.cpu().numpy(), want2)
    f.assert_unchanged(snap[:3], gaits=keep)
    f.assert_equals_oracle(want2, gaits=others + [NOLEN])


def test_host_side_errors_launch_nothing():
    """check 5, on the host: WG_ERR_BAD_ARG and no launch (every buffer unchanged); B = 0 is WG_OK"""
    nl = 320
    g, F = gains(nl)
    f = Synth(4, nl, g, F, seed=1)
    f.feed(np.full(4, nl + 10))
    snap = f.snapshot()
    lib = wg.lib()
    p = lambda x: x.data_ptr()  # noqa: E731
    args = [4, f.lcap, p(f.length), p(f.done), p(f.q[0]), p(f.q[1]), p(f.state), p(f.com), p(f.z2), 1, None]

    def call(**kw):
        a = list(args)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.wg_preview_follow_dev(*a)
    with wg.Context(0) as ctx:                                      # a context without wg_preview_configure
        assert ctx.call("wg_preview_follow_dev", *args) == BAD_ARG
    assert call(a1=nl - 1) == BAD_ARG                               # lcap < nl
    assert call(a2=None) == BAD_ARG and call(a3=None) == BAD_ARG    # length, done
    assert call(a4=None) == BAD_ARG and call(a5=None) == BAD_ARG and call(a6=None) == BAD_ARG
    assert call(a0=-1) == BAD_ARG
    assert call(a0=0) == 0
    f.t.cuda.synchronize()
    f.assert_unchanged(snap)
    assert f.follow() == 0                                          # ... and the same arguments in order do run
    assert np.array_equal(f.done.cpu().numpy(), np.full(4, 11))


def test_with_the_real_walk():
    """check 6: the loop of test_a_gait_ends_while_others_go_on with the preview behind every begin / append / end, fed by the
    `length` array those calls wrote; the host reads nothing back between the calls"""
    import torch
    from test_zmpdisc_online_gpu import Walk, ragged_fleet, ragged_plan

    class QuietWalk(Walk):
        def lengths(self):                                          # Walk's calls return this: no read-back, no synchronisation
            return None

    f = ragged_fleet(70, 3.0)
    g, F = gains(320)
    wg.preview_configure(g, F)
    nl, B = g.nl, f.B
    assert (f.lens >= nl).all() and len(set(f.lens.tolist())) > 8
    rows = f.lcap - nl + 1
    new = lambda *s: torch.full(s, CANARY, dtype=torch.float64, device="cuda")  # noqa: E731
    Lmax = int(f.lens.max()) - nl + 1
    st1, com1, z1 = torch.zeros(B, 8, dtype=torch.float64, device="cuda"), new(rows, 6, B), new(rows, 2, B)
    wg.preview_run_batch_dev(B, Lmax, f.full["zmp_x"].data_ptr(), f.full["zmp_y"].data_ptr(), st1.data_ptr(), com1.data_ptr(), z1.data_ptr())
    st2, com2, z2 = torch.zeros(B, 8, dtype=torch.float64, device="cuda"), new(rows, 6, B), new(rows, 2, B)
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    w = QuietWalk(f, ("zmp_x", "zmp_y"))

    def follow():
        wg.preview_follow_dev(B, f.lcap, w.buf["length"].data_ptr(), done.data_ptr(), w.buf["zmp_x"].data_ptr(), w.buf["zmp_y"].data_ptr(),
                              st2.data_ptr(), com2.data_ptr(), z2.data_ptr())
    plan = ragged_plan(np.random.default_rng(B), f.n_steps)
    assert len(plan) > 2
    for i, counts in enumerate(plan):
        w.begin(counts) if i == 0 else w.append(counts)
        follow()
        ends = (w.given == f.n_steps) & ~w.ended                    # host bookkeeping of what was GIVEN, as in the loop it repeats
        w.end(ends.astype(np.int32))
        follow()
    torch.cuda.synchronize()
    assert w.ended.all()
    assert np.array_equal(w.buf["length"].cpu().numpy(), f.lens)
    L = f.lens.astype(np.int64) - nl + 1
    assert np.array_equal(done.cpu().numpy(), L)
    c1, c2, p1, p2 = (x.cpu().numpy() for x in (com1, com2, z1, z2))
    zx, zy = f.host_queue()
    s2 = st2.cpu().numpy()
    for b in range(B):
        n = int(L[b])
        assert np.array_equal(c1[:n, :, b], c2[:n, :, b]) and np.array_equal(p1[:n, :, b], p2[:n, :, b]), b
        assert (c2[n:, :, b] == CANARY).all() and (p2[n:, :, b] == CANARY).all(), b
        s = np.zeros((1, 8))
        oracle_run(g, F, np.ascontiguousarray(zx[:f.lens[b], b])[None], np.ascontiguousarray(zy[:f.lens[b], b])[None], s, n)
        assert np.array_equal(s2[b], s[0]), b
    assert np.abs(s2).max() > 0


def test_kajita_fleet_ragged_online_prints_the_batch_checksum():
    """check 7: host/kajita_fleet.cpp --ragged: step counts in [S/2, S], gaits ended as their steps run out, the preview following
    d_len -- against the batch path on the same fleet, each gait's own rows"""
    exe = os.path.join(ROOT, "jrl-walkgen_amd", "bin", "kajita_fleet")
    assert os.path.exists(exe)
    sums = []
    for extra in ([], ["--online", "3"]):
        r = subprocess.run([exe, "--ragged", "--batch", "70", "--steps", "8"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ragged" in r.stdout, r.stdout + r.stderr
        sums.append(re.search(r"checksum ([0-9a-f]{16})", r.stdout).group(1))
    assert sums[0] == sums[1]
