"""wg_preview_run_fleet_dev / wg_preview_follow_fleet_dev (through the C ABI): the stage-1 preview of a fleet whose gaits differ
in CoM height, every gait with its own gains (zc [B], K_tm [4][B], F_tm [nl][B] on the device).  Contract: gait b's bytes are
those of a preview configured with gait b's gains -- the oracle's wgo_preview_run, called once per gait with that gait's
wg_riccati_gains -- in every kernel form: eight lanes per gait and axis for windows of 64 .. 384 samples (T = 40 FULL at
nl = 320, T = 16 not FULL with seven lanes at nl = 100, T = 16 with four lanes at nl = 64), one lane per gait and axis below
and above (nl = 40, 400), batch and follow.

The follow form's queues are NaN wherever a gait holds no sample yet: any read at or past length[b] poisons the result."""
import ctypes as C
import importlib
import os
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
T = 0.005
GUARD = 2                                       # canary rows behind the rows a call may write

_gains = {}


def gains_of(zc, nl):
    """(PreviewGains, F[nl]) of one height, from the host call; computed once per (height, window)"""
    key = (float(zc), nl)
    if key not in _gains:
        g, F = wg.preview_gains(T, float(zc), nl * T + 1e-9)
        assert g.nl == nl
        F.setflags(write=False)
        _gains[key] = (g, F)
    return _gains[key]


def heights(B, seed=0):
    return np.random.default_rng(1000 + B + seed).uniform(0.5, 1.0, B)


class Fleet:
    """zc, K_tm, F_tm of B heights on the device, and the wg_preview_fleet_t over them"""

    def __init__(self, zc, nl):
        import torch
        wg.init(0)
        self.zc, self.nl, self.B = np.array(zc, dtype=np.float64), nl, len(zc)
        self.g = [gains_of(z, nl) for z in self.zc]
        K = np.array([[g.Ks, g.Kx[0], g.Kx[1], g.Kx[2]] for g, _ in self.g]).T          # [4][B]
        F = np.array([f for _, f in self.g]).T                                          # [nl][B]
        self.dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (self.zc, K, F)]
        self.c = wg.preview_fleet(T, nl, *(d.data_ptr() for d in self.dev))

    def oracle(self, b, zx, zy, s0, L, sim):
        """gait b alone with its own gains: com [L][6], zmp2 [L][2], state [8]"""
        s = np.array(s0, dtype=np.float64)[None].copy()
        if L == 0:
            return np.zeros((0, 6)), np.zeros((0, 2)), s[0]
        g, F = self.g[b]
        n = L + self.nl - 1
        com, z2 = oracle_run(g, F, np.ascontiguousarray(zx[None, :n]), np.ascontiguousarray(zy[None, :n]), s, L, simulation=sim)
        return com[0], z2[0], s[0]


def p(x):
    return x.data_ptr() if x is not None else None


def run_fleet(fl, ZX, ZY, s0, L, sim=True, want_com=True, want_z2=True, ctx=None):
    """one batch call: ZX, ZY [B][L + nl - 1] gait-major on the host -> state [B][8], com [L + GUARD][6][B], zmp2 [L + GUARD][2][B]"""
    import torch
    B = fl.B
    zx = torch.from_numpy(np.ascontiguousarray(ZX[:, :L + fl.nl - 1].T)).cuda()
    zy = torch.from_numpy(np.ascontiguousarray(ZY[:, :L + fl.nl - 1].T)).cuda()
    st = torch.from_numpy(np.ascontiguousarray(s0)).cuda()
    new = lambda *s: torch.full(s, CANARY, dtype=torch.float64, device="cuda")  # noqa: E731
    com = new(L + GUARD, 6, B) if want_com else None
    z2 = new(L + GUARD, 2, B) if want_z2 else None
    args = (B, L, C.addressof(fl.c), p(zx), p(zy), p(st), p(com), p(z2), int(sim), None)
    rc = ctx.call("wg_preview_run_fleet_dev", *args) if ctx else wg.lib().wg_preview_run_fleet_dev(*args)
    assert rc == 0, wg.lib().wg_last_error()
    torch.cuda.synchronize()
    return st.cpu().numpy(), com.cpu().numpy() if want_com else None, z2.cpu().numpy() if want_z2 else None


def assert_gaits_equal_oracle(fl, ZX, ZY, s0, L, sim, st, com, z2, gaits=None):
    for b in (range(fl.B) if gaits is None else gaits):
        c, q, s = fl.oracle(b, ZX[b], ZY[b], s0[b], L, sim)
        assert np.array_equal(st[b], s), b
        if com is not None:
            assert np.array_equal(com[:L, :, b], c), b
        if z2 is not None:
            assert np.array_equal(z2[:L, :, b], q), b
    if com is not None:
        assert (com[L:] == CANARY).all()
    if z2 is not None:
        assert (z2[L:] == CANARY).all()


@pytest.mark.parametrize("nl", [320, 100, 64, 40, 400])
@pytest.mark.parametrize("B", [1, 9, 70])
def test_batch_form_bit_parity_per_gait(B, nl):
    """B = 9 leaves surplus groups in the second block of the split form, B = 70 crosses a wave of the plain form; L = 1 and 23,
    with and without the simulation, com and zmp2 each left out once"""
    fl = Fleet(heights(B), nl)
    rng = np.random.default_rng(nl * 100 + B)
    ZX, ZY = zmpref.random_batch(rng, B, 23, nl)
    s0 = rng.normal(0, 0.01, (B, 8))
    for L in (1, 23):
        for sim in (True, False):
            outs = ((True, True),) if (L, sim) != (23, True) else ((True, True), (False, True), (True, False))
            for want_com, want_z2 in outs:
                st, com, z2 = run_fleet(fl, ZX, ZY, s0, L, sim, want_com, want_z2)
                assert_gaits_equal_oracle(fl, ZX, ZY, s0, L, sim, st, com, z2)
                if not sim:
                    assert np.array_equal(st[:, 6:], s0[:, 6:])
    assert B == 1 or len({st[b].tobytes() for b in range(B)}) == B


@pytest.mark.parametrize("nl", [320, 40])
def test_one_height_for_all_equals_the_configured_call(nl):
    import torch
    B, L = 9, 23
    g, F = gains_of(0.814, nl)
    fl = Fleet(np.full(B, 0.814), nl)
    rng = np.random.default_rng(nl)
    ZX, ZY = zmpref.random_batch(rng, B, L, nl)
    s0 = rng.normal(0, 0.01, (B, 8))
    st, com, z2 = run_fleet(fl, ZX, ZY, s0, L)
    wg.preview_configure(g, F)
    zx, zy = (torch.from_numpy(np.ascontiguousarray(Z.T)).cuda() for Z in (ZX, ZY))
    st1 = torch.from_numpy(s0.copy()).cuda()
    com1 = torch.full((L + GUARD, 6, B), CANARY, dtype=torch.float64, device="cuda")
    z21 = torch.full((L + GUARD, 2, B), CANARY, dtype=torch.float64, device="cuda")
    wg.preview_run_batch_dev(B, L, p(zx), p(zy), p(st1), p(com1), p(z21))
    torch.cuda.synchronize()
    assert st.tobytes() == st1.cpu().numpy().tobytes()
    assert com.tobytes() == com1.cpu().numpy().tobytes() and z2.tobytes() == z21.cpu().numpy().tobytes()
    assert np.abs(com[:L]).max() > 0


@pytest.mark.parametrize("nl", [320, 40])
def test_swapped_heights_change_exactly_those_two_gaits(nl):
    """guards the layout of F_tm and K_tm: gait-major indexing would move every gait"""
    B, L = 9, 23
    zc = heights(B)
    sw = zc.copy()
    sw[[2, 5]] = zc[[5, 2]]
    rng = np.random.default_rng(7 + nl)
    ZX, ZY = zmpref.random_batch(rng, B, L, nl)
    s0 = rng.normal(0, 0.01, (B, 8))
    a = run_fleet(Fleet(zc, nl), ZX, ZY, s0, L)
    fs = Fleet(sw, nl)
    b = run_fleet(fs, ZX, ZY, s0, L)
    same = [g for g in range(B) if g not in (2, 5)]
    assert a[0][same].tobytes() == b[0][same].tobytes()
    assert a[1][..., same].tobytes() == b[1][..., same].tobytes() and a[2][..., same].tobytes() == b[2][..., same].tobytes()
    for g in (2, 5):
        assert not np.array_equal(a[0][g], b[0][g]) and not np.array_equal(a[1][:L, :, g], b[1][:L, :, g])
    assert_gaits_equal_oracle(fs, ZX, ZY, s0, L, True, *b, gaits=(2, 5))


def test_context_is_not_touched_and_context_forms():
    """the configured gains of a context give the same bytes before and after a fleet call on it; the _ctx form on a second
    context, never configured, equals the default one"""
    import torch
    B, L, nl = 9, 23, 320
    g, F = ini_gains()
    rng = np.random.default_rng(4)
    ZX, ZY = zmpref.random_batch(rng, B, L, nl)
    s0 = rng.normal(0, 0.01, (B, 8))
    zx, zy = (torch.from_numpy(np.ascontiguousarray(Z.T)).cuda() for Z in (ZX, ZY))

    def configured():
        st = torch.from_numpy(s0.copy()).cuda()
        com = torch.zeros(L, 6, B, dtype=torch.float64, device="cuda")
        z2 = torch.zeros(L, 2, B, dtype=torch.float64, device="cuda")
        wg.preview_run_batch_dev(B, L, p(zx), p(zy), p(st), p(com), p(z2))
        torch.cuda.synchronize()
        return b"".join(x.cpu().numpy().tobytes() for x in (st, com, z2))
    wg.init(0)
    wg.preview_configure(g, F)
    before = configured()
    fl = Fleet(heights(B), nl)
    out = run_fleet(fl, ZX, ZY, s0, L)
    fl40 = Fleet(heights(B), 40)                                              # another window than the configured one
    Z40 = zmpref.random_batch(rng, B, L, 40)
    run_fleet(fl40, Z40[0], Z40[1], s0, L)
    assert int(wg.lib().wg_preview_window()) == nl
    assert configured() == before
    with wg.Context(0) as ctx:
        assert int(ctx.call("wg_preview_window")) == 0
        out2 = run_fleet(fl, ZX, ZY, s0, L, ctx=ctx)
        assert int(ctx.call("wg_preview_window")) == 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(out, out2))
    assert wg.lib().wg_preview_run_fleet_dev(0, L, C.addressof(fl.c), p(zx), p(zy), p(zx), None, None, 1, None) == 0
    assert wg.lib().wg_preview_run_fleet_dev(B, 0, C.addressof(fl.c), p(zx), p(zy), p(zx), None, None, 1, None) == 0


# ---- the follow form -----------------------------------------------------------------------------------------------------------

def scripted_lengths(rng, B, nl, n_calls):
    """[n_calls][B] lengths after each feeding, non-decreasing per gait, the last in [nl - 5, nl + 60] (the generator of
    test_preview_follow_gpu.py).  Gaits 0, 1, 2 take turns: in call c gait j runs 9 or 10 steps, exactly 1, or none
    ((c + j) % 3 = 0, 1, 2) -- together in the first wave.  Gait 4 never gets a safe row.  The others grow at random, with calls
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
                    cuts[c] = cuts[c - 1]
                elif rng.random() < 0.2 and cuts[c - 1] >= nl:
                    cuts[c] = cuts[c - 1] + 1
            ln[:, b] = np.maximum.accumulate(np.minimum(cuts, fin))
            ln[-1, b] = fin
    assert (np.diff(ln, axis=0) >= 0).all() and (ln[-1] >= nl - 5).all() and (ln[-1] <= nl + 60).all()
    return ln


def safe_rows(ln, nl):
    return np.maximum(0, np.asarray(ln, np.int64) - nl + 1)


@pytest.mark.parametrize("nl", [320, 40])
@pytest.mark.parametrize("B", [5, 70])
def test_follow_form_equals_one_batch_run_over_the_final_queue(B, nl):
    """four ragged feedings.  Gait 4 never gets a safe row; gait 3 sits the first call out (length < 0) and joins after it; at
    B = 70 gait 10 sits every call out and gait 11 is refused in the first call (length > lcap) and stays so."""
    import torch
    n_calls = 4
    fl = Fleet(heights(B, seed=nl), nl)
    rng = np.random.default_rng(900 + B + nl)
    plan = scripted_lengths(rng, B, nl, n_calls)
    lcap = nl + 63
    rows = lcap - nl + 1
    ZX, ZY = zmpref.random_batch(rng, B, rows, nl)                              # [B][lcap]: the final queues
    s0 = rng.normal(0, 0.01, (B, 8))
    SITS, REFUSED = (10, 11) if B > 11 else (None, None)

    _whole = {}

    def whole(d):
        """ONE batch fleet run of d steps over the final queue"""
        if d not in _whole:
            _whole[d] = run_fleet(fl, ZX, ZY, s0, d) if d > 0 else (s0, None, None)
        return _whole[d]

    hq = [np.full((lcap, B), np.nan) for _ in range(2)]
    q = [torch.from_numpy(h.copy()).cuda() for h in hq]
    state = torch.from_numpy(s0.copy()).cuda()
    com = torch.full((rows + GUARD, 6, B), CANARY, dtype=torch.float64, device="cuda")
    z2 = torch.full((rows + GUARD, 2, B), CANARY, dtype=torch.float64, device="cuda")
    length = torch.zeros(B, dtype=torch.int32, device="cuda")
    done = torch.zeros(B, dtype=torch.int32, device="cuda")
    have = np.zeros(B, np.int64)
    want = np.zeros(B, np.int64)
    kinds = set()
    for c in range(n_calls):
        for b in range(B):
            lo, hi = int(have[b]), int(plan[c, b])
            hq[0][lo:hi, b] = ZX[b, lo:hi]
            hq[1][lo:hi, b] = ZY[b, lo:hi]
        have = plan[c].copy()
        report = plan[c].copy()
        if c == 0:
            report[3] = -1
        if SITS is not None:
            report[SITS] = -1
            if c == 0:
                report[REFUSED] = lcap + 1
        for a in range(2):
            q[a].copy_(torch.from_numpy(hq[a]))
        length.copy_(torch.from_numpy(report.astype(np.int32)))
        rc = wg.lib().wg_preview_follow_fleet_dev(B, lcap, p(length), p(done), C.addressof(fl.c), p(q[0]), p(q[1]), p(state), p(com),
                                                  p(z2), 1, None)
        assert rc == 0, wg.lib().wg_last_error()
        torch.cuda.synchronize()
        for b in range(B):
            if report[b] < 0 or want[b] < 0:
                kinds.add("sits")
            elif report[b] > lcap:
                want[b] = BAD_ARG
                kinds.add("refused")
            else:
                want[b] = safe_rows(report[b], nl)
        assert np.array_equal(done.cpu().numpy(), want), c
        st, cm, zz = state.cpu().numpy(), com.cpu().numpy(), z2.cpu().numpy()
        Lmax = int(want.max())
        _, wc, wz = whole(Lmax)
        for b in range(B):
            d = max(int(want[b]), 0)
            assert np.array_equal(st[b], whole(d)[0][b]), (c, b)
            assert np.array_equal(cm[:d, :, b], wc[:d, :, b]) and np.array_equal(zz[:d, :, b], wz[:d, :, b]), (c, b)
            assert (cm[d:, :, b] == CANARY).all() and (zz[d:, :, b] == CANARY).all(), (c, b)
    assert want[4] == 0 and plan[-1, 4] < nl and want[3] > 0
    kinds.add("never safe")
    assert kinds == ({"sits", "refused", "never safe"} if B > 11 else {"sits", "never safe"})
    if B > 11:
        assert want[SITS] == 0 and want[REFUSED] == BAD_ARG
    assert (want > 8).any() and np.isfinite(st).all()
    # the final state against the oracle, every gait with its own gains
    for b in range(B):
        d = max(int(want[b]), 0)
        c_, q_, s_ = fl.oracle(b, ZX[b], ZY[b], s0[b], d, True)
        assert np.array_equal(st[b], s_) and np.array_equal(cm[:d, :, b], c_) and np.array_equal(zz[:d, :, b], q_), b


# The windows above reach T = 16 (both), 40 FULL of the split form.  These reach the rest -- T = 24 FULL / not, 32 FULL / not,
# 40 not, 48 FULL / not -- so that every instantiation of the fleet forms is launched: the batch form with one partial block,
# the follow form with its sitting-out and its refused gait.
SPLIT_REST = [144, 150, 224, 200, 300, 336, 350]


@pytest.mark.parametrize("nl", SPLIT_REST)
def test_batch_form_every_other_split_instantiation(nl):
    test_batch_form_bit_parity_per_gait(9, nl)


@pytest.mark.parametrize("nl", [64, 100] + SPLIT_REST)
def test_follow_form_every_other_split_instantiation(nl):
    test_follow_form_equals_one_batch_run_over_the_final_queue(70, nl)
