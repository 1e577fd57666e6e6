"""The walk audit on the device (wg_zmp_audit_dev, wg_zmp_audit_append_dev and their _ctx forms) against the host twin
wg_zmp_audit, which tests/test_zmp_audit_host.py holds to the rule's restatement and to the geometric truth.  Every comparison is
byte equality: the 32 bytes of every gait's wg_zmp_audit_t and every sample's margin, with canary rows around every array.

Shapes: B = 67 (one full wave and a partial one), lcap = 3 CH + 5 with CH = wg_foot_constraints_chunk(): three full chunks and a
partial one, ragged lengths on and around every chunk edge.  The chains run the 70-gait fleet of tests/test_dimitrov_walk_gpu.py
and a 5-gait Morisawa fleet at smax = 3."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zmpaudit as za  # noqa: E402
import morisawa_fleets as mf  # noqa: E402
from test_zmp_audit_host import ASZ, CANARY, CH, FILL_B, N as LCAP, clone, hp, library_queue, track  # noqa: E402
from test_zmpdisc_online_gpu import Fleet, Walk  # noqa: E402
from test_dimitrov_walk_gpu import BF, PSZ, QCAP, SMAX, SOLE, device_queues, fleet70, times  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu

B = 67
QC = 8                                         # the synthetic queues' capacity
BAD = -2
PATTERN = bytes([FILL_B] * ASZ)
REFUSED = PATTERN[:28] + BAD.to_bytes(4, "little", signed=True)
EMPTY = za.pack(za.EMPTY)
LENGTHS = [0, 1, CH - 1, CH, CH + 1, 2 * CH - 1, 2 * CH, 2 * CH + 1, 3 * CH - 1, 3 * CH, 3 * CH + 1, LCAP]


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


# ---- the host twin on copied-back arrays -----------------------------------------------------------------------------------
def host_audits(time, px, py, queues, ts, te, count, qcap, lengths, lcap, refused=()):
    """per gait wg_zmp_audit(0, length[b], ...): ([B] 32-byte strings, margins [lcap][B] with CANARY where nothing is written).
    px, py [lcap][B]; queues [B][qcap * PSZ] uint8; a gait in `refused` keeps the pattern and gets the status"""
    nb = len(lengths)
    audits, margins = [], np.full((lcap, nb), CANARY)
    for b in range(nb):
        L = int(lengths[b])
        if b in refused:
            audits.append(REFUSED)
            continue
        A = wg.ZmpAudit()
        m = np.full(max(L, 1), CANARY)
        x, y = np.ascontiguousarray(px[:L, b]), np.ascontiguousarray(py[:L, b])
        q = np.ascontiguousarray(queues[b])
        rc = wg.lib().wg_zmp_audit(0, L, hp(time), hp(x), hp(y), 1, int(count[b]), qcap, hp(q), hp(np.ascontiguousarray(ts[b])),
                                   hp(np.ascontiguousarray(te[b])), C.addressof(A), hp(m))
        assert rc == 0, (b, rc)
        audits.append(bytes(A))
        margins[:L, b] = m[:L]
    return audits, margins


class Synthetic:
    """B gaits on the five-phase queue of tests/test_zmp_audit_host.py, each with its own track, ragged lengths, a few queues
    altered (a short count, a count past the capacity, an empty queue, a bad row count), non-finite samples, and three gaits the
    call refuses.  The tracks lie in one [lcap + 2][2][B] array between canary rows, so pitch = 2 B reads it as it is; the
    pitch = B runs read compact copies.  Past a gait's length the tracks hold NaN."""

    def __init__(self):
        rng = np.random.default_rng(5)
        self.t, q = library_queue()
        self.lengths = np.array((LENGTHS + [int(v) for v in rng.integers(1, LCAP + 1, B)])[:B], np.int32)
        self.count = np.full(B, q[3], np.int32)
        self.queues = np.zeros((B, QC * PSZ), np.uint8); self.ts = np.full((B, QC), CANARY); self.te = np.full((B, QC), CANARY)
        xy = np.zeros((LCAP, 2, B))
        for b in range(B):
            g = clone(q)
            if b == 20:
                self.count[b] = 2
            elif b == 21:
                self.count[b] = QC + 3
            elif b == 22:
                self.count[b] = 0
            elif b == 23:
                g[0][3].nrows = 9
            self.queues[b, :q[3] * PSZ] = np.frombuffer(bytes(g[0]), np.uint8)[:q[3] * PSZ]
            self.queues[b, q[3] * PSZ:] = FILL_B
            self.ts[b, :q[3]], self.te[b, :q[3]] = g[1], g[2]
            xy[:, 0, b], xy[:, 1, b] = track(100 + b, self.t)
        xy[7, 0, 30], xy[70, 1, 30], xy[130, 0, 31] = float("nan"), float("inf"), -float("inf")
        self.lengths[[20, 21, 22, 23, 30, 31]] = LCAP
        self.refused = {40: "length -1", 41: "length lcap + 1", 66: "count -2"}
        self.lengths[40], self.lengths[41], self.count[66] = -1, LCAP + 1, -2
        for b in range(B):
            xy[max(int(self.lengths[b]), 0):, :, b] = float("nan")
        self.xy = xy

    def upload(self):
        import torch
        xy = self.xy
        pad = np.full((1, 2, B), CANARY)
        self.d_xy = dev(np.concatenate([pad, xy, pad]))
        self.d_x, self.d_y = dev(np.concatenate([pad[:, 0], xy[:, 0], pad[:, 0]])), dev(np.concatenate([pad[:, 0], xy[:, 1], pad[:, 0]]))
        self.d_time, self.d_q, self.d_ts, self.d_te = dev(self.t), dev(self.queues), dev(self.ts), dev(self.te)
        self.d_count, self.d_len = dev(self.count), dev(self.lengths)
        self.torch = torch
        return self

    def track_ptrs(self, pitch):
        if pitch == B:
            return self.d_x[1:].data_ptr(), self.d_y[1:].data_ptr()
        assert pitch == 2 * B
        return self.d_xy[1:].data_ptr(), self.d_xy[1:].data_ptr() + 8 * B

    def expect(self, lengths, refused=None):
        return host_audits(self.t, self.xy[:, 0], self.xy[:, 1], self.queues, self.ts, self.te, self.count, QC, lengths, LCAP,
                           self.refused if refused is None else refused)

    def outputs(self):
        t = self.torch
        return (t.full((B + 2, ASZ), FILL_B, dtype=t.uint8, device="cuda"), t.full((LCAP + 2, B), CANARY, dtype=t.float64, device="cuda"))

    def inputs_untouched(self):
        for d, h in ((self.d_q, self.queues), (self.d_ts, self.ts), (self.d_te, self.te), (self.d_count, self.count), (self.d_len, self.lengths)):
            assert d.cpu().numpy().tobytes() == h.tobytes()
        got = self.d_xy.cpu().numpy()
        assert (got[0] == CANARY).all() and (got[-1] == CANARY).all() and got[1:-1].tobytes() == self.xy.tobytes()


def check_outputs(audit, margin, want_audits, want_margins, what=""):
    """device outputs (with their canary rows) against the host's"""
    a, m = audit.cpu().numpy(), margin.cpu().numpy()
    assert a[0].tobytes() == PATTERN and a[-1].tobytes() == PATTERN, what
    assert (m[0] == CANARY).all() and (m[-1] == CANARY).all(), what
    for b, want in enumerate(want_audits):
        assert a[1 + b].tobytes() == want, (what, b, wg.ZmpAudit.from_buffer_copy(a[1 + b].tobytes()).margin)
    if want_margins is not None:
        assert m[1:-1].tobytes() == want_margins.tobytes(), what


@pytest.fixture(scope="module")
def syn():
    wg.init(0)
    assert wg.foot_constraints_chunk() == CH
    s = Synthetic().upload()
    s.want = s.expect(s.lengths)
    return s


# ---- 1. the batch call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_margin", [True, False])
@pytest.mark.parametrize("pitch", [B, 2 * B])
def test_batch_is_the_host_twin(syn, pitch, with_margin):
    audit, margin = syn.outputs()
    px, py = syn.track_ptrs(pitch)
    wg.zmp_audit_dev(B, LCAP, syn.d_len.data_ptr(), syn.d_time.data_ptr(), px, py, pitch, QC, syn.d_q.data_ptr(), syn.d_ts.data_ptr(),
                     syn.d_te.data_ptr(), syn.d_count.data_ptr(), audit[1:].data_ptr(), margin[1:].data_ptr() if with_margin else None,
                     _stream())
    syn.torch.cuda.synchronize()
    want_a, want_m = syn.want
    check_outputs(audit, margin, want_a, want_m if with_margin else np.full((LCAP, B), CANARY), "pitch %d" % pitch)
    syn.inputs_untouched()
    # the fleet has what the test is about
    got = [wg.ZmpAudit.from_buffer_copy(a) for a in want_a]
    assert want_a[0] == EMPTY and sum(a == REFUSED for a in want_a) == 3
    assert got[22].n_uncovered == LCAP and got[20].n_uncovered > 0 and got[23].n_uncovered == 40 and got[30].n_nonfinite == 2
    assert len({g.worst_sample // CH for g in got if g.status == 0 and g.worst_sample >= 0}) >= 3     # worst samples in several chunks


def test_batch_does_not_depend_on_the_batch(syn):
    """the first gait alone, and the first 64: the bytes they have in the fleet of 67"""
    for nb in (1, 64):
        audit, margin = syn.outputs()
        t = syn.torch
        x, y = syn.d_x[1:, :nb].contiguous(), syn.d_y[1:, :nb].contiguous()
        q, ts, te = syn.d_q[:nb].contiguous(), syn.d_ts[:nb].contiguous(), syn.d_te[:nb].contiguous()
        a = t.full((nb, ASZ), FILL_B, dtype=t.uint8, device="cuda")
        m = t.full((LCAP, nb), CANARY, dtype=t.float64, device="cuda")
        wg.zmp_audit_dev(nb, LCAP, syn.d_len.data_ptr(), syn.d_time.data_ptr(), x.data_ptr(), y.data_ptr(), nb, QC, q.data_ptr(),
                         ts.data_ptr(), te.data_ptr(), syn.d_count.data_ptr(), a.data_ptr(), m.data_ptr(), _stream())
        t.cuda.synchronize()
        assert [r.tobytes() for r in a.cpu().numpy()] == syn.want[0][:nb]
        assert m.cpu().numpy().tobytes() == np.ascontiguousarray(syn.want[1][:, :nb]).tobytes()


def test_host_side_errors(syn):
    lib = wg.lib()
    audit, margin = syn.outputs()
    px, py = syn.track_ptrs(B)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = [B, LCAP, p(syn.d_len), p(syn.d_time), C.c_void_p(px), C.c_void_p(py), B, QC, p(syn.d_q), p(syn.d_ts), p(syn.d_te), p(syn.d_count),
            p(audit[1:]), p(margin[1:]), None]
    for i, bad in ((0, -1), (1, 0), (2, None), (3, None), (4, None), (5, None), (6, B - 1), (7, 0), (8, None), (9, None), (10, None),
                   (11, None), (12, None)):
        args = list(good)
        args[i] = bad
        assert lib.wg_zmp_audit_dev(*args) == BAD, i
    args = list(good)
    args[0] = 0
    assert lib.wg_zmp_audit_dev(*args) == 0
    done = syn.torch.zeros(B, dtype=syn.torch.int32, device="cuda")
    good_app = good[:2] + [0, p(done)] + good[2:]
    for i, bad in ((2, -1), (3, None), (8, B - 1), (14, None)):
        args = list(good_app)
        args[i] = bad
        assert lib.wg_zmp_audit_append_dev(*args) == BAD, i
    syn.torch.cuda.synchronize()
    check_outputs(audit, margin, [PATTERN] * B, np.full((LCAP, B), CANARY), "refused calls wrote nothing")
    assert (done == 0).all()


# ---- 2. the append form ----------------------------------------------------------------------------------------------------
def cut_schedules(lens):
    """the "samples" and "ragged" schedules of tests/test_footcons_online_gpu.py: per call, the length every gait has reached"""
    per_gait = {"samples": [[1, CH - 1, CH, CH + 1, 2 * CH, lens[b]] for b in range(len(lens))],
                "ragged": [[1 + b, CH - 1 + b, CH + b, CH + 1 + b, 2 * CH + b, lens[b]] for b in range(len(lens))]}
    return {name: [np.array([min(c[i], lens[b]) for b, c in enumerate(cuts)], np.int32) for i in range(6)] for name, cuts in per_gait.items()}


def append(syn, state, lengths, first_sample=0, pitch=B, rc=0):
    audit, margin, done = state
    px, py = syn.track_ptrs(pitch)
    ln = dev(np.asarray(lengths, np.int32))
    got = wg.lib().wg_zmp_audit_append_dev(B, LCAP, int(first_sample), C.c_void_p(done.data_ptr()), C.c_void_p(ln.data_ptr()),
                                           C.c_void_p(syn.d_time.data_ptr()), C.c_void_p(px), C.c_void_p(py), pitch, QC,
                                           C.c_void_p(syn.d_q.data_ptr()), C.c_void_p(syn.d_ts.data_ptr()), C.c_void_p(syn.d_te.data_ptr()),
                                           C.c_void_p(syn.d_count.data_ptr()), C.c_void_p(audit[1:].data_ptr()),
                                           C.c_void_p(margin[1:].data_ptr()), _stream())
    assert got == rc, (got, wg.lib().wg_last_error())
    syn.torch.cuda.synchronize()


def batch_on(syn, lengths):
    """wg_zmp_audit_dev for these lengths: the audits as the device writes them"""
    audit, margin = syn.outputs()
    ln = dev(np.asarray(lengths, np.int32))
    px, py = syn.track_ptrs(B)
    wg.zmp_audit_dev(B, LCAP, ln.data_ptr(), syn.d_time.data_ptr(), px, py, B, QC, syn.d_q.data_ptr(), syn.d_ts.data_ptr(),
                     syn.d_te.data_ptr(), syn.d_count.data_ptr(), audit[1:].data_ptr(), margin[1:].data_ptr(), _stream())
    syn.torch.cuda.synchronize()
    return audit.cpu().numpy(), margin.cpu().numpy()


@pytest.mark.parametrize("first", ["zero", "min"])
@pytest.mark.parametrize("name", ["samples", "ragged"])
def test_every_cut_is_the_batch_call_on_the_prefix(syn, name, first):
    t = syn.torch
    lens = np.where(np.isin(np.arange(B), list(syn.refused)), LCAP, syn.lengths)       # the refusals have a test of their own
    lens = np.maximum(lens, 1)                                     # a gait that never begins: test_second_context_and_stream
    calls = cut_schedules(lens)[name]
    audit, margin = syn.outputs()
    done = t.zeros(B, dtype=t.int32, device="cuda")
    refused = {66: "count -2"}
    was = np.zeros(B, np.int32)
    for i, call in enumerate(calls):
        append(syn, (audit, margin, done), call, first_sample=int(np.delete(was, 66).min()) if first == "min" else 0)
        want_a, want_m = syn.expect(call, refused)
        check_outputs(audit, margin, want_a, want_m, "%s call %d" % (name, i))
        ba, bm = batch_on(syn, call)                               # and the batch call itself on the prefix
        assert audit.cpu().numpy().tobytes() == ba.tobytes(), (name, i)
        assert margin.cpu().numpy().tobytes() == bm.tobytes()
        d = done.cpu().numpy()
        assert np.array_equal(np.delete(d, 66), np.delete(call, 66)) and d[66] == 0, (name, i)
        was = call
    assert np.array_equal(was, lens)


def test_sit_outs_and_refusals(syn):
    t = syn.torch
    lens = np.full(B, LCAP, np.int32)
    L1, L2, L3 = np.full(B, CH + 3, np.int32), np.full(B, 2 * CH + 1, np.int32), lens
    first = CH
    clean = syn.outputs() + (t.zeros(B, dtype=t.int32, device="cuda"),)
    for L, fs in ((L1, 0), (L2, first), (L3, first)):
        append(syn, clean, L, first_sample=fs)
    state = syn.outputs() + (t.zeros(B, dtype=t.int32, device="cuda"),)
    append(syn, state, L1)
    before_a, before_m, before_d = (s.clone() for s in state)
    ln = L2.copy()
    ln[0] = L1[0]                                      # sits the call out
    ln[1] = -1                                         # a gait a producer refused
    ln[2] = LCAP + 1
    d = before_d.cpu().numpy().copy()
    d[3] = -1
    d[4] = ln[4] + 1
    d[5] = first - 1                                   # below first_sample
    state[2].copy_(t.from_numpy(d))
    state[0][1 + 6, 28:32] = t.from_numpy(np.frombuffer((-5).to_bytes(4, "little", signed=True), np.uint8).copy()).cuda()   # a status that is not WG_OK
    state[0][1 + 0, 0:8] = 0x5A                        # the sitting-out gait's bytes are not even read
    offenders = list(range(1, 7)) + [66]
    for rnd, (L, fs) in enumerate(((ln, first), (L3, min(first, int(d[5]))))):
        scribbled = state[0].clone()
        append(syn, state, L, first_sample=fs)
        a, m, dn = (s.cpu().numpy() for s in state)
        for b in offenders:
            want = scribbled[1 + b].cpu().numpy().tobytes()[:28] + BAD.to_bytes(4, "little", signed=True)
            assert a[1 + b].tobytes() == want, (rnd, b)             # the status and nothing else
            assert dn[b] == d[b], (rnd, b)                          # done unchanged
            assert m[1:-1, b].tobytes() == before_m.cpu().numpy()[1:-1, b].tobytes(), (rnd, b)
        if rnd == 0:
            assert a[1].tobytes() == scribbled[1].cpu().numpy().tobytes() and dn[0] == L1[0]      # gait 0 sat out: untouched
            assert m[1:-1, 0].tobytes() == before_m.cpu().numpy()[1:-1, 0].tobytes()
            state[0][1 + 0] = before_a[1 + 0]                       # give it back what it had: it walks on next round
    # the neighbours' bytes (and gait 0's, which sat a call out) are those of the run without the offenders
    a, m, dn = (s.cpu().numpy() for s in state)
    ca, cm, cd = (s.cpu().numpy() for s in clean)
    keep = [b for b in range(B) if b not in offenders]
    assert a[1:-1][keep].tobytes() == ca[1:-1][keep].tobytes()
    assert np.ascontiguousarray(m[:, keep]).tobytes() == np.ascontiguousarray(cm[:, keep]).tobytes() and np.array_equal(dn[keep], cd[keep])
    want_a, _ = syn.expect(lens, {66: ""})
    assert [a[1 + b].tobytes() for b in keep] == [want_a[b] for b in keep]
    # done[b] == 0 restarts a refused gait
    state[2][1:7] = 0
    append(syn, state, L3)
    a = state[0].cpu().numpy()
    assert [a[1 + b].tobytes() for b in range(1, 7)] == want_a[1:7]


# ---- 3. contexts and streams -----------------------------------------------------------------------------------------------
def test_second_context_and_stream(syn):
    t = syn.torch
    st = t.cuda.Stream()
    px, py = syn.track_ptrs(2 * B)
    with wg.Context(0) as ctx:
        audit, margin = syn.outputs()
        state = syn.outputs() + (t.zeros(B, dtype=t.int32, device="cuda"),)
        t.cuda.synchronize()
        args = (syn.d_time.data_ptr(), px, py, 2 * B, QC, syn.d_q.data_ptr(), syn.d_ts.data_ptr(), syn.d_te.data_ptr(), syn.d_count.data_ptr())
        wg.zmp_audit_dev(B, LCAP, syn.d_len.data_ptr(), *args, audit[1:].data_ptr(), margin[1:].data_ptr(), st.cuda_stream, ctx=ctx)
        wg.zmp_audit_append_dev(B, LCAP, 0, state[2].data_ptr(), syn.d_len.data_ptr(), *args, state[0][1:].data_ptr(),
                                state[1][1:].data_ptr(), st.cuda_stream, ctx=ctx)
        st.synchronize()
        check_outputs(audit, margin, *syn.want, "second context")
        want_a = [PATTERN if syn.lengths[b] == 0 else a for b, a in enumerate(syn.want[0])]
        check_outputs(state[0], state[1], want_a, syn.want[1], "second context, append")


def test_two_launches_of_one_context_on_two_streams_are_ordered(syn):
    """both launches keep their per-chunk partial results in the context's one buffer: the second is ordered behind the first"""
    t = syn.torch
    s1, s2 = t.cuda.Stream(), t.cuda.Stream()
    short = np.where(syn.lengths > 0, np.maximum(syn.lengths // 2, 1), syn.lengths).astype(np.int32)
    d_short = dev(short)
    want_short = syn.expect(short, {b: w for b, w in syn.refused.items() if b != 41})      # half of lcap + 1 is a length
    px, py = syn.track_ptrs(B)
    with wg.Context(0) as ctx:
        outs = [syn.outputs() for _ in range(6)]
        t.cuda.synchronize()
        for i, (audit, margin) in enumerate(outs):
            ln, st = (syn.d_len, s1) if i % 2 == 0 else (d_short, s2)
            wg.zmp_audit_dev(B, LCAP, ln.data_ptr(), syn.d_time.data_ptr(), px, py, B, QC, syn.d_q.data_ptr(), syn.d_ts.data_ptr(),
                             syn.d_te.data_ptr(), syn.d_count.data_ptr(), audit[1:].data_ptr(), margin[1:].data_ptr(), st.cuda_stream, ctx=ctx)
        s1.synchronize(); s2.synchronize()
        for i, (audit, margin) in enumerate(outs):
            check_outputs(audit, margin, *(syn.want if i % 2 == 0 else want_short), "launch %d" % i)


# ---- 4. chains -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kajita():
    """fleet70(0.7, 0.13) through wg_zmpdisc_full_batch_dev -> wg_foot_constraints_batch_dev, as tests/test_footcons_online_gpu.py"""
    wg.init(0)
    zm, steps, n_steps, init = fleet70(0.7, 0.13)
    f = Fleet(zm, steps, n_steps, init, SMAX, check_oracle=False)
    time = dev(times(f.lcap, zm.T))
    F = dict(B=f.B, lcap=f.lcap, ln=f.full["length"], time=time, lf=f.full["left"], lty=f.full["left_type"], rf=f.full["right"])
    return dict(f=f, time=time, Q=device_queues(F))


def audit_chain(nb, lcap, d_len, d_time, d_x, d_y, pitch, Q, qcap):
    import torch
    audit = torch.full((nb + 2, ASZ), FILL_B, dtype=torch.uint8, device="cuda")
    margin = torch.full((lcap + 2, nb), CANARY, dtype=torch.float64, device="cuda")
    wg.zmp_audit_dev(nb, lcap, d_len.data_ptr(), d_time.data_ptr(), d_x.data_ptr(), d_y.data_ptr(), pitch, qcap, Q["queues"].data_ptr(),
                     Q["ts"].data_ptr(), Q["te"].data_ptr(), Q["count"].data_ptr(), audit[1:].data_ptr(), margin[1:].data_ptr(), _stream())
    torch.cuda.synchronize()
    return audit, margin


def host_chain(nb, lcap, lengths, time, x, y, Q, qcap):
    return host_audits(time, x, y, Q["queues"].cpu().numpy(), Q["ts"].cpu().numpy(), Q["te"].cpu().numpy(), Q["count"].cpu().numpy(), qcap,
                       lengths, lcap)


def test_kajita_chain(kajita):
    f, Q = kajita["f"], kajita["Q"]
    audit, margin = audit_chain(BF, f.lcap, f.full["length"], kajita["time"], f.full["zmp_x"], f.full["zmp_y"], BF, Q, QCAP)
    want = host_chain(BF, f.lcap, f.lens, kajita["time"].cpu().numpy(), f.full["zmp_x"].cpu().numpy(), f.full["zmp_y"].cpu().numpy(), Q, QCAP)
    check_outputs(audit, margin, *want, "Kajita chain")
    got = [wg.ZmpAudit.from_buffer_copy(a) for a in want[0]]
    assert all(g.status == 0 and g.n_uncovered == 0 and g.n_nonfinite == 0 and g.worst_sample >= 0 for g in got)
    print("ZMP reference of the 70-gait fleet: least margin %.6f m, %d samples violated" % (min(g.margin for g in got), sum(g.n_violated for g in got)))


def test_morisawa_chain():
    import torch
    from test_morisawa_gpu import Dev
    wg.init(0)
    nb, smax = 5, 3
    f = mf.Fleet(nb, smax, 503)
    t0, lcap = mf.t_start_of(f.model), mf.lcap_for(f, False)
    d = Dev(f, wg.morisawa_block_bytes(smax) // 8, lcap)
    time = dev(times(lcap, f.model.T))
    o = {k: v[1:] for k, v in d.outs.items()}
    Q = dict(queues=torch.full((nb, QCAP * PSZ), FILL_B, dtype=torch.uint8, device="cuda"),
             ts=torch.full((nb, QCAP), CANARY, dtype=torch.float64, device="cuda"), te=torch.full((nb, QCAP), CANARY, dtype=torch.float64, device="cuda"),
             count=torch.full((nb,), -77, dtype=torch.int32, device="cuda"))
    ln = d.length[1:]
    # one stream, nothing in between
    wg.morisawa_walk_dev(f.model, nb, smax, *d.solve_args(f.model)[3:], t0, lcap, d.out_ptrs(), ln.data_ptr(), stream=_stream())
    wg.foot_constraints_batch_dev(nb, lcap, ln.data_ptr(), time.data_ptr(), o["left"].data_ptr(), o["left_type"].data_ptr(), o["right"].data_ptr(),
                                  *SOLE, QCAP, Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(), Q["count"].data_ptr(), _stream())
    audit, margin = audit_chain(nb, lcap, ln[:nb], time, o["zmp_x"][:lcap], o["zmp_y"][:lcap], nb, Q, QCAP)
    lens = ln[:nb].cpu().numpy()
    assert (d.status[1:-1] == 0).all() and (lens > 100).all() and (Q["count"].cpu().numpy() >= 3).all()
    want = host_chain(nb, lcap, lens, time.cpu().numpy(), o["zmp_x"][:lcap].cpu().numpy(), o["zmp_y"][:lcap].cpu().numpy(), Q, QCAP)
    check_outputs(audit, margin, *want, "Morisawa chain")
    got = [wg.ZmpAudit.from_buffer_copy(a) for a in want[0]]
    assert all(g.status == 0 and g.n_uncovered == 0 and g.n_violated == 0 and g.margin > 0.04 for g in got)    # the analytic ZMP stays well inside
    # the CoM's ground projection read in place: com_tm [lcap][4][B], pitch = 4 B
    com = o["com"]
    a2, m2 = audit_chain(nb, lcap, ln[:nb], time, com[:lcap], com[:lcap].reshape(-1)[nb:], 4 * nb, Q, QCAP)
    c = com[:lcap].cpu().numpy()
    want2 = host_chain(nb, lcap, lens, time.cpu().numpy(), c[:, 0], c[:, 1], Q, QCAP)
    check_outputs(a2, m2, *want2, "Morisawa chain, CoM")


def test_online_dimitrov_chain_ends_with_the_batch_audit(kajita):
    import torch
    f, Qfull = kajita["f"], kajita["Q"]
    want_audit, want_margin = audit_chain(BF, f.lcap, f.full["length"], kajita["time"], f.full["zmp_x"], f.full["zmp_y"], BF, Qfull, QCAP)
    w = Walk(f, ("zmp_x", "zmp_y", "left", "left_type", "right", "right_type"))
    Q = dict(queues=torch.full((BF, QCAP * PSZ), FILL_B, dtype=torch.uint8, device="cuda"),
             ts=torch.full((BF, QCAP), -7.25, dtype=torch.float64, device="cuda"), te=torch.full((BF, QCAP), -7.25, dtype=torch.float64, device="cuda"),
             count=torch.full((BF,), -77, dtype=torch.int32, device="cuda"), done=torch.zeros(BF, dtype=torch.int32, device="cuda"))
    audit = torch.full((BF + 2, ASZ), FILL_B, dtype=torch.uint8, device="cuda")
    margin = torch.full((f.lcap + 2, BF), CANARY, dtype=torch.float64, device="cuda")
    adone = torch.zeros(BF, dtype=torch.int32, device="cuda")
    done = np.zeros(BF, np.int32)
    calls = 0

    def grow(lens):
        nonlocal done, calls
        fs = int(done.min())
        wg.foot_constraints_append_dev(BF, w.lcap, fs, Q["done"].data_ptr(), w.buf["length"].data_ptr(), kajita["time"].data_ptr(),
                                       w.buf["left"].data_ptr(), w.buf["left_type"].data_ptr(), w.buf["right"].data_ptr(), *SOLE, QCAP,
                                       Q["queues"].data_ptr(), Q["ts"].data_ptr(), Q["te"].data_ptr(), Q["count"].data_ptr(), _stream())
        wg.zmp_audit_append_dev(BF, w.lcap, fs, adone.data_ptr(), w.buf["length"].data_ptr(), kajita["time"].data_ptr(),
                                w.buf["zmp_x"].data_ptr(), w.buf["zmp_y"].data_ptr(), BF, QCAP, Q["queues"].data_ptr(), Q["ts"].data_ptr(),
                                Q["te"].data_ptr(), Q["count"].data_ptr(), audit[1:].data_ptr(), margin[1:].data_ptr(), _stream())
        done = lens.copy()
        calls += 1

    def end_those_out_of_steps():
        out = (w.given == f.n_steps) & ~w.ended
        if out.any():
            grow(w.end(out.astype(np.int32)))

    grow(w.begin(np.full(BF, 2, np.int32)))
    end_those_out_of_steps()
    while not w.ended.all():
        grow(w.append(np.where(w.ended, 0, np.minimum(3, f.n_steps - w.given)).astype(np.int32)))
        end_those_out_of_steps()
    torch.cuda.synchronize()
    assert calls >= 4 and np.array_equal(adone.cpu().numpy(), f.lens)
    for k in ("queues", "ts", "te", "count"):
        assert torch.equal(Q[k], Qfull[k]), k
    assert torch.equal(audit, want_audit) and torch.equal(margin, want_margin)
