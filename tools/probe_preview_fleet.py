"""What gains per gait cost the stage-1 preview (PB = 4096 gaits, PS = 16 steps, the standard 1.6 s / 5 ms window nl = 320, the
walks of host/kajita_fleet.cpp: every gait the model's support times, hence equal lengths -- the same work for every form):
  (a) parent   wg_preview_run_batch_dev of the library named by PARENT_LIB (a build of the commit before the fleet forms), loaded
               next to this build's in the same process; left out when PARENT_LIB is not set
  (b) batch    the same call on this build: the same code, the no-regression check
  (c) fleet1   wg_preview_run_fleet_dev with one height for all gaits (asserted: the bytes of (b))
  (d) fleetB   wg_preview_run_fleet_dev with B distinct heights in [0.6, 0.9]
  (e) gains    wg_riccati_gains_batch_dev for the B heights of (d), against a host loop of B wg_riccati_gains calls
               (asserted: the same bits)
(a) .. (d) alternate PREPS times in one session after a warm-up pass, each repetition starting with another form; (e)'s two sides
alternate in a loop of their own behind them.  Host clock around work that ends in a device synchronise; medians and spreads
(max - min), one JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); S = int(os.environ.get("PS", "16")); REPS = int(os.environ.get("PREPS", "5"))
ZC = 0.8078
zm = wg.zmpdisc_defaults()
nl = int(zm.preview_time / zm.T)
g, F = wg.preview_gains(zm.T, ZC, zm.preview_time)
assert g.nl == nl
wg.preview_configure(g, F)
parent = None
if os.environ.get("PARENT_LIB"):
    parent = wg.bind(C.CDLL(os.environ["PARENT_LIB"]))                   # this header's signatures on what the parent exports
    assert not hasattr(parent, "wg_preview_run_fleet_dev"), "PARENT_LIB already has the fleet forms"
    assert parent.wg_init(0) == 0 and parent.wg_preview_configure(C.byref(g), F.ctypes.data) == 0
rng = np.random.default_rng(2003)
steps = (wg.RelStep * (B * S))()
for b in range(B):
    side = 1.0 if b & 1 else -1.0
    for i in range(S):
        ends = i == 0 or i == S - 1
        steps[b * S + i] = wg.RelStep(0.0 if ends else rng.uniform(0.1, 0.25), side * (0.105 if i == 0 else 0.21),
                                      0.0 if ends else rng.uniform(-5.0, 5.0), zm.t_single, zm.t_double, 1, 0)
        side = -side
first = (wg.RelStep * S)(*[steps[i] for i in range(S)])
L = wg.zmpdisc_length(zm, first)
Lrun = L - nl + 1
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
p = lambda t: t.data_ptr()  # noqa: E731
d_steps = dev(np.frombuffer(steps, dtype=np.uint8).copy()); d_ns = dev(np.full(B, S, np.int32))
d_init = dev(np.tile(np.array([0.0094903, 0.095, 0.0, 0.0094903, -0.095, 0.0]), (B, 1)))
zx = torch.zeros(L, B, dtype=torch.float64, device="cuda"); zy = torch.zeros_like(zx)
ln = torch.zeros(B, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream(); sp = stream.cuda_stream
assert wg.lib().wg_zmpdisc_batch_dev(C.byref(zm), B, S, p(d_steps), p(d_ns), p(d_init), L, p(zx), p(zy), p(ln), sp) == 0
torch.cuda.synchronize()
assert (ln == L).all()


class Gains:
    """zc, K_tm, F_tm, status on the device and the wg_preview_fleet_t over them; made by the kernel"""

    def __init__(self, zc):
        self.zc_h = np.ascontiguousarray(zc, dtype=np.float64)
        self.zc = dev(self.zc_h)
        self.K = torch.zeros(4, B, dtype=torch.float64, device="cuda"); self.F = torch.zeros(nl, B, dtype=torch.float64, device="cuda")
        self.status = torch.zeros(B, dtype=torch.int32, device="cuda")
        self.c = wg.preview_fleet(zm.T, nl, p(self.zc), p(self.K), p(self.F))
        self.make()
        torch.cuda.synchronize()
        assert (self.status == 0).all()

    def make(self):
        wg.riccati_gains_batch_dev(B, zm.T, p(self.zc), 1.0, 1e-6, nl, wg.RICCATI_WITHOUT_INITIALPOS, p(self.K), p(self.F), p(self.status), sp)


class Out:
    def __init__(self):
        self.st = torch.zeros(B, 8, dtype=torch.float64, device="cuda")
        self.com = torch.zeros(Lrun, 6, B, dtype=torch.float64, device="cuda")


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


one, many = Gains(np.full(B, ZC)), Gains(np.linspace(0.6, 0.9, B))
Kh = np.zeros((B, 4)); Fh = np.zeros((B, nl))


def host_loop():
    lib = wg.lib()
    for b in range(B):
        assert lib.wg_riccati_gains(zm.T, float(many.zc_h[b]), 1.0, 1e-6, nl, wg.RICCATI_WITHOUT_INITIALPOS, Kh[b].ctypes.data,
                                    Fh[b].ctypes.data) == 0


def run_parent(o):
    assert parent.wg_preview_run_batch_dev(B, Lrun, p(zx), p(zy), p(o.st), p(o.com), None, 1, sp) == 0


OA, OB, OC, OD = Out(), Out(), Out(), Out()
forms = dict(b=lambda: wg.preview_run_batch_dev(B, Lrun, p(zx), p(zy), p(OB.st), p(OB.com), None, True, sp),
             c=lambda: wg.preview_run_fleet_dev(B, Lrun, one.c, p(zx), p(zy), p(OC.st), p(OC.com), None, True, sp),
             d=lambda: wg.preview_run_fleet_dev(B, Lrun, many.c, p(zx), p(zy), p(OD.st), p(OD.com), None, True, sp))
if parent is not None:
    forms = dict(a=lambda: run_parent(OA), **forms)
gains = dict(e_device=many.make, e_host=host_loop)
t = {k: [] for k in list(forms) + list(gains)}
at_head = {k: [] for k in forms}                                 # the times a form clocked as the first of its repetition
names = list(forms)
# The preview forms alternate back to back, each repetition starting with another form: the one that follows an idle device runs
# slower than the ones behind it (seen with the host loop of (e) inside this alternation: 19 ms without device work in front of (a)),
# so no form keeps that place.  The gains alternate in a loop of their own behind it.
for rep in range(REPS + 1):                                    # the first pass warms up
    for o in (OA, OB, OC, OD):
        o.st.zero_()
    order = names[rep % len(names):] + names[:rep % len(names)]
    for pos, k in enumerate(order):
        v = clock(forms[k])
        if rep:
            t[k].append(round(v * 1e3, 4))
            if pos == 0:
                at_head[k].append(round(v * 1e3, 4))
for rep in range(REPS + 1):
    for k, fn in gains.items():
        v = clock(fn)
        if rep:
            t[k].append(round(v * 1e3, 4))
assert torch.equal(OC.com, OB.com) and torch.equal(OC.st, OB.st)   # one height for all: the configured call's bytes
if parent is not None:
    assert torch.equal(OA.com, OB.com) and torch.equal(OA.st, OB.st)
assert not torch.equal(OD.com, OB.com) and torch.isfinite(OD.com).all()
assert np.array_equal(many.K.cpu().numpy().T.view(np.uint64), Kh.view(np.uint64))
assert np.array_equal(many.F.cpu().numpy().T.view(np.uint64), Fh.view(np.uint64))
med = {k: float(np.median(v)) for k, v in t.items()}
spread = {k: round(max(v) - min(v), 4) for k, v in t.items()}
base = "a" if parent is not None else "b"
res = dict(B=B, steps=S, samples=L, nl=nl, reps=REPS, ms=t, first_of_its_repetition_ms=at_head, median_ms=med, spread_ms=spread, base=base,
           over_base={k: med[k] / med[base] for k in ("b", "c", "d")}, host_over_device_gains=med["e_host"] / med["e_device"],
           gait_steps_per_s={k: B * Lrun / med[k] * 1e3 for k in med if k in "abcd"})
for k in t:
    print("(%s) median %.4f ms, spread %.4f ms: %s" % (k, med[k], spread[k], t[k]))
print(json.dumps(res))
