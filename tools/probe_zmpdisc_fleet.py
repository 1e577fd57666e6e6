"""The producers with a model per gait against their one-model calls, at the fleet drivers' size (PB = 4096 gaits of PS = 6 steps,
every output of the walk resident), on one stream:
  (a) batch       wg_zmpdisc_full_batch_dev, one model (the parent's kernel, unchanged: the baseline)
  (b) fleet M=1   wg_zmpdisc_full_fleet_dev, every gait bound to that ONE model (the same walk; the model read from LDS, not SGPRs)
  (c) fleet M=B   wg_zmpdisc_full_fleet_dev, a model per gait, every one that same model (the same arithmetic, B models read)
  (d) robots      a model per gait, robots of size 0.8 .. 1.2: support times, step height, foot geometry (other walks: for information)
  (e) soles       wg_foot_constraints_batch_dev against wg_foot_constraints_fleet_dev with that sole for every gait, on (a)'s feet
(a), (b), (c) must leave the same checksum (ZMP queue, lengths, every 64th row of the left foot), (e)'s two forms the same queues,
and every variant the same checksum in every repetition.  The variants alternate PR (5) times in one session; min, median, max.
One JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, zlib, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); S = int(os.environ.get("PS", "6")); REPS = int(os.environ.get("PR", "5"))
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
raw = lambda ct: torch.frombuffer(bytearray(bytes(ct)), dtype=torch.uint8).cuda()  # noqa: E731
p = lambda t: t.data_ptr()  # noqa: E731
stream = torch.cuda.Stream(); sp = stream.cuda_stream

base = wg.zmpdisc_defaults()
base.t_single, base.t_double, base.omega = 0.7, 0.13, 2.0
base.foot_b, base.foot_h, base.foot_f = 0.1, 0.105, 0.13


def robot(s):
    """the base robot scaled by s: a single support out of a table of multiples of T, the lengths by s"""
    m = wg.ZmpDiscModel.from_buffer_copy(bytes(base))
    m.t_single = (0.6, 0.65, 0.7, 0.75, 0.8)[min(int((s - 0.8) / 0.4 * 5), 4)]
    m.step_height, m.foot_b, m.foot_h, m.foot_f = base.step_height * s, base.foot_b * s, base.foot_h * s, base.foot_f * s
    return m


rng = np.random.default_rng(2008)
steps = (wg.RelStep * (B * S))()
for g in range(B):
    side = 1.0 if g & 1 else -1.0
    for i in range(S):
        ends = i in (0, S - 1)
        steps[g * S + i] = wg.RelStep(0.0 if ends else rng.uniform(0.1, 0.25), side * (0.105 if i == 0 else 0.21), 0.0, base.t_single, 0.0, 1, 0)
        side = -side
robots = [robot(s) for s in np.linspace(0.8, 1.2, B)]
one_steps = (wg.RelStep * S)(*[steps[i] for i in range(S)])
lcap = max(wg.zmpdisc_length(m, one_steps) for m in [base] + robots[::64] + robots[-1:])
d_steps, d_ns = raw(steps), dev(np.full(B, S, np.int32))
d_feet = dev(np.tile([0.0, 0.095, 0.0, 0.0, -0.095, 0.0], (B, 1)))
f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")  # noqa: E731
i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")  # noqa: E731
O = dict(zmp_x=f64(lcap, B), zmp_y=f64(lcap, B), zmp_theta=f64(lcap, B), zmp_type=i32(lcap, B), left=f64(lcap, 6, B), left_type=i32(lcap, B),
         right=f64(lcap, 6, B), right_type=i32(lcap, B))
outs = [p(O[k]) for k in wg.ZMPDISC_OUTPUTS]
ln = i32(B)
d_one, d_same, d_robots = raw((wg.ZmpDiscModel * 1)(base)), raw((wg.ZmpDiscModel * B)(*[base] * B)), raw((wg.ZmpDiscModel * B)(*robots))
zeros = i32(B)
fleets = {"fleet M=1": wg.zmpdisc_fleet(base, 1, p(d_one), p(zeros)), "fleet M=B": wg.zmpdisc_fleet(base, B, p(d_same)),
          "robots": wg.zmpdisc_fleet(base, B, p(d_robots))}
lib = wg.lib()


def walk(fl):
    if fl is None:
        rc = lib.wg_zmpdisc_full_batch_dev(C.byref(base), B, S, p(d_steps), p(d_ns), p(d_feet), lcap, *outs, p(ln), sp)
    else:
        rc = lib.wg_zmpdisc_full_fleet_dev(C.byref(fl), B, S, p(d_steps), p(d_ns), p(d_feet), lcap, *outs, p(ln), sp)
    assert rc == 0, lib.wg_last_error()


def walk_sum():
    crc = 0
    for a in (O["zmp_x"], O["zmp_y"], ln, O["left"][::64]):
        crc = zlib.crc32(a.contiguous().cpu().numpy().tobytes(), crc)
    return "%08x" % crc


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def clear():
    for a in list(O.values()) + [ln]:
        a.zero_()
    torch.cuda.synchronize()                                   # torch's own stream: done before anything is launched on `stream`


ways = {"batch": None}
ways.update(fleets)
result = dict(B=B, steps=S, lcap=lcap, reps=REPS)
secs = {k: [] for k in ways}; sums = {k: [] for k in ways}
for fl in ways.values():                                       # warm-up: code objects
    walk(fl)
torch.cuda.synchronize()
for _ in range(REPS):                                          # alternating: a drift of the machine hits every variant alike
    for k, fl in ways.items():
        clear()
        secs[k].append(clock(lambda: walk(fl)))
        sums[k].append(walk_sum())                             # of EVERY repetition: a short time did the whole walk
for k in ways:
    assert len(set(sums[k])) == 1, (k, sums[k], secs[k])
assert sums["batch"][0] == sums["fleet M=1"][0] == sums["fleet M=B"][0], sums
med = {}
for k in ways:
    ms = np.array(secs[k]) * 1e3
    med[k] = float(np.median(ms))
    result[k] = dict(ms_min=ms.min(), ms_median=med[k], ms_max=ms.max(), ms=[round(float(x), 4) for x in ms], checksum=sums[k][0],
                     ratio_to_batch=med[k] / med["batch"])
    print("%-10s ms per walk of %d gaits: min %.4f  median %.4f  max %.4f  (x %.4f of batch), checksum %s in each of %d repetitions: %s"
          % (k, B, ms.min(), med[k], ms.max(), med[k] / med["batch"], sums[k][0], REPS, " ".join("%.4f" % x for x in ms)))

# ---- (e) the foot constraints, on the baseline's feet ----------------------------------------------------------------------------
clear(); walk(None); torch.cuda.synchronize()
SOLE = (0.24, 0.138, 0.02, 0.02)
qcap = max(2 * S + 8, 64)                                      # two polytopes per step, the rest phases either side (dimitrov_fleet's)
d_time = dev(np.arange(lcap) * base.T)
d_soles = dev(np.tile(SOLE, (B, 1)))
Q = dict(q=torch.zeros(B, qcap, C.sizeof(wg.ZmpPolytope), dtype=torch.uint8, device="cuda"), ts=f64(B, qcap), te=f64(B, qcap), count=i32(B))
qargs = (qcap, p(Q["q"]), p(Q["ts"]), p(Q["te"]), p(Q["count"]), sp)
feet = (B, lcap, p(ln), p(d_time), p(O["left"]), p(O["left_type"]), p(O["right"]))
forms = {"one sole": lambda: wg.foot_constraints_batch_dev(*feet, *SOLE, *qargs),
         "sole per gait": lambda: wg.foot_constraints_fleet_dev(*feet, p(d_soles), *qargs)}
fsecs = {k: [] for k in forms}; fsums = {k: [] for k in forms}
for fn in forms.values():
    fn()
torch.cuda.synchronize()
for _ in range(REPS):
    for k, fn in forms.items():
        for a in Q.values():
            a.zero_()
        fsecs[k].append(clock(fn))
        crc = 0
        for a in Q.values():
            crc = zlib.crc32(a.cpu().numpy().tobytes(), crc)
        fsums[k].append("%08x" % crc)
assert len(set(fsums["one sole"] + fsums["sole per gait"])) == 1, fsums
assert int(Q["count"].min()) > 0 and int(Q["count"].max()) <= qcap, (int(Q["count"].min()), int(Q["count"].max()))
for k in forms:
    ms = np.array(fsecs[k]) * 1e3
    result[k] = dict(ms_min=ms.min(), ms_median=float(np.median(ms)), ms_max=ms.max(), checksum=fsums[k][0])
    print("%-13s ms per %d queues: min %.4f  median %.4f  max %.4f, checksum %s in each of %d repetitions" %
          (k, B, ms.min(), np.median(ms), ms.max(), fsums[k][0], REPS))
print(json.dumps(result))
