"""Dimitrov-2008 fleet walks with a model per gait against the configured walk, at the bench's size (PB = 4096 gaits, N = 16,
PT = 100 ticks), in the modes PLDP and QLDANDLQ:
  (a) configured  wg_dimitrov_walk_dev on a context configured with the default model (the parent's path; its kernels are unchanged)
  (b) fleet M=1   wg_dimitrov_walk_fleet_dev, every gait bound to ONE block of that model (the same tick, the block cache-hot)
  (c) fleet M=B   wg_dimitrov_walk_fleet_dev, a block per gait, every block that same model (the same arithmetic, B blocks read)
  (d) heights     a block per gait, CoM heights 0.6 .. 0.9 (another walk: for information)
(a), (b), (c) must leave the same state checksum, and every variant the same one in every repetition.  The variants alternate PR (5) times in one session; min, median, max of each.
Then  (e) constants  wg_dimitrov_constants_batch_dev for M = PB models against a host loop of wg_dimitrov_constants (same bytes).
One JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, zlib, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); TICKS = int(os.environ.get("PT", "100")); S = int(os.environ.get("PS", "16")); QCAP = 64
REPS = int(os.environ.get("PR", "5"))
zm = wg.zmpdisc_defaults(); zm.t_single, zm.t_double = 0.7, 0.13
SOLE = (0.24, 0.138, 0.02, 0.02)
rng = np.random.default_rng(2008)
steps = (wg.RelStep * (B * S))()
for g in range(B):                                            # straight walks of varying step length, axis-aligned soles
    side = 1.0 if g & 1 else -1.0
    for i in range(S):
        ends = i == 0 or i == S - 1
        steps[g * S + i] = wg.RelStep(0.0 if ends else rng.uniform(0.1, 0.25), side * (0.105 if i == 0 else 0.21), 0.0, zm.t_single, 0.0, 1, 0)
        side = -side
L = wg.zmpdisc_length(zm, (wg.RelStep * S)(*[steps[i] for i in range(S)]))
base = wg.dimitrov_defaults(); N, T = base.N, base.T
assert L * zm.T > (TICKS + N) * T, "queues shorter than the run: raise PS"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
p = lambda t: t.data_ptr()  # noqa: E731
d_steps = dev(np.frombuffer(steps, dtype=np.uint8).copy()); d_ns = dev(np.full(B, S, np.int32))
d_init = dev(np.tile(np.array([0.0, 0.095, 0.0, 0.0, -0.095, 0.0]), (B, 1)))
d_time = dev(np.cumsum(np.full(L, zm.T)) - zm.T)
lf = torch.zeros(L, 6, B, dtype=torch.float64, device="cuda"); rf = torch.zeros_like(lf)
lty = torch.zeros(L, B, dtype=torch.int32, device="cuda"); ln = torch.zeros(B, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream(); sp = stream.cuda_stream
assert wg.lib().wg_zmpdisc_full_batch_dev(C.byref(zm), B, S, p(d_steps), p(d_ns), p(d_init), L, None, None, None, None, p(lf), p(lty), p(rf),
                                          None, p(ln), sp) == 0
PSZ, SSZ, NB = C.sizeof(wg.ZmpPolytope), C.sizeof(wg.DimitrovState), wg.dimitrov_constants_bytes()
dq = torch.zeros(B, QCAP * PSZ, dtype=torch.uint8, device="cuda"); dts = torch.zeros(B, QCAP, dtype=torch.float64, device="cuda")
dte = torch.zeros_like(dts); dcnt = torch.zeros(B, dtype=torch.int32, device="cuda")
wg.foot_constraints_batch_dev(B, L, p(ln), p(d_time), p(lf), p(lty), p(rf), *SOLE, QCAP, p(dq), p(dts), p(dte), p(dcnt), sp)
torch.cuda.synchronize()


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def fresh():
    st = np.zeros(B * SSZ, np.uint8).view(np.dtype([("xk", "f8", 6), ("pldp", "u1", C.sizeof(wg.PldpState)), ("n_removed", "i4"), ("starting", "i4")]))
    st["starting"] = 1
    return dev(st.view(np.uint8))


def blocks_of(model, heights):
    M = len(heights)
    blocks = torch.zeros(M, NB, dtype=torch.uint8, device="cuda"); status = torch.zeros(M, dtype=torch.int32, device="cuda")
    d_h = dev(np.asarray(heights, np.float64))
    wg.dimitrov_constants_batch_dev(M, model, p(d_h), None, None, p(blocks), p(status), sp)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    return blocks


result = dict(B=B, N=N, ticks=TICKS, reps=REPS, block_bytes=NB)
for solver, name in ((0, "PLDP"), (2, "QLDANDLQ")):
    model = wg.dimitrov_defaults(); model.solver = solver
    wg.dimitrov_configure(model)
    one = blocks_of(model, [model.com_height]); same = blocks_of(model, [model.com_height] * B)
    spread = blocks_of(model, np.linspace(0.6, 0.9, B))
    zeros = torch.zeros(B, dtype=torch.int32, device="cuda"); ident = torch.arange(B, dtype=torch.int32, device="cuda")
    fleets = dict(one=wg.dimitrov_fleet(model, 1, p(one), p(zeros)), same=wg.dimitrov_fleet(model, B, p(same), p(ident)),
                  spread=wg.dimitrov_fleet(model, B, p(spread), p(ident)))
    ways = {"configured": lambda st: wg.dimitrov_walk_dev(B, QCAP, p(dq), p(dts), p(dte), p(dcnt), 0.0, TICKS, p(st), None, None, 0, sp)}
    for key, label in (("one", "fleet M=1"), ("same", "fleet M=B"), ("spread", "heights")):
        ways[label] = (lambda st, fl=fleets[key]: wg.dimitrov_walk_fleet_dev(B, fl, QCAP, p(dq), p(dts), p(dte), p(dcnt), 0.0, TICKS, p(st),
                                                                            None, None, 0, sp))
    secs = {k: [] for k in ways}; sums = {k: [] for k in ways}
    for k, way in ways.items():                                # warm-up: code objects, the context's buffers
        st = fresh(); way(st)
        torch.cuda.synchronize()                               # the walk is asynchronous: its states live until it has ended
    for _ in range(REPS):                                      # alternating: a drift of the machine hits every variant alike
        for k, way in ways.items():
            st = fresh()
            secs[k].append(clock(lambda: way(st)))
            sums[k].append("%08x" % zlib.crc32(st.cpu().numpy().tobytes()))    # of EVERY repetition: a short time did the whole walk
    for k in ways:
        assert len(set(sums[k])) == 1, (k, sums[k], secs[k])
    assert sums["configured"][0] == sums["fleet M=1"][0] == sums["fleet M=B"][0], sums
    result[name] = {}
    for k in ways:
        ms = np.array(secs[k]) / TICKS * 1e3
        result[name][k] = dict(ms_per_tick_min=ms.min(), ms_per_tick_median=float(np.median(ms)), ms_per_tick_max=ms.max(),
                               ms_per_tick=[round(float(x), 4) for x in ms], checksum=sums[k][0], checksums_equal_over_reps=True)
        print("%-9s %-11s ms per tick of %d gaits: min %.4f  median %.4f  max %.4f  (%.3f M ticks/s at the median), state checksum %s in "
              "each of %d repetitions: %s" % (name, k, B, ms.min(), np.median(ms), ms.max(), B / np.median(ms) / 1e3, sums[k][0], REPS,
                                              " ".join("%.4f" % x for x in ms)))

# ---- (e) the constants: device against a host loop ---------------------------------------------------------------------------
model = wg.dimitrov_defaults()
h = np.linspace(0.6, 0.9, B); d_h = dev(h)
blocks = torch.zeros(B, NB, dtype=torch.uint8, device="cuda"); status = torch.zeros(B, dtype=torch.int32, device="cuda")
make = lambda: wg.dimitrov_constants_batch_dev(B, model, p(d_h), None, None, p(blocks), p(status), sp)  # noqa: E731
make()
sec_dev = min(clock(make) for _ in range(REPS))
hb = np.zeros((B, NB), np.uint8)
t0 = time.perf_counter()
for m in range(B):
    model.com_height = h[m]
    assert wg.lib().wg_dimitrov_constants(C.byref(model), hb[m].ctypes.data_as(C.c_void_p)) == 0
sec_host = time.perf_counter() - t0
assert blocks.cpu().numpy().tobytes() == hb.tobytes()         # the same blocks, byte for byte
print("constants of %d models (%d bytes each): device %.3f ms, host loop %.1f ms" % (B, NB, sec_dev * 1e3, sec_host * 1e3))
result["constants"] = dict(M=B, device_ms=sec_dev * 1e3, host_loop_ms=sec_host * 1e3)
print(json.dumps(result))
