"""Dimitrov-2008 fleet, step sequences to ticks, fed three ways at the bench's size (PB = 4096 gaits, N = 16, PT = 100 ticks):
  host    as callers had to write it before wg_foot_constraints_batch_dev / wg_dimitrov_walk_dev: feet copied back, host
          wg_foot_constraints per gait, per tick a host queue walk (numpy, vectorised over the fleet), upload of B x N polytopes,
          wg_dimitrov_tick_batch_dev
  select  queues built on the device; per tick wg_dimitrov_select_polys_dev + wg_dimitrov_tick_batch_dev
  walk    queues built on the device; ONE wg_dimitrov_walk_dev
Asserts the same checksum of the final states on all three; prints ticks/s of each (host clock around work that ends in a device
synchronise), the time of wg_foot_constraints_batch_dev alone against the host loop over the gaits, one JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, zlib, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); TICKS = int(os.environ.get("PT", "100")); S = int(os.environ.get("PS", "16")); QCAP = 64
model = wg.dimitrov_defaults(); model.solver = int(os.environ.get("PSOLVER", "0")); wg.dimitrov_configure(model); N, T = model.N, model.T
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
assert L * zm.T > (TICKS + N) * T, "queues shorter than the run: raise PS"
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
d_steps = dev(np.frombuffer(steps, dtype=np.uint8).copy()); d_ns = dev(np.full(B, S, np.int32))
d_init = dev(np.tile(np.array([0.0, 0.095, 0.0, 0.0, -0.095, 0.0]), (B, 1)))
tm = np.cumsum(np.full(L, zm.T)) - zm.T; d_time = dev(tm)
lf = torch.zeros(L, 6, B, dtype=torch.float64, device="cuda"); rf = torch.zeros_like(lf)
lty = torch.zeros(L, B, dtype=torch.int32, device="cuda"); ln = torch.zeros(B, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream(); sp = stream.cuda_stream
p = lambda t: t.data_ptr()  # noqa: E731
assert wg.lib().wg_zmpdisc_full_batch_dev(C.byref(zm), B, S, p(d_steps), p(d_ns), p(d_init), L, None, None, None, None, p(lf), p(lty), p(rf),
                                          None, p(ln), sp) == 0
torch.cuda.synchronize()
PT = np.dtype([("nrows", "i4"), ("pad", "i4"), ("similar", "i4", 8), ("A", "f8", (8, 2)), ("B", "f8", 8), ("centre", "f8", 2)])
PSZ, SSZ = C.sizeof(wg.ZmpPolytope), C.sizeof(wg.DimitrovState)
assert PT.itemsize == PSZ


def clock(fn, reps=1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


# ---- queues: device, then the host loop over the gaits -------------------------------------------------------------------------
dq = torch.zeros(B, QCAP * PSZ, dtype=torch.uint8, device="cuda"); dts = torch.zeros(B, QCAP, dtype=torch.float64, device="cuda")
dte = torch.zeros_like(dts); dcnt = torch.zeros(B, dtype=torch.int32, device="cuda")
build = lambda: wg.foot_constraints_batch_dev(B, L, p(ln), p(d_time), p(lf), p(lty), p(rf), *SOLE, QCAP, p(dq), p(dts), p(dte), p(dcnt), sp)  # noqa: E731
build(); sec_dev_build = clock(build, 20)
t0 = time.perf_counter()
h_lf = np.ascontiguousarray(lf.cpu().numpy().transpose(2, 0, 1)); h_rf = np.ascontiguousarray(rf.cpu().numpy().transpose(2, 0, 1))
h_lty = np.ascontiguousarray(lty.cpu().numpy().T)
sec_copy_back = time.perf_counter() - t0
hq = np.zeros((B, QCAP), PT); hts = np.zeros((B, QCAP)); hte = np.zeros((B, QCAP)); hcnt = np.zeros(B, np.int32)
vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
t0 = time.perf_counter()
for g in range(B):
    hcnt[g] = wg.lib().wg_foot_constraints(L, vp(tm), vp(h_lf[g]), vp(h_lty[g]), vp(h_rf[g]), *SOLE, QCAP, vp(hq[g]), vp(hts[g]), vp(hte[g]))
sec_host_build = time.perf_counter() - t0
assert hcnt.min() >= 3 and hcnt.max() <= QCAP
assert np.array_equal(dcnt.cpu().numpy(), hcnt) and dq.cpu().numpy().tobytes() == hq.tobytes()        # the same queues, byte for byte
print("queues of %d gaits x %d samples: device %.3f ms, host loop %.1f ms (+ %.1f ms to copy the feet back and transpose them)"
      % (B, L, sec_dev_build * 1e3, sec_host_build * 1e3, sec_copy_back * 1e3))


def fresh():
    st = np.zeros(B * SSZ, np.uint8).view(np.dtype([("xk", "f8", 6), ("pldp", "u1", C.sizeof(wg.PldpState)), ("n_removed", "i4"), ("starting", "i4")]))
    st["starting"] = 1
    return dev(st.view(np.uint8))


def host_select(t0):
    """BuildConstraintMatrices' walk for the whole fleet at once: [B, N] queue positions"""
    k = np.arange(QCAP)[None, :]
    hit = (hts <= t0) & (t0 <= hte) & (k < hcnt[:, None])
    assert hit.any(axis=1).all()
    q = hit.argmax(axis=1); rows = np.arange(B); sel = np.zeros((B, N), np.int64)
    for i in range(N):
        q = q + (t0 + i * T > hte[rows, q])
        assert (q < hcnt).all()
        sel[:, i] = q
    return sel


def way_host(st):
    t0 = 0.0
    for _ in range(TICKS):
        polys = dev(np.ascontiguousarray(hq[np.arange(B)[:, None], host_select(t0)]).view(np.uint8))
        assert wg.lib().wg_dimitrov_tick_batch_dev(B, p(polys), p(st), None, 0, sp) == 0
        stream.synchronize()                                   # the upload buffer is reused by the caller tick after tick
        t0 += T


dpolys = torch.zeros(B * N * PSZ, dtype=torch.uint8, device="cuda")


def way_select(st):
    t0 = 0.0
    for _ in range(TICKS):
        wg.dimitrov_select_polys_dev(B, QCAP, p(dq), p(dts), p(dte), p(dcnt), t0, p(dpolys), None, sp)
        wg.dimitrov_tick_batch_dev(B, p(dpolys), p(st), None, 0, sp)
        t0 += T


def way_walk(st):
    wg.dimitrov_walk_dev(B, QCAP, p(dq), p(dts), p(dte), p(dcnt), 0.0, TICKS, p(st), None, None, 0, sp)


res = {}
for name, way in (("host", way_host), ("select", way_select), ("walk", way_walk)):
    way(fresh())                                               # warm-up: code objects, the context's buffers
    best = None
    for _ in range(3):
        st = fresh()
        sec = clock(lambda: way(st))
        best = sec if best is None else min(best, sec)
    res[name] = dict(ticks_per_s=B * TICKS / best, ms_per_tick=best / TICKS * 1e3, checksum="%08x" % zlib.crc32(st.cpu().numpy().tobytes()))
    print("%-6s %.3f M ticks/s (%.3f ms per tick of %d gaits), state checksum %s" % (name, res[name]["ticks_per_s"] / 1e6, res[name]["ms_per_tick"], B, res[name]["checksum"]))
assert res["host"]["checksum"] == res["select"]["checksum"] == res["walk"]["checksum"], "the three ways disagree"
print(json.dumps(dict(B=B, N=N, ticks=TICKS, solver=model.solver, samples=L, queues_device_ms=sec_dev_build * 1e3, queues_host_loop_ms=sec_host_build * 1e3,
                      feet_copy_back_ms=sec_copy_back * 1e3, **{k: v for k, v in res.items()})))
