"""What planning the steps on the device buys a fleet (PB = 4096 gaits): the first stage of an on-line Kajita walk,
  (a) device   wg_steps_plan_dev (support foot + an arc of the gait's own radius and angle, from commands resident on the device)
               -> wg_zmpdisc_begin_dev, one stream, nothing uploaded;
  (b) host     wg_steps_plan per gait on the host, the upload of steps [B][PSMAX] and n_steps [B], wg_zmpdisc_begin_dev;
and the plan kernel alone (events around PN = 50 back-to-back launches).  The steps both ways are asserted equal, byte
for byte; (a) and (b) alternate PREPS = 5 times in one session.  Host clock around work that ends in a device synchronise; one
JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); SMAX = int(os.environ.get("PSMAX", "16")); REPS = int(os.environ.get("PREPS", "5")); N = int(os.environ.get("PN", "50"))
m = wg.zmpdisc_defaults()
cmds = (wg.StepCmd * (B * 2))()
for g in range(B):                                            # 1 .. 9 steps on the arc: a ragged fleet
    foot = 1 if g & 1 else -1
    R = 0.4 + 0.05 * (g % 17)
    cmds[2 * g] = wg.StepCmd(wg.STEP_SUPPORT_FOOT, foot, (0.0, 0.0, 0.0))
    cmds[2 * g + 1] = wg.StepCmd(wg.STEP_ARC, -foot, (0.0, -R if g & 2 else R, float(np.degrees((g % 9 + 0.5) * 0.15 / R))))
n_cmds = np.full(B, 2, np.int32)
fresh = np.tile(np.array([1, 0, 0, 0], np.int32), (B, 1))
d_cmds = torch.from_numpy(np.frombuffer(cmds, dtype=np.uint8).copy()).cuda(); d_nc = torch.from_numpy(n_cmds).cuda()
d_stack = torch.from_numpy(fresh).cuda(); d_fresh = torch.from_numpy(fresh).cuda()
SB = C.sizeof(wg.RelStep)
d_steps = torch.zeros(B * SMAX * SB, dtype=torch.uint8, device="cuda"); d_ns = torch.zeros(B, dtype=torch.int32, device="cuda")
init = torch.from_numpy(np.tile(np.array([0.0, 0.095, 0.0, 0.0, -0.095, 0.0]), (B, 1))).cuda()
one = (wg.RelStep * SMAX)()
for i in range(SMAX):
    one[i] = wg.RelStep(0, 0, 0, m.t_single, m.t_double, 0, 0)
lcap = wg.zmpdisc_length_after(m, one, 10)                     # the longest gait: support foot + 9
zx = torch.zeros(lcap, B, dtype=torch.float64, device="cuda"); zy = torch.zeros_like(zx)
state = torch.zeros(B * wg.ZMPDISC_STATE_BYTES, dtype=torch.uint8, device="cuda"); d_len = torch.zeros(B, dtype=torch.int32, device="cuda")
sp = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()  # noqa: E731
outs = {"zmp_x": p(zx), "zmp_y": p(zy)}


def begin():
    wg.zmpdisc_begin_dev(m, B, SMAX, p(d_steps), p(d_ns), p(init), lcap, outs, p(state), p(d_len), sp)


def device():
    d_stack.copy_(d_fresh)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    wg.steps_plan_dev(B, 2, p(d_cmds), p(d_nc), m.t_single, m.t_double, p(d_stack), SMAX, p(d_steps), p(d_ns), sp)
    begin()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


h_steps = np.zeros((B, SMAX, SB), np.uint8); h_ns = np.zeros(B, np.int32)


def host():
    torch.cuda.synchronize(); t0 = time.perf_counter()
    lib, n = wg.lib(), C.c_int(0)
    for g in range(B):
        stack = wg.StepStack(1, 0, 0, 0)
        lib.wg_steps_plan(C.addressof(cmds) + 2 * g * C.sizeof(wg.StepCmd), 2, m.t_single, m.t_double, C.addressof(stack), SMAX,
                          h_steps[g].ctypes.data, C.addressof(n))
        h_ns[g] = n.value
    t1 = time.perf_counter()
    d_steps.copy_(torch.from_numpy(h_steps).reshape(-1)); d_ns.copy_(torch.from_numpy(h_ns))
    begin()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, t1 - t0


device(); dev_steps, dev_ns, dev_len = d_steps.cpu().numpy().reshape(B, SMAX, SB).copy(), d_ns.cpu().numpy().copy(), d_len.cpu().numpy().copy()
host()
assert np.array_equal(dev_ns, h_ns) and np.array_equal(d_len.cpu().numpy(), dev_len) and dev_len.min() > 0
for g in range(B):
    assert np.array_equal(dev_steps[g, :dev_ns[g]], h_steps[g, :h_ns[g]]), g
rows = {"device_ms": [], "host_ms": [], "host_plan_alone_ms": []}
for _ in range(REPS):                                          # alternating: both see the same machine state
    rows["device_ms"].append(device() * 1e3)
    t, tp = host()
    rows["host_ms"].append(t * 1e3); rows["host_plan_alone_ms"].append(tp * 1e3)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(N):
    wg.steps_plan_dev(B, 2, p(d_cmds), p(d_nc), m.t_single, m.t_double, p(d_stack), SMAX, p(d_steps), p(d_ns), sp)
e1.record(); torch.cuda.synchronize()
res = dict(B=B, smax=SMAX, steps=int(dev_ns.sum()), plan_kernel_us=e0.elapsed_time(e1) / N * 1e3, **rows)
print("B = %d gaits, %d steps: plan + begin on the device %s ms; host plan + upload + begin %s ms (the host plan alone %s ms); the plan "
      "kernel alone %.1f us a launch" % (B, res["steps"], ["%.2f" % v for v in rows["device_ms"]], ["%.2f" % v for v in rows["host_ms"]],
                                         ["%.2f" % v for v in rows["host_plan_alone_ms"]], res["plan_kernel_us"]))
print(json.dumps(res))
