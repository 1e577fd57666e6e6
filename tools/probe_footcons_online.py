"""What the polytope queues of a Dimitrov fleet cost (PB = 4096 gaits, PS = 16 steps, straight walks as tools/probe_dimitrov_walk.py):
  batch    wg_foot_constraints_batch_dev on the whole feet trajectories, mean of 20 calls -- also with an older library
           (WG_LIB_PATH=...), for A/B runs of the whole-sequence path
  on line  the walk fed PK = 2 steps per call: the sum of the wg_foot_constraints_append_dev calls, against the sum of
           re-running the batch call on every growing prefix (what a fleet had to do without the append call); the final queues
           of both are asserted equal as bytes.  Skipped with a library that has no append call.
Host clock around work that ends in a device synchronise; one JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); S = int(os.environ.get("PS", "16")); K = int(os.environ.get("PK", "2")); QCAP = 64
REPS = int(os.environ.get("PREPS", "5"))
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
first = (wg.RelStep * S)(*[steps[i] for i in range(S)])
L = wg.zmpdisc_length(zm, first)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
d_steps = dev(np.frombuffer(steps, dtype=np.uint8).copy()); d_ns = dev(np.full(B, S, np.int32))
d_init = dev(np.tile(np.array([0.0, 0.095, 0.0, 0.0, -0.095, 0.0]), (B, 1)))
d_time = dev(np.cumsum(np.full(L, zm.T)) - zm.T)
lf = torch.zeros(L, 6, B, dtype=torch.float64, device="cuda"); rf = torch.zeros_like(lf)
lty = torch.zeros(L, B, dtype=torch.int32, device="cuda"); ln = torch.zeros(B, dtype=torch.int32, device="cuda")
stream = torch.cuda.Stream(); sp = stream.cuda_stream
p = lambda t: t.data_ptr()  # noqa: E731
assert wg.lib().wg_zmpdisc_full_batch_dev(C.byref(zm), B, S, p(d_steps), p(d_ns), p(d_init), L, None, None, None, None, p(lf), p(lty), p(rf),
                                          None, p(ln), sp) == 0
torch.cuda.synchronize()
assert (ln == L).all()
PSZ = C.sizeof(wg.ZmpPolytope)


def clock(fn, reps=1):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def outputs():
    return dict(q=torch.zeros(B, QCAP * PSZ, dtype=torch.uint8, device="cuda"), ts=torch.zeros(B, QCAP, dtype=torch.float64, device="cuda"),
                te=torch.zeros(B, QCAP, dtype=torch.float64, device="cuda"), cnt=torch.zeros(B, dtype=torch.int32, device="cuda"))


def batch(Q, length):
    wg.foot_constraints_batch_dev(B, L, p(length), p(d_time), p(lf), p(lty), p(rf), *SOLE, QCAP, p(Q["q"]), p(Q["ts"]), p(Q["te"]), p(Q["cnt"]), sp)


Qb = outputs()
batch(Qb, ln)
ms_batch = clock(lambda: batch(Qb, ln), 20) * 1e3
res = dict(lib=os.path.basename(wg.LIB_PATH) if hasattr(wg, "LIB_PATH") else "", B=B, steps=S, samples=L, batch_ms=ms_batch)
print("wg_foot_constraints_batch_dev, %d gaits x %d samples: %.4f ms" % (B, L, ms_batch))

if hasattr(wg.lib(), "wg_foot_constraints_append_dev"):
    # every gait has the model's support times, hence the same sample count after each call
    cuts = [wg.zmpdisc_length_after(zm, first, min(n, S)) for n in range(2, S + K, K)] + [L]
    lens = [dev(np.full(B, c, np.int32)) for c in cuts]
    Qa = outputs(); done = torch.zeros(B, dtype=torch.int32, device="cuda")

    def append(i):
        wg.foot_constraints_append_dev(B, L, cuts[i - 1] if i else 0, p(done), p(lens[i]), p(d_time), p(lf), p(lty), p(rf), *SOLE, QCAP,
                                       p(Qa["q"]), p(Qa["ts"]), p(Qa["te"]), p(Qa["cnt"]), sp)

    sums = []
    for rep in range(REPS + 1):                                # the first pass warms up
        done.zero_()
        a = sum(clock(lambda: append(i)) for i in range(len(cuts)))
        b = sum(clock(lambda: batch(Qb, lens[i])) for i in range(len(cuts)))
        if rep:
            sums.append((a * 1e3, b * 1e3))
    for k in Qa:
        assert torch.equal(Qa[k], Qb[k]), k                    # the same queues, byte for byte
    res.update(calls=len(cuts), steps_per_call=K, cuts=cuts, append_sum_ms=[round(a, 4) for a, _ in sums], rebatch_sum_ms=[round(b, 4) for _, b in sums])
    print("walk of %d steps fed %d per call (%d calls, prefixes %s): appends %s ms, batch call on every prefix %s ms"
          % (S, K, len(cuts), cuts, res["append_sum_ms"], res["rebatch_sum_ms"]))
print(json.dumps(res))
