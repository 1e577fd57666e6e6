"""What the preview that follows each gait's own queue costs (PB = 4096 gaits, PS = 16 steps, the standard 1.6 s / 5 ms window, the
walks of host/kajita_fleet.cpp: every gait the model's support times, hence equal lengths -- the same work for every form):
  (a) batch    one wg_preview_run_batch_dev over the finished queues
  (b) follow   one wg_preview_follow_dev over the same finished queues (done = 0, length = L)
  (c) on line  the loop of kajita_fleet --online PK (PK = 2): after every begin / append / end the rows that became safe, with
               the batch call (the host knows the lengths: online_plan's arithmetic) against the follow call (it does not)
(a) and (b) alternate PREPS times in one session, as do the two loops of (c); the zmpdisc calls are outside the clocks of (c): the
queues are finished, only `length` is set to each call's prefix.  All forms are asserted to leave the same bytes.
Host clock around work that ends in a device synchronise; one JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); S = int(os.environ.get("PS", "16")); K = int(os.environ.get("PK", "2"))
REPS = int(os.environ.get("PREPS", "5"))
zm = wg.zmpdisc_defaults()
nl = int(zm.preview_time / zm.T)
g, F = wg.preview_gains(zm.T, 0.8078, zm.preview_time)
assert g.nl == nl
wg.preview_configure(g, F)
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


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


class Out:
    def __init__(self):
        self.st = torch.zeros(B, 8, dtype=torch.float64, device="cuda")
        self.com = torch.zeros(Lrun, 6, B, dtype=torch.float64, device="cuda")
        self.done = torch.zeros(B, dtype=torch.int32, device="cuda")

    def reset(self):
        self.st.zero_(); self.done.zero_()


def batch(o, row0, n):
    wg.preview_run_batch_dev(B, n, p(zx[row0:]), p(zy[row0:]), p(o.st), p(o.com[row0:]), None, True, sp)


def follow(o, length):
    wg.preview_follow_dev(B, L, p(length), p(o.done), p(zx), p(zy), p(o.st), p(o.com), None, True, sp)


# every gait has the model's support times, hence the same sample count after each call
cuts = [wg.zmpdisc_length_after(zm, first, min(n, S)) for n in range(2, S + K, K)] + [L]
lens = [dev(np.full(B, c, np.int32)) for c in cuts]


def loop_batch(o):
    done = 0
    for c in cuts:
        n = c - nl + 1 - done
        if n > 0:
            batch(o, done, n)
            done += n


def loop_follow(o):
    for length in lens:
        follow(o, length)


A, Fo, CA, CF = Out(), Out(), Out(), Out()
t = dict(a=[], b=[], c_batch=[], c_follow=[])
for rep in range(REPS + 1):                                    # the first pass warms up
    for o in (A, Fo, CA, CF):
        o.reset()
    r = (clock(lambda: batch(A, 0, Lrun)), clock(lambda: follow(Fo, ln)), clock(lambda: loop_batch(CA)), clock(lambda: loop_follow(CF)))
    if rep:
        for k, v in zip(t, r):
            t[k].append(round(v * 1e3, 4))
for o in (Fo, CA, CF):
    assert torch.equal(o.com, A.com) and torch.equal(o.st, A.st)   # the same trajectories, byte for byte
assert (Fo.done == Lrun).all() and (CF.done == Lrun).all()
med = {k: float(np.median(v)) for k, v in t.items()}
res = dict(B=B, steps=S, samples=L, nl=nl, calls=len(cuts), steps_per_call=K, ms=t,
           follow_over_batch=med["b"] / med["a"], online_follow_over_online_batch=med["c_follow"] / med["c_batch"],
           gait_steps_per_s=dict(batch=B * Lrun / med["a"] * 1e3, follow=B * Lrun / med["b"] * 1e3))
print("B = %d, %d samples, nl = %d: (a) batch %s ms, (b) follow %s ms, (c) %d calls of %d steps: batch %s ms, follow %s ms"
      % (B, L, nl, t["a"], t["b"], len(cuts), K, t["c_batch"], t["c_follow"]))
print(json.dumps(res))
