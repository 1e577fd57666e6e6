"""Herdt-2010 multi-tick launches with a model per gait against the configured run, at the bench's size (PB = 4096 gaits, N = 16,
the benchmark's gaits and references, PT = 100 ticks per launch with the references staged every 50):
  (a) configured  wg_mpc_run_sched_dev on a context configured with the default model (the parent's path; its kernels are unchanged)
  (b) fleet M=1   wg_mpc_run_fleet_dev, every gait bound to ONE block of that model (the same tick, the block cache-hot)
  (c) fleet M=B   wg_mpc_run_fleet_dev, a block per gait, every block that same model (the same arithmetic, B blocks read)
  (d) heights     a block per gait, com_height_qp 0.75 .. 0.88 (other QPs: for information)
Every repetition starts from the start pose, runs the control loop's first two ticks as single-tick launches (untimed) and times
one launch of PT ticks.  (a), (b), (c) must leave the same state checksum, and every variant the same one in every repetition.
The variants alternate PR (5) times in one session; min, median, max of each.
Then  (e) blocks  wg_mpc_blocks_batch_dev for M = PB models against a host loop of wg_mpc_block (same bytes).
One JSON line at the end."""
import ctypes as C, importlib, json, os, sys, time, zlib, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import workload as w  # noqa: E402
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); TICKS = int(os.environ.get("PT", "100")); REPS = int(os.environ.get("PR", "5"))
model = wg.model_defaults()
wg.mpc_configure(model)
NB = wg.mpc_block_bytes()
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
p = lambda t: t.data_ptr()  # noqa: E731
stream = torch.cuda.Stream(); sp = stream.cuda_stream
n_seg = (TICKS + 2 + w.REDRAW - 1) // w.REDRAW
vtab = dev(w.velocity_table(0, B, n_seg))                       # [seg, B, 3]
# the launch of ticks 2 .. TICKS + 1 takes its references from stretch (2 + k * REDRAW) // REDRAW: staged per period from its own t = 0
sched = dev(np.stack([w.velocity_table(0, B, n_seg)[min((2 + k * w.REDRAW) // w.REDRAW, n_seg - 1)] for k in range((TICKS + w.REDRAW - 1) // w.REDRAW)]))


def clock(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def blocks_of(models):
    M = len(models)
    arr = (wg.Model * M)(*models)
    d_m = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    blocks = torch.zeros(M, NB, dtype=torch.uint8, device="cuda"); status = torch.zeros(M, dtype=torch.int32, device="cuda")
    wg.mpc_blocks_batch_dev(M, p(d_m), p(blocks), p(status), sp)
    torch.cuda.synchronize()
    assert not status.cpu().numpy().any()
    return blocks, d_m, status


def with_height(h):
    m = wg.Model.from_buffer_copy(bytes(model)); m.com_height_qp = float(h)
    return m


heights = [with_height(h) for h in np.linspace(0.75, 0.88, B)]
one, _, _ = blocks_of([model]); same, _, _ = blocks_of([model] * B); spread, d_hm, d_hs = blocks_of(heights)
zeros = torch.zeros(B, dtype=torch.int32, device="cuda"); ident = torch.arange(B, dtype=torch.int32, device="cuda")
fleets = {"fleet M=1": wg.mpc_fleet(model, 1, p(one), p(zeros)), "fleet M=B": wg.mpc_fleet(model, B, p(same), p(ident)),
          "heights": wg.mpc_fleet(model, B, p(spread), p(ident))}


def head(st, fl):
    """the control loop's first two ticks, one launch each"""
    wg.mpc_set_velref_dev(B, p(st), p(vtab[0]), sp)
    for t in (0, 1):
        if fl is None:
            wg.mpc_tick_batch_dev(B, p(st), None, None, w.advance_calls(t), stream=sp)
        else:
            assert wg.mpc_tick_fleet_dev(B, fl, p(st), None, None, w.advance_calls(t), stream=sp) == 0


def run(st, fl):
    if fl is None:
        wg.mpc_run_sched_dev(B, p(st), TICKS, p(sched), w.REDRAW, 20, None, None, sp)
    else:
        assert wg.mpc_run_fleet_dev(B, fl, p(st), TICKS, 20, p(sched), w.REDRAW, None, None, sp) == 0


ways = {"configured": None}
ways.update(fleets)
result = dict(B=B, N=model.N, ticks=TICKS, reps=REPS, block_bytes=NB)
secs = {k: [] for k in ways}; sums = {k: [] for k in ways}
fresh = lambda: w.to_device(w.start_bytes(wg.gait_init, model), B)  # noqa: E731
for k, fl in ways.items():                                     # warm-up: code objects, the context's buffers
    st = fresh(); head(st, fl); run(st, fl)
    torch.cuda.synchronize()
for _ in range(REPS):                                          # alternating: a drift of the machine hits every variant alike
    for k, fl in ways.items():
        st = fresh(); head(st, fl)
        secs[k].append(clock(lambda: run(st, fl)))
        sums[k].append("%08x" % zlib.crc32(st.cpu().numpy().tobytes()))        # of EVERY repetition: a short time did the whole run
for k in ways:
    assert len(set(sums[k])) == 1, (k, sums[k], secs[k])
assert sums["configured"][0] == sums["fleet M=1"][0] == sums["fleet M=B"][0], sums
for k in ways:
    ms = np.array(secs[k]) / TICKS * 1e3
    result[k] = dict(ms_per_tick_min=ms.min(), ms_per_tick_median=float(np.median(ms)), ms_per_tick_max=ms.max(),
                     ms_per_tick=[round(float(x), 4) for x in ms], checksum=sums[k][0], checksums_equal_over_reps=True)
    print("%-11s ms per tick of %d gaits: min %.4f  median %.4f  max %.4f  (%.3f M ticks/s at the median), state checksum %s in "
          "each of %d repetitions: %s" % (k, B, ms.min(), np.median(ms), ms.max(), B / np.median(ms) / 1e3, sums[k][0], REPS,
                                          " ".join("%.4f" % x for x in ms)))

# ---- (e) the blocks: device against a host loop -------------------------------------------------------------------------------
make = lambda: wg.mpc_blocks_batch_dev(B, p(d_hm), p(spread), p(d_hs), sp)  # noqa: E731
make()
sec_dev = min(clock(make) for _ in range(REPS))
hb = np.zeros((B, NB), np.uint8)
t0 = time.perf_counter()
for m in range(B):
    assert wg.lib().wg_mpc_block(C.byref(heights[m]), hb[m].ctypes.data_as(C.c_void_p)) == 0
sec_host = time.perf_counter() - t0
assert spread.cpu().numpy().tobytes() == hb.tobytes()           # the same blocks, byte for byte
print("blocks of %d models (%d bytes each): device %.3f ms, host loop %.1f ms" % (B, NB, sec_dev * 1e3, sec_host * 1e3))
result["blocks"] = dict(M=B, device_ms=sec_dev * 1e3, host_loop_ms=sec_host * 1e3)
print(json.dumps(result))
