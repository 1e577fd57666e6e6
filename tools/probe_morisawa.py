"""Morisawa-2007 analytic walks, the device against the host twins, at the fleet drivers' size (PB = 4096 gaits of PS = 7 steps, every
output resident, from 2 t_single as the reference's queue), on one stream:
  (a) walk         wg_morisawa_walk_dev: one wavefront per gait solves, a lane per gait samples; nothing leaves the device
  (b) solve        wg_morisawa_solve_dev alone
  (c) sample       wg_morisawa_sample_dev alone, on (b)'s blocks
  (d) host         a loop of wg_morisawa_solve + wg_morisawa_sample over the gaits, in chunks on the cores granted (threads: the twins
                   hold no lock and ctypes drops the interpreter's)
(a) and (d) must leave the same checksum (ZMP, CoM, lengths, every 64th row of both feet) -- the host's bytes are the kernel's --
and every variant the same checksum in every repetition.  The variants alternate PR (5) times in one session; min, median, max.
One JSON line at the end.
With --long: the long family (wg_morisawa_long_*) at S = 7, 14, 32 and 64 next to the short solve at 7 and 14; see long_probe.
With --resolve [--long]: the re-plan from a kept factor against the full solve of the same plans; see resolve_probe."""
import concurrent.futures as cf, ctypes as C, importlib, json, os, sys, time, zlib, numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd"); wg.init(0)
B = int(os.environ.get("PB", "4096")); S = int(os.environ.get("PS", "7")); REPS = int(os.environ.get("PR", "5"))
CORES = int(os.environ.get("OMP_NUM_THREADS", "0")) or len(os.sched_getaffinity(0))
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
raw = lambda ct: torch.frombuffer(bytearray(bytes(ct)), dtype=torch.uint8).cuda()  # noqa: E731
p = lambda t: t.data_ptr()  # noqa: E731
stream = torch.cuda.Stream(); sp = stream.cuda_stream



def long_probe():
    """--long: the long family (wg_morisawa_long_*, Z as a band) at S = 7, 14, 32 and 64 on one fleet of B gaits per size: the long
    solve and the long walk on the device, next to them at S = 7 and 14 the short solve of the same build on the same fleet, and the
    host loop (wg_morisawa_long_solve + _long_sample in chunks on the cores granted).  PR alternating repetitions, medians.  The long
    blocks of a chunk of gaits must be the host twin's bytes, and at S <= 14 the long walk's outputs the short walk's by value."""
    m = wg.morisawa_defaults()
    result = dict(B=B, reps=REPS, cores=CORES, sizes={})
    pool = cf.ThreadPoolExecutor(CORES)
    for S_ in (7, 14, 32, 64):
        rng = np.random.default_rng(2007 + S_)
        steps = (wg.RelStep * (B * S_))()
        for g in range(B):
            side = 1.0 if g & 1 else -1.0
            for i in range(S_):
                ends = i in (0, S_ - 1)
                steps[g * S_ + i] = wg.RelStep(0.0 if ends else rng.uniform(0.1, 0.25), side * (0.105 if i == 0 else 0.19),
                                               0.0 if ends else rng.uniform(-5.0, 5.0), 0.0, 0.0, 1, 0)
                side = -side
        n_steps = np.full(B, S_, np.int32)
        feet = np.tile([0.0, 0.09, 0.0, 0.0, -0.09, 0.0], (B, 1))
        com0 = np.tile([0.0316054587, 0.0, 0.7116911], (B, 1)); com0[:, 2] += np.linspace(0.0, 0.1, B)
        t0 = 2.0 * m.t_single
        lcap = wg.morisawa_long_length(m, S_, t0)
        words = wg.morisawa_long_block_bytes(S_) // 8
        d_steps, d_ns, d_feet, d_com0 = raw(steps), dev(n_steps), dev(feet), dev(com0)
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")  # noqa: E731
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")  # noqa: E731
        O = dict(zmp_x=f64(lcap, B), zmp_y=f64(lcap, B), com=f64(lcap, 4, B), left=f64(lcap, 6, B), left_type=i32(lcap, B),
                 right=f64(lcap, 6, B), right_type=i32(lcap, B))
        outs = {k: p(v) for k, v in O.items()}
        blocks, status, ln = f64(B, words), i32(B), i32(B)
        args = (B, S_, p(d_steps), p(d_ns), p(d_feet), p(d_com0))
        ways = {"long_walk": lambda: wg.morisawa_long_walk_dev(m, *args, p(blocks), p(status), t0, lcap, outs, p(ln), sp),
                "long_solve": lambda: wg.morisawa_long_solve_dev(m, *args, p(blocks), p(status), sp),
                "long_sample": lambda: wg.morisawa_long_sample_dev(B, S_, p(blocks), p(status), t0, m.T, lcap, outs, p(ln), sp)}
        if S_ <= wg.MORISAWA_MAX_STEPS:
            sblocks = f64(B, wg.morisawa_block_bytes(S_) // 8)
            ways["short_solve"] = lambda: wg.morisawa_solve_dev(m, *args, p(sblocks), p(status), sp)
            ways["short_walk"] = lambda: wg.morisawa_walk_dev(m, *args, p(sblocks), p(status), t0, lcap, outs, p(ln), sp)
        CH = 32
        step_bytes = bytes(steps)

        def host_chunk(lo, keep=None):
            hi = min(lo + CH, B)
            st = (wg.RelStep * ((hi - lo) * S_)).from_buffer_copy(step_bytes[lo * S_ * 48:hi * S_ * 48])
            blk, stat = wg.morisawa_long_solve(m, st, n_steps[lo:hi], feet[lo:hi], com0[lo:hi], S_)
            r = wg.morisawa_long_sample(blk, stat, S_, t0, m.T, lcap, want=("zmp_x", "zmp_y", "com", "left", "right"))
            if keep is not None:
                keep.update(blocks=blk, **r)

        # what is compared: the first chunk of gaits, host against device; at S <= 14 the long walk against the short walk
        first = {}
        host_chunk(0, first)
        ways["long_walk"](); torch.cuda.synchronize()
        assert int(status.abs().max()) == 0 and int(ln.min()) == int(ln.max()) == lcap
        assert blocks[:CH].cpu().numpy().tobytes() == first["blocks"].tobytes()
        for k in ("zmp_x", "zmp_y", "com", "left", "right"):
            assert O[k][..., :CH].cpu().numpy().tobytes() == np.ascontiguousarray(first[k]).tobytes(), k
        if "short_walk" in ways:
            keep = {k: v.clone() for k, v in O.items()}
            ways["short_walk"](); torch.cuda.synchronize()
            assert all(bool((keep[k] == O[k]).all()) for k in O)
        secs = {k: [] for k in list(ways) + ["host"]}
        for _ in range(REPS):                                      # alternating: a drift of the machine hits every variant alike
            for k in ways:
                if k == "long_sample":
                    ways["long_solve"](); torch.cuda.synchronize()
                secs[k].append(clock(ways[k]))
            t = time.perf_counter(); list(pool.map(host_chunk, range(0, B, CH))); secs["host"].append(time.perf_counter() - t)
        row = dict(lcap=lcap, block_bytes=words * 8)
        for k, v in secs.items():
            ms = np.array(v) * 1e3
            row[k] = dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()))
        result["sizes"][S_] = row
        print("S = %2d, %d gaits x %d samples, ms (median of %d): %s" % (S_, B, lcap, REPS, "  ".join("%s %.3f" % (k, row[k]["ms_median"]) for k in secs)))
        del O, blocks, outs
        torch.cuda.empty_cache()
    print(json.dumps(result))


def resolve_probe(lng):
    """--resolve: B plans of S steps on one model and one CoM height, (a) solved in full (wg_morisawa[_long]_solve_dev) and (b) re-planned
    from the kept factor of one solved block (wg_morisawa[_long]_resolve_dev, the block made beforehand and not timed), in one process on
    one stream.  S = 7 and 14 for the short family, 7, 14, 32 and 64 with --long.  A warm-up of each, then PR alternating repetitions:
    min, median, max.  Both must leave the same checksum (CRC-32 of all blocks) in every repetition: the re-plan's bytes are the
    solve's.  "faster" is said only where the re-plan's max lies below the solve's min."""
    fam = "morisawa_long_" if lng else "morisawa_"
    solve_dev, resolve_dev, block_bytes = (getattr(wg, fam + k) for k in ("solve_dev", "resolve_dev", "block_bytes"))
    m = wg.morisawa_defaults()
    result = dict(B=B, reps=REPS, family="long" if lng else "short", sizes={})
    for S_ in ((7, 14, 32, 64) if lng else (7, 14)):
        rng = np.random.default_rng(2007 + S_)
        steps = (wg.RelStep * (B * S_))()
        for g in range(B):
            side = 1.0 if g & 1 else -1.0
            for i in range(S_):
                ends = i in (0, S_ - 1)
                steps[g * S_ + i] = wg.RelStep(0.0 if ends else rng.uniform(0.1, 0.25), side * (0.105 if i == 0 else 0.19),
                                               0.0 if ends else rng.uniform(-5.0, 5.0), 0.0, 0.0, 1, 0)
                side = -side
        n_steps = np.full(B, S_, np.int32)
        feet = np.tile([0.0, 0.09, 0.0, 0.0, -0.09, 0.0], (B, 1))
        com0 = np.tile([0.0316054587, 0.0, 0.7116911], (B, 1)); com0[:, 0] += rng.uniform(-0.01, 0.01, B)
        words = block_bytes(S_) // 8
        d_steps, d_ns, d_feet, d_com0 = raw(steps), dev(n_steps), dev(feet), dev(com0)
        blocks = torch.zeros(B, words, dtype=torch.float64, device="cuda")
        factor = torch.zeros(1, words, dtype=torch.float64, device="cuda")
        status, fstatus = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        ways = {"solve": lambda: solve_dev(m, B, S_, p(d_steps), p(d_ns), p(d_feet), p(d_com0), p(blocks), p(status), sp),
                "resolve": lambda: resolve_dev(m, B, S_, p(factor), 1, None, p(d_steps), p(d_feet), p(d_com0), p(blocks), p(status), sp)}
        solve_dev(m, 1, S_, p(d_steps), p(d_ns), p(d_feet), p(d_com0), p(factor), p(fstatus), sp)       # gait 0's block: the factor
        for k in ways:                                               # warm-up: code objects, the LDS attribute
            ways[k]()
        torch.cuda.synchronize()
        secs = {k: [] for k in ways}; sums = {k: [] for k in ways}
        for _ in range(REPS):                                        # alternating: a drift of the machine hits both alike
            for k in ways:
                blocks.zero_(); status.fill_(-77); torch.cuda.synchronize()
                secs[k].append(clock(ways[k]))
                assert int(status.abs().max()) == 0 and int(fstatus[0]) == 0
                sums[k].append("%08x" % zlib.crc32(blocks.cpu().numpy().tobytes()))
        assert len(set(sums["solve"] + sums["resolve"])) == 1, sums
        row = dict(block_bytes=words * 8, checksum=sums["solve"][0])
        for k, v in secs.items():
            ms = np.array(v) * 1e3
            row[k] = dict(ms_min=float(ms.min()), ms_median=float(np.median(ms)), ms_max=float(ms.max()), ms=[round(float(x), 4) for x in ms])
            print("%-5s S = %2d %-7s ms per %d gaits: min %.3f  median %.3f  max %.3f, checksum %s in each of %d repetitions: %s"
                  % (result["family"], S_, k, B, ms.min(), np.median(ms), ms.max(), sums[k][0], REPS, " ".join("%.3f" % x for x in ms)))
        row["resolve_faster"] = row["resolve"]["ms_max"] < row["solve"]["ms_min"]
        row["solve_over_resolve_median"] = row["solve"]["ms_median"] / row["resolve"]["ms_median"]
        print("%-5s S = %2d the re-plan's max %s the solve's min; medians solve / re-plan = %.2f"
              % (result["family"], S_, "lies below" if row["resolve_faster"] else "does NOT lie below", row["solve_over_resolve_median"]))
        result["sizes"][S_] = row
        del blocks
        torch.cuda.empty_cache()
    print(json.dumps(result))


if "--resolve" in sys.argv or "--long" in sys.argv:
    def clock(fn):
        torch.cuda.synchronize(); t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t
    resolve_probe("--long" in sys.argv) if "--resolve" in sys.argv else long_probe()
    sys.exit(0)

m = wg.morisawa_defaults()
rng = np.random.default_rng(2007)
steps = (wg.RelStep * (B * S))()
for g in range(B):
    side = 1.0 if g & 1 else -1.0
    for i in range(S):
        ends = i in (0, S - 1)
        steps[g * S + i] = wg.RelStep(0.0 if ends else (0.2 if g == 0 else rng.uniform(0.1, 0.25)), side * (0.105 if i == 0 else 0.19),
                                      0.0 if ends or g == 0 else rng.uniform(-5.0, 5.0), 0.0, 0.0, 1, 0)
        side = -side
n_steps = np.full(B, S, np.int32)
feet = np.tile([0.0, 0.09, 0.0, 0.0, -0.09, 0.0], (B, 1))
com0 = np.tile([0.0316054587, 0.0, 0.7116911], (B, 1)); com0[:, 2] += np.linspace(0.0, 0.1, B)
t0 = 2.0 * m.t_single
lcap = wg.morisawa_length(m, S, t0)
words = wg.morisawa_block_bytes(S) // 8
d_steps, d_ns, d_feet, d_com0 = raw(steps), dev(n_steps), dev(feet), dev(com0)
f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device="cuda")  # noqa: E731
i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")  # noqa: E731
O = dict(zmp_x=f64(lcap, B), zmp_y=f64(lcap, B), com=f64(lcap, 4, B), left=f64(lcap, 6, B), left_type=i32(lcap, B), right=f64(lcap, 6, B),
         right_type=i32(lcap, B))
outs = {k: p(v) for k, v in O.items()}
blocks, status, ln = f64(B, words), i32(B), i32(B)


def checksum(zx, zy, com, length, left, right):
    crc = 0
    for a in (zx, zy, com, length, left[::64], right[::64]):
        crc = zlib.crc32(np.ascontiguousarray(a).tobytes(), crc)
    return "%08x" % crc


def dev_sum():
    h = lambda t: t.contiguous().cpu().numpy()  # noqa: E731
    return checksum(h(O["zmp_x"]), h(O["zmp_y"]), h(O["com"]), h(ln), h(O["left"]), h(O["right"]))


def clock(fn):
    torch.cuda.synchronize(); t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def clear(with_blocks=True):
    for a in list(O.values()) + [ln] + ([blocks, status] if with_blocks else []):
        a.zero_()
    torch.cuda.synchronize()                                   # torch's own stream: done before anything is launched on `stream`


solve_args = (B, S, p(d_steps), p(d_ns), p(d_feet), p(d_com0), p(blocks), p(status))
ways = {"walk": lambda: wg.morisawa_walk_dev(m, *solve_args, t0, lcap, outs, p(ln), sp),
        "solve": lambda: wg.morisawa_solve_dev(m, *solve_args, sp),
        "sample": lambda: wg.morisawa_sample_dev(B, S, p(blocks), p(status), t0, m.T, lcap, outs, p(ln), sp)}

# ---- the host loop: the gaits in chunks, one thread per core granted ----
H = dict(zmp_x=np.zeros((lcap, B)), zmp_y=np.zeros((lcap, B)), com=np.zeros((lcap, 4, B)), left=np.zeros((lcap, 6, B)), right=np.zeros((lcap, 6, B)),
         length=np.zeros(B, np.int32))
CHUNK = 32
step_bytes = bytes(steps)


def host_chunk(lo):
    hi = min(lo + CHUNK, B)
    st = (wg.RelStep * ((hi - lo) * S)).from_buffer_copy(step_bytes[lo * S * 48:hi * S * 48])
    blk, stat = wg.morisawa_solve(m, st, n_steps[lo:hi], feet[lo:hi], com0[lo:hi], S)
    r = wg.morisawa_sample(blk, stat, S, t0, m.T, lcap, want=("zmp_x", "zmp_y", "com", "left", "right"))
    for k in ("zmp_x", "zmp_y", "com", "left", "right"):
        H[k][..., lo:hi] = r[k]
    H["length"][lo:hi] = r["length"]


pool = cf.ThreadPoolExecutor(CORES)


def host_loop():
    list(pool.map(host_chunk, range(0, B, CHUNK)))


result = dict(B=B, steps=S, lcap=lcap, reps=REPS, cores=CORES, block_bytes=words * 8)
secs = {k: [] for k in list(ways) + ["host"]}; sums = {k: [] for k in secs}
ways["walk"](); torch.cuda.synchronize()                      # warm-up: code objects
for _ in range(REPS):                                          # alternating: a drift of the machine hits every variant alike
    for k in ("walk", "solve", "sample"):
        clear(with_blocks=k != "sample")                       # sample runs on the blocks solve has just left
        secs[k].append(clock(ways[k]))
        sums[k].append(dev_sum() if k != "solve" else "%08x" % zlib.crc32(blocks.cpu().numpy().tobytes()))
    for a in H.values():
        a[...] = 0
    t = time.perf_counter(); host_loop(); secs["host"].append(time.perf_counter() - t)
    sums["host"].append(checksum(H["zmp_x"], H["zmp_y"], H["com"], H["length"], H["left"], H["right"]))
for k in secs:
    assert len(set(sums[k])) == 1, (k, sums[k], secs[k])
assert sums["walk"][0] == sums["sample"][0] == sums["host"][0], sums
assert int(status.abs().max()) == 0 and int(ln.min()) == int(ln.max()) == lcap
med = {k: float(np.median(np.array(v) * 1e3)) for k, v in secs.items()}
for k in secs:
    ms = np.array(secs[k]) * 1e3
    result[k] = dict(ms_min=ms.min(), ms_median=med[k], ms_max=ms.max(), ms=[round(float(x), 4) for x in ms], checksum=sums[k][0])
    print("%-7s ms per fleet of %d gaits x %d samples: min %.3f  median %.3f  max %.3f, checksum %s in each of %d repetitions: %s"
          % (k, B, lcap, ms.min(), med[k], ms.max(), sums[k][0], REPS, " ".join("%.3f" % x for x in ms)))
gb = B * lcap * 152 / 1e9
result["host_over_walk"] = med["host"] / med["walk"]
result["sample_store_GBps"] = gb / (med["sample"] * 1e-3)
print("host loop on %d cores / device walk = %.1f; the sampler's %.3f GB of stores at %.0f GB/s" % (CORES, result["host_over_walk"], gb, result["sample_store_GBps"]))
print(json.dumps(result))
