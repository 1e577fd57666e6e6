"""What following each gait's own queue costs a Dimitrov fleet (PB = 4096 gaits, PS = 8 steps, PT = 40 ticks, PK = 2 steps per
call, PLDP; straight walks as host/dimitrov_fleet.cpp draws them):
  (a) uniform  bin/dimitrov_fleet --online PK (walk pieces sized on the host: wg_dimitrov_walk_safe_ticks over the shortest gait
               still walking) against --online PK --follow (one wg_dimitrov_follow_dev behind every feeding), alternating PREPS = 3
               times in one session; "the walk alone" of each run, by events around the walk pieces / follow calls.  The checksums
               of all runs are asserted equal.  Expected: equal up to the spread, plus the follow call's rounds in which no gait goes.
  (b) ragged   the same two with --ragged (gait g walks S/2 .. S steps).  The total of ticks is the same: what follow buys is not
               throughput but a host that keeps no lengths and each gait's CoM at the earliest tick its own queue allows.
  empty round  one follow call of PROUNDS = 200 rounds on a fleet whose gaits all have their ticks (ticks == tick_cap): two
               near-empty launches per round, nothing else -- the price of a round the host could not know to be empty.
Host clock around work that ends in a device synchronise for the empty rounds; one JSON line at the end."""
import ctypes as C, importlib, json, os, re, subprocess, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
wg = importlib.import_module("jrl-walkgen_amd")
B = int(os.environ.get("PB", "4096")); S = int(os.environ.get("PS", "8")); TICKS = int(os.environ.get("PT", "40")); K = int(os.environ.get("PK", "2"))
REPS = int(os.environ.get("PREPS", "3")); ROUNDS = int(os.environ.get("PROUNDS", "200"))
EXE = os.path.join(ROOT, "jrl-walkgen_amd", "bin", "dimitrov_fleet")


def fleet_run(extra):
    r = subprocess.run([EXE, "--batch", str(B), "--steps", str(S), "--ticks", str(TICKS)] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"in ([0-9.]+) ms = .*the walk alone ([0-9.]+) ms = .*checksum ([0-9a-f]{16})", r.stdout)
    return float(m.group(1)), float(m.group(2)), m.group(3)


res = dict(B=B, steps=S, ticks=TICKS, steps_per_call=K)
for name, shape in (("uniform", []), ("ragged", ["--ragged"])):
    rows = {"walk": [], "follow": []}
    sums = {fleet_run(shape)[2]}
    for _ in range(REPS):                                       # alternating: both see the same machine state
        for key, extra in (("walk", []), ("follow", ["--follow"])):
            total, walk, h = fleet_run(shape + ["--online", str(K)] + extra)
            rows[key].append((total, walk)); sums.add(h)
    assert len(sums) == 1, sums                                 # whole sequence, walk pieces and follow: the same final states
    res[name] = {k: dict(total_ms=[t for t, _ in v], walk_alone_ms=[w for _, w in v]) for k, v in rows.items()}
    print("%s fleet, %d gaits x %d ticks fed %d steps per call: the walk alone %s ms with host-sized pieces, %s ms following"
          % (name, B, TICKS, K, res[name]["walk"]["walk_alone_ms"], res[name]["follow"]["walk_alone_ms"]))

# the empty round: every gait has its ticks, so every select wave decides and leaves, every tick block returns at once
wg.init(0)
wg.dimitrov_configure(wg.dimitrov_defaults())
z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")  # noqa: E731
QCAP, LCAP = 4, 4
q = z(B * QCAP * C.sizeof(wg.ZmpPolytope), torch.uint8); ts = z(B * QCAP, torch.float64); te = z(B * QCAP, torch.float64)
count = torch.ones(B, dtype=torch.int32, device="cuda"); have = torch.ones(B, dtype=torch.int32, device="cuda"); tm = z(LCAP, torch.float64)
clock = z(B, torch.float64); ticks = torch.full((B,), TICKS, dtype=torch.int32, device="cuda"); st = z(B * C.sizeof(wg.DimitrovState), torch.uint8)
sp = torch.cuda.current_stream().cuda_stream
p = lambda t: t.data_ptr()  # noqa: E731
call = lambda n: wg.dimitrov_follow_dev(B, QCAP, p(q), p(ts), p(te), p(count), LCAP, p(tm), p(have), None, wg.DIMITROV_FOLLOW_ALL_FINAL,  # noqa: E731
                                        p(clock), p(ticks), TICKS, n, p(st), None, None, 0, sp)
call(ROUNDS); torch.cuda.synchronize()
t0 = time.perf_counter(); call(ROUNDS); torch.cuda.synchronize()
res["empty_round_us"] = (time.perf_counter() - t0) / ROUNDS * 1e6
assert (ticks == TICKS).all() and not st.any()
print("a round in which no gait goes (B = %d): %.2f us" % (B, res["empty_round_us"]))
print(json.dumps(res))
