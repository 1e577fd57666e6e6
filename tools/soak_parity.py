"""Whole-batch parity soak (evidence, not a test): EVERY gait of the benchmark workload, advanced on the GPU exactly as bench.py
does it (two single ticks, then multi-tick launches with the velocity references staged on the device: tests/workload.py's
bench_plan_run), against the CPU checker (oracle/ with the portable trigonometry, the bit-exact partner of the kernels) on the
pool of tests/fleet_oracle.py -- at most 16 spawned processes that never load torch or the HIP runtime, queued first, working
while the GPU runs.  Final gait states compared word for word; with SOAK_VSCALE a NaN matches a NaN, nothing else is forgiven.
N = 16: 4096 gaits x 250 ticks; N = 32: 8192 gaits x 50 ticks.   python tools/soak_parity.py > profiles/<tag>_soak_parity.txt
The checker runs beside the product path here, as in tests/: nothing of it is measured or shipped."""
import importlib
import os
import sys
import time

import numpy as np

# SOAK_VSCALE=k: the benchmark's velocity references times k (both sides): at k = 3 .. 6 the QPs of many ticks are infeasible or
# inconsistent -- the failure paths of the tick, not only its walking
VSCALE = float(os.environ.get("SOAK_VSCALE", "1"))


def soak(N, B, n_ticks, pool, workers):
    import fleet_oracle as fo
    import workload as w
    wg = importlib.import_module("jrl-walkgen_amd")
    bench = w.bench_module()
    model = wg.model_defaults(); model.N = N
    n_seg = (n_ticks + bench.REDRAW_TICKS - 1) // bench.REDRAW_TICKS
    sz = fo.layout_of(wg)["state_size"]
    t0 = time.perf_counter()
    job = fo.submit(pool, fo.layout_of(wg), bytes(model), w.start_bytes(wg.gait_init, model), w.velocity_table(0, B, n_seg) * VSCALE,
                    bench.REDRAW_TICKS, n_ticks, nan_aware=VSCALE != 1.0)
    with wg.Context(0) as ctx:
        ctx.mpc_configure(model)
        t1 = time.perf_counter()
        fin, d, _ = w.bench_plan_run(ctx, model, B, n_ticks, n_ticks, bench, vel_scale=VSCALE)
        t_gpu = time.perf_counter() - t1
    t_said = time.perf_counter()
    while job.done()[0] < job.done()[1]:
        time.sleep(0.2)
        if time.perf_counter() - t_said > 60:                        # lost gaits run maxit iterations per tick: say that it is alive
            t_said = time.perf_counter()
            print("   ... CPU checker: %d of %d chunks" % job.done(), flush=True)
    cpu = job.result()
    t_cpu = time.perf_counter() - t0
    assert not any(r["torch"] or r["libs"] for r in cpu["workers"]), "a checker process holds torch or the HIP runtime"
    which = [r for r, _, _, _ in fo.record_mismatches(cpu["states"], b"".join(fin), sz, nan_aware=VSCALE != 1.0)]
    lost = fo.nan_gaits(cpu["states"], sz)
    if which:
        print("   differing gaits: %s%s" % (which[:24], " ..." if len(which) > 24 else ""), flush=True)
    print("N = %d%s: %d gaits x %d ticks = %d MPC ticks; gaits whose final state differs from the CPU checker's: %d%s; "
          "failed QPs %d; QL iterations mean %.1f max %d; n in %s; GPU %.2f s (launch plan %s), CPU checker %.1f s on %d processes"
          % (N, "" if VSCALE == 1.0 else " (references x %g)" % VSCALE, B, n_ticks, B * n_ticks, len(which),
             "" if not lost else " (%d gaits end with NaNs in their state, on both sides)" % lost, int((d[..., 0] != 0).sum()), float(d[..., 1].mean()), int(d[..., 1].max()),
             sorted(set(int(v) for v in np.unique(d[..., 3]))), t_gpu, bench.launch_plan(0, n_ticks), t_cpu, workers), flush=True)
    return len(which)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
    import fleet_oracle as fo
    import workload as w
    importlib.import_module("jrl-walkgen_amd").init(0)
    fo.build_oracle()
    workers = fo.pool_size(w.bench_module())
    # SOAK_LONG=1: four times the ticks at N = 16 and other horizons through the element view as well
    long_run = os.environ.get("SOAK_LONG") == "1"
    runs = [(16, 4096, 1000 if long_run else 250), (32, 8192, 50)]
    if long_run:
        runs += [(20, 2048, 100), (24, 2048, 80), (28, 2048, 60)]
    if os.environ.get("SOAK_ONLY"):                              # "N:B:T[,N:B:T...]": these runs instead of the standard ones
        runs = [tuple(int(v) for v in spec.split(":")) for spec in os.environ["SOAK_ONLY"].split(",")]
    with fo.make_pool(workers) as pool:
        bad = sum(soak(N, B, T, pool, workers) for N, B, T in runs)
    print("soak parity: %s" % ("PASS (bit-identical)" if bad == 0 else "FAIL"))
    return 1 if bad else 0


if __name__ == "__main__":                                       # the pool's processes import this file too: nothing above loads torch
    sys.exit(main())
