"""The lock-step driver of the PLDP tests: B receding-horizon gaits solved tick by tick on the oracle (oracle/pldp_oracle.c) and,
where a GPU solve is given, on the GPU from the same inputs -- ret, iteration count, activation sequence, X and hot-start state
compared after every solve, the failed ones included -- plus the property gate against the reference-pinned QL oracle.
numpy + oraclelib only: the GPU side comes in as a callable."""
import collections

import numpy as np

import dimitrov as dv
import oraclelib as ol


def pack(dm, probs, mcap):
    B = len(probs); n = 2 * dm.N
    m = np.array([p["m"] for p in probs], dtype=np.int32)
    D = np.stack([p["D"] for p in probs])
    A = np.zeros((B, (mcap + 1) * n)); b = np.zeros((B, mcap)); sim = np.zeros((B, mcap), dtype=np.int32)
    for i, p in enumerate(probs):
        A[i, :p["A"].size] = p["A"]; b[i, :p["m"]] = p["b"]; sim[i, :p["m"]] = p["similar"]
    z = np.stack([p["zmpref"] for p in probs]); xk = np.stack([p["xk"] for p in probs])
    return m, D, A, b, z, xk, sim


def state_tuple(s):
    return (s.n_prev, list(s.prev_active[:s.n_prev]), list(s.prev_zmp), s.internal_time)


def same_state(a, b):
    """state_tuple equality, bit for bit on the doubles, a NaN matching a NaN (oraclelib.same_bits_nan_aware)"""
    return (a.n_prev == b.n_prev and list(a.prev_active[:a.n_prev]) == list(b.prev_active[:b.n_prev])
            and ol.same_bits_nan_aware(np.array(a.prev_zmp), np.array(b.prev_zmp))
            and ol.same_bits_nan_aware(np.array([a.internal_time]), np.array([b.internal_time])))


def ql_gate(dm, p, X, active, gate):
    """One solved problem against the reference-pinned QL oracle (oracle/ql_oracle.c == the reference's compiled qld.cpp):
    min 1/2 |v|^2 + D'v  s.t.  A v + b >= 0  has ONE optimum v*.  PLDP is a primal active-set method that never drops a
    constraint inside a solve (PLDPSolver.cpp:654-1007), so it ends either AT v* (projected gradient gone, multipliers of the
    right sign) or on a vertex it activated on the way and could not leave -- feasible, objective above the optimum.  Checked on
    EVERY solve: feasibility, f(X) >= f(v*) (up to what PLDP's own 1e-8 slack outside a face can buy, ComputeAlpha :613-621);
    where the KKT signs hold: X == v* to 2e-5 (1e-8 of slack over constraint rows of norm ~1e-3 -- 1e-9 on x is below what
    the method's own tolerance allows) and the objectives to 1e-9 relative."""
    m, n = p["m"], 2 * dm.N
    A = p["A"].reshape((n, m + 1)).T[:m]
    q = dict(n=n, m=m, me=0, mmax=m + 1, nmax=n, C=np.asfortranarray(np.eye(n)), d=p["D"].copy(),
             A=np.asfortranarray(np.vstack([A, np.zeros((1, n))])), b=np.concatenate([p["b"], [0.0]]),
             xl=np.full(n, -1e8), xu=np.full(n, 1e8))
    o = ol.oracle_ql(q)
    assert o["ifail"] == 0
    f = lambda z: 0.5 * z @ z + p["D"] @ z  # noqa: E731
    lam_sum = float(np.abs(o["u"][:m]).sum())
    assert (A @ X + p["b"]).min() > -5e-8
    gap = f(X) - f(o["x"])
    assert gap >= -5e-8 * lam_sum - 1e-9 * max(1.0, abs(f(X))), gap
    act = np.asarray(active, dtype=int)                        # PLDP's own active set, in activation order
    if len(act):
        lam, *_ = np.linalg.lstsq(A[act].T, X + p["D"], rcond=None)
        kkt = np.abs(A[act].T @ lam - (X + p["D"])).max() < 1e-9 and (lam > -1e-12).all()
    else:
        kkt = np.abs(X + p["D"]).max() < 1e-9
    gate["solves"] += 1
    if kkt:
        assert np.abs(X - o["x"]).max() < 2e-5 and abs(gap) <= 5e-8 * lam_sum + 1e-9 * max(1.0, abs(f(X)))
        gate["optimal"] += 1
    else:
        gate["stuck"] += 1
        gate["worst_gap"] = max(gate["worst_gap"], gap / max(1e-12, abs(f(o["x"]))))
        gate["worst_dx"] = max(gate["worst_dx"], float(np.abs(X - o["x"]).max()))


def new_gate():
    return dict(solves=0, optimal=0, stuck=0, worst_gap=0.0, worst_dx=0.0)


def summary(st):
    """one line of what a run recorded (solves, range of m, largest active set, exit codes)"""
    return ("solves %d, m %d..%d, largest active set %d, highest active row %d, both halves active in %d, iterations <= %d, exits %s"
            % (st["solves"], min(st["m"], default=-1), max(st["m"], default=-1), max(st["nact"], default=0), st["max_row"],
               st["both_halves"], max(st["iters"], default=0), dict(sorted(st["rets"].items()))))


def run_lockstep(dm, plans, n_ticks, offs=None, max_iter=0, mcap=ol.PLDP_MMAX, gate=None, gpu_solve=None, gpu_states=None,
                 on_solve=None):
    """plans: one slot list per gait (footplans / pldpgen), gait g read from tick offs[g] on.  gpu_solve(N, mcap, m, D, A, b, zmpref,
    xkyk, similar, n_removed, starting, states, max_iter=) -> dict(ret, n_iter, active, X) with gpu_states its state array
    (wg.pldp_solve_batch and a (wg.PldpState * B)()), or None: the oracle alone (the gate then runs on the oracle's solutions).
    A gait stops at its first non-zero exit, like the reference process.  on_solve(it, g, problem, oracle result) sees every solve."""
    B = len(plans)
    offs = offs if offs is not None else [0] * B
    M = ol.pldp_setup(dm.N, dm.iPu, dm.Px, dm.Pu)
    xk = [np.zeros(6) for _ in range(B)]
    st_o = [ol.PldpState() for _ in range(B)]
    alive = np.ones(B, dtype=bool)
    n_removed = np.zeros(B, dtype=np.int32); starting = np.ones(B, dtype=np.int32)
    stats = dict(solves=0, neg_alpha=0, iters=[], nact=[], m=[], rets=collections.Counter(), max_row=-1, both_halves=0)
    for it in range(n_ticks):
        probs = [dm.problem(xk[g], dv.polys_at(plans[g], it + offs[g], dm.N)) for g in range(B)]
        out = None
        if gpu_solve is not None:
            m, D, A, b, z, xkk, sim = pack(dm, probs, mcap)
            out = gpu_solve(dm.N, mcap, m, D, A, b, z, xkk, sim, n_removed, starting, gpu_states, max_iter=max_iter)
        for g in range(B):
            if not alive[g]:
                continue
            p = probs[g]
            o = ol.pldp_solve(M, st_o[g], p["D"], p["m"], p["A"], p["b"], p["zmpref"], p["xk"], p["similar"],
                              int(n_removed[g]), bool(starting[g]), max_iter=max_iter)
            if out is not None:
                assert out["ret"][g] == o["ret"], (it, g, out["ret"][g], o["ret"])
                assert out["n_iter"][g] == o["n_iter"], (it, g)
                assert np.array_equal(out["active"][g], o["active"]), (it, g, out["active"][g], o["active"])
                assert ol.same_bits_nan_aware(out["X"][g], o["X"]), (it, g, np.abs(out["X"][g] - o["X"]).max())
                assert same_state(gpu_states[g], st_o[g]), (it, g)
            act = o["active"]
            stats["solves"] += 1; stats["iters"].append(o["n_iter"]); stats["nact"].append(len(act)); stats["m"].append(p["m"])
            stats["rets"][o["ret"]] += 1
            if len(act):
                stats["max_row"] = max(stats["max_row"], int(act.max()))
                stats["both_halves"] += bool(act.min() < 64 <= act.max())
            if on_solve is not None:
                on_solve(it, g, p, o)
            if o["ret"] != 0:
                stats["neg_alpha"] += (o["ret"] == -2)
                alive[g] = False                            # the reference process would have exited here
                continue
            if gate is not None:
                ql_gate(dm, p, out["X"][g] if out is not None else o["X"], act, gate)
            xk[g] = dm.step(xk[g], o["X"])
        n_removed = np.array([p["first_rows"] for p in probs], dtype=np.int32)
        starting[:] = 0
    return stats
