"""Input families for the PLDP back-end outside the band the standard plans (tests/footplans.py) reach: more than 68 rows,
horizons below 16, empty polytopes, rows either side of row 64 (the second slot of a lane in the kernel's step-length pass),
an exact arg-min tie between rows 63 and 64, ragged batches.  Pure numpy geometry, no solver, no checker.  Polytopes are the tuples
of footplans.py -- (A rows x 2, B rows, centre, similar), A z + B >= 0 inside -- so Dimitrov.problem and polys_at work on them.

Row counts that repeat with period N keep the number of rows m of every window constant from tick to tick (a window is N
consecutive slots); the families that need a fixed layout (straddle, duplicate, ragged_batch) are built that way and must be walked
for at most len(slots) - N ticks (polys_at repeats the last slot beyond that)."""
import numpy as np

from footplans import polys_at  # noqa: F401  (re-exported: the families are read the way the standard plans are)

ROWS = (2, 3, 4, 6, 8)


def ngon(cx, cy, hx, hy, rows):
    """The polygon of `rows` edges around the ellipse of half-axes (hx, hy) at (cx, cy), inward unit normals.  `similar` is what
    FindSimilarConstraints emits (FootConstraintsAsLinearSystem.cpp:55-93): [0,0,-2,-2] for 4 rows, [0,0,0,-3,-3,-3] for 6 (rows
    i + rows/2 exactly antiparallel to row i), zeros otherwise.  rows = 0 is the empty polytope; 2 rows are the strip |x - cx| <= hx."""
    rows = int(rows)
    assert 0 <= rows <= 8
    if rows == 4:                                                      # footplans.box, row for row
        A = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
        B = np.array([-(cx - hx), -(cy - hy), cx + hx, cy + hy])
        return A, B, (cx, cy), np.array([0, 0, -2, -2])
    if rows == 2:
        return np.array([[1.0, 0.0], [-1.0, 0.0]]), np.array([-(cx - hx), cx + hx]), (cx, cy), np.zeros(2, dtype=int)
    th = 2.0 * np.pi * np.arange(rows) / max(rows, 1) + (np.pi / 2 if rows == 3 else 0.0)
    out = np.stack([np.cos(th), np.sin(th)], axis=1).reshape(rows, 2)  # outward normals
    if rows == 6:
        out[3:] = -out[:3]                                             # exact antiparallel pairs
    s = np.sqrt((hx * out[:, 0]) ** 2 + (hy * out[:, 1]) ** 2)         # support function of the ellipse
    A = -out
    B = out @ np.array([cx, cy]) + s                                   # -n.z + n.c + s >= 0
    sim = np.array([0, 0, 0, -3, -3, -3]) if rows == 6 else np.zeros(rows, dtype=int)
    return A, B, (cx, cy), sim


def track(rng, n_steps=8, hx=0.07, hy=0.03, ss=7, ds=1, tail=40):
    """The straight walk of footplans.plan as phases [(slots, cx, cy, hx, hy)]: a start double support (10 slots), n_steps single
    supports (ss slots) separated by double supports (ds slots: the box over both feet), a final double support."""
    ph = [(10, 0.0, 0.0, hx, hy + 0.095)]
    lx, ly, rx, ry = 0.0, 0.095, 0.0, -0.095
    left = bool(rng.integers(2))
    for _ in range(n_steps):
        cx, cy = (lx, ly) if left else (rx, ry)
        ph.append((ss, cx, cy, hx, hy))
        dx = rng.uniform(0.05, 0.25); dy = rng.uniform(-0.02, 0.02)
        if left:
            rx, ry = lx + dx, -0.095 + dy
        else:
            lx, ly = rx + dx, 0.095 + dy
        ph.append((ds, 0.5 * (lx + rx), 0.5 * (ly + ry), hx + 0.5 * abs(lx - rx), hy + 0.5 * abs(ly - ry)))
        left = not left
    ph.append((tail, 0.5 * (lx + rx), 0.5 * (ly + ry), hx + 0.5 * abs(lx - rx), hy + 0.095))
    return ph


def plan_rows(rng, rows, n_steps=8, **kw):
    """A walking plan with a fixed number of rows per instant: 8 (m = 8N, the tick's full mcap), 6 (every instant a reuse triple), ...
    One polytope object per phase, shared by its slots (like footplans.plan)."""
    slots = []
    for (k, cx, cy, hx, hy) in track(rng, n_steps, **kw):
        slots += [ngon(cx, cy, hx, hy, rows)] * k
    return slots


def plan_mixed(rng, n_steps=8, **kw):
    """seeded mix: every phase draws its row count from ROWS"""
    ph = track(rng, n_steps, **kw)
    slots = []
    for (k, cx, cy, hx, hy) in ph:
        slots += [ngon(cx, cy, hx, hy, int(rng.choice(ROWS)))] * k
    return slots


def plan_empty(rng, every=0, n_steps=8, **kw):
    """Polytopes with nrows = 0: all of them (every = 0: m = 0, the unconstrained minimiser) or all but each `every`-th slot, which
    keeps a polygon of 2, 3 or 4 rows (small m, most instants without a row, the first instant among them)."""
    slots = []
    i = 0
    for (k, cx, cy, hx, hy) in track(rng, n_steps, **kw):
        for _ in range(k):
            keep = every > 0 and i % every == every - 1
            slots.append(ngon(cx, cy, hx, hy, (2, 3, 4)[(i // every) % 3] if keep else 0))
            i += 1
    return slots


def _pattern_plan(rng, counts, n_slots, twin_at=None, n_steps=6):
    """slot i carries counts[i % len(counts)] rows, its geometry from the walk's track; twin_at: the pattern position whose box lists
    its last half-plane twice (similar all zero, so both twins are computed by the same arithmetic)"""
    geo = []
    for (k, cx, cy, hx, hy) in track(rng, n_steps, tail=n_slots):
        geo += [(cx, cy, hx, hy)] * k
    slots = []
    for i in range(n_slots):
        c = counts[i % len(counts)]
        if twin_at is not None and i % len(counts) == twin_at:
            A, B, ctr, _ = ngon(*geo[i], 4)
            slots.append((np.vstack([A, A[3:4]]), np.concatenate([B, B[3:4]]), ctr, np.zeros(5, dtype=int)))
        else:
            slots.append(ngon(*geo[i], c))
    return slots


STRADDLE_COUNTS = [4] * 13 + [3, 6, 6]       # rows before the last instant: 52 + 3 + 6 = 61 -> its six rows are 61..66
DUPLICATE_COUNTS = [4] * 15 + [5]            # the last instant: rows 60..64, the twins are its rows 3 and 4 = 63 and 64


def straddle(rng, n_slots=64):
    """N = 16: whenever the window starts on a multiple of 16 the last instant is a hexagon on rows 61..66, whose reuse pairs
    (61,64), (62,65), (63,66) cross the lane-slot boundary at row 64; m = 67 at every tick."""
    slots = _pattern_plan(rng, STRADDLE_COUNTS, n_slots)
    sim = np.concatenate([p[3] for p in polys_at(slots, 0, 16)])
    assert len(sim) == 67 and list(sim[61:67]) == [0, 0, 0, -3, -3, -3]
    assert [(r + sim[r], r) for r in (64, 65, 66)] == [(61, 64), (62, 65), (63, 66)]
    return slots


def duplicate(rng, n_slots=64):
    """N = 16: whenever the window starts on a multiple of 16 the last instant lists its half-plane y <= cy + hy twice, as rows 63
    and 64, with similar 0: an exact arg-min tie between lane 63's first-slot candidate and lane 0's second-slot candidate, and --
    once one twin is active -- a row whose A_i d is zero or rounding noise; m = 65 at every tick."""
    slots = _pattern_plan(rng, DUPLICATE_COUNTS, n_slots, twin_at=15)
    w = polys_at(slots, 0, 16)
    A = np.vstack([p[0] for p in w]); B = np.concatenate([p[1] for p in w]); sim = np.concatenate([p[3] for p in w])
    assert len(B) == 65 and np.array_equal(A[63], A[64]) and B[63] == B[64] and sim[63] == 0 and sim[64] == 0
    return slots


RAGGED_M = (0, 1, 2, 63, 64, 65, 96, 127, 128)


def ragged_batch(rng, mcap, N=16, n_slots=64):
    """one plan per m in RAGGED_M that fits mcap, rows spread over the N instants (period N: every window has m rows):
    -> (list of m, list of plans)"""
    ms = [m for m in RAGGED_M if m <= mcap]
    plans = []
    for m in ms:
        counts = [m // N + (1 if i < m % N else 0) for i in range(N)]
        assert sum(counts) == m and max(counts) <= 8
        plans.append(_pattern_plan(rng, counts, n_slots))
    return ms, plans


FAMILIES = ("std", "rows8", "rows6", "mixed", "straddle", "duplicate", "empty")


def fleet(name, B, seed=1000):
    """B plans of one family, gait g from its own generator seed + g -> (plans, tick offsets that de-synchronise the gaits)"""
    from footplans import plan
    rng = lambda g: np.random.default_rng(seed + g)  # noqa: E731
    steps = lambda g: 4 + g % 5  # noqa: E731
    make = {"std": lambda g: plan(rng(g), n_steps=steps(g)),
            "rows8": lambda g: plan_rows(rng(g), 8, n_steps=steps(g)),
            "rows6": lambda g: plan_rows(rng(g), 6, n_steps=steps(g)),
            "mixed": lambda g: plan_mixed(rng(g), n_steps=steps(g)),
            "straddle": lambda g: straddle(rng(g)),
            "duplicate": lambda g: duplicate(rng(g)),
            "empty": lambda g: plan_empty(rng(g), every=(0, 3, 5, 7)[g % 4])}[name]
    # the pattern families show their layout when a window starts on a multiple of 16: offsets 0, 4, 8, 12 reach it at several ticks
    offs = [(4 * g) % 16 for g in range(B)] if name in ("straddle", "duplicate") else [(3 * g) % 9 for g in range(B)]
    return [make(g) for g in range(B)], offs
