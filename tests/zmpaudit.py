"""Yardsticks of the walk audit (wg_zmp_audit, wg_zmp_audit_dev, wg_zmp_audit_append_dev), independent of the C++:

  audit_float   the rule of include/wg_mpc.h ("Walk audit") restated serially in plain Python floats -- IEEE doubles, the same
                order of operations, no FMA -- with a linear search for the FIRST entry that holds a sample's time;
  audit_mp      the same rule in 50-digit mpmath;
  polygon_margin_mp   the geometric truth: for a convex polygon given by its vertices, the signed distance of a point to the
                boundary lines, positive inside, the least over the edges -- from the vertices, not from the rows.

A queue is (polys, t_start, t_end, count, qcap): polys a ctypes array of wg.ZmpPolytope (only read field by field)."""
import math
import struct

import mpmath as mp

INF = float("inf")
SLACK = -1e-8                                  # ZMPConstrainedQPFastFormulation.cpp:322
OK, BAD = 0, -2
EMPTY = (INF, -1, -1, 0, 0, 0, OK)


def pack(a):
    """the 32 bytes of a wg_zmp_audit_t from (margin, worst_sample, worst_row, n_violated, n_uncovered, n_nonfinite, status)"""
    return struct.pack("<diiiiii", *a)


def find_entry(t, t_start, t_end, stored):
    for q in range(stored):
        if t_start[q] <= t <= t_end[q]:
            return q
    return -1


def sample_float(x, y, poly):
    """(margin, row, violated, uncovered, nonfinite) of one sample; poly None: no entry holds its time"""
    nonfinite = not (math.isfinite(x) and math.isfinite(y))
    uncovered = poly is None or not 1 <= poly.nrows <= 8
    if nonfinite or uncovered:
        return -INF, -1, True, uncovered, nonfinite
    m, row, violated = 0.0, -1, False
    for j in range(poly.nrows):
        a0, a1, b = float(poly.A[j][0]), float(poly.A[j][1]), float(poly.B[j])
        v = (a0 * x + a1 * y) + b
        nrm = math.sqrt(a0 * a0 + a1 * a1)
        if nrm == 0.0:                         # Python raises where IEEE says v / +0: NaN for 0 or NaN, else an infinity of v's sign
            d = float("nan") if v == 0.0 or math.isnan(v) else math.copysign(INF, v)
        else:
            d = v / nrm
        if not math.isfinite(d):
            d = -INF
        if j == 0 or d < m:
            m, row = d, j
        if v < SLACK:
            violated = True
    return m, row, violated, False, False


def audit_float(time, px, py, queue, first=0, n=None, audit=None, margin=None):
    """the audit of samples [first, n) folded into `audit` (a tuple as EMPTY; ignored when first == 0); returns (tuple, margins)"""
    polys, ts, te, count, qcap = queue
    n = len(time) if n is None else n
    a = list(EMPTY if first == 0 else audit)
    margin = [None] * n if margin is None else margin
    stored = min(count, qcap)
    for k in range(first, n):
        t = float(time[k])
        q = find_entry(t, ts, te, stored)
        m, row, viol, unc, nonf = sample_float(float(px[k]), float(py[k]), polys[q] if q >= 0 else None)
        margin[k] = m
        if m < a[0]:
            a[0], a[1], a[2] = m, k, row
        a[3] += viol; a[4] += unc; a[5] += nonf
    a[6] = OK
    return tuple(a), margin


def audit_mp(time, px, py, queue, n=None):
    """the same rule with 50 digits: (margin (mpf or -inf), worst_sample, worst_row, n_violated, n_uncovered, n_nonfinite), margins"""
    polys, ts, te, count, qcap = queue
    n = len(time) if n is None else n
    with mp.workdps(50):
        best, ws, wr, nv, nu, nn = mp.inf, -1, -1, 0, 0, 0
        margins = []
        for k in range(n):
            q = find_entry(float(time[k]), ts, te, min(count, qcap))
            x, y = float(px[k]), float(py[k])
            nonf = not (math.isfinite(x) and math.isfinite(y))
            unc = q < 0 or not 1 <= polys[q].nrows <= 8
            m, row, viol = -mp.inf, -1, nonf or unc
            if not viol:
                for j in range(polys[q].nrows):
                    a0, a1, b = mp.mpf(float(polys[q].A[j][0])), mp.mpf(float(polys[q].A[j][1])), mp.mpf(float(polys[q].B[j]))
                    v = (a0 * mp.mpf(x) + a1 * mp.mpf(y)) + b
                    nrm = mp.sqrt(a0 * a0 + a1 * a1)
                    d = v / nrm if nrm != 0 and mp.isfinite(v) and mp.isfinite(nrm) else -mp.inf
                    if j == 0 or d < m:
                        m, row = d, j
                    viol = viol or v < mp.mpf(SLACK)
            margins.append(m)
            if m < best:
                best, ws, wr = m, k, row
            nv += viol; nu += unc; nn += nonf
        return (best, ws, wr, nv, nu, nn), margins


# ---- geometry from vertices ------------------------------------------------------------------------------------------------
def sole_corners_mp(fx, fy, theta_deg, sole_w, sole_h, cx, cy):
    """the four corners of the sole minus its margins at (fx, fy), heading theta (degrees), exactly (50 digits)"""
    with mp.workdps(50):
        hw, hh = mp.mpf(sole_w) / 2 - mp.mpf(cx), mp.mpf(sole_h) / 2 - mp.mpf(cy)
        th = mp.mpf(theta_deg) * mp.pi / 180
        c, s = mp.cos(th), mp.sin(th)
        return [(mp.mpf(fx) + (sx * hw * c - sy * hh * s), mp.mpf(fy) + (sx * hw * s + sy * hh * c))
                for sx, sy in ((1, -1), (1, 1), (-1, 1), (-1, -1))]


def hull_mp(points):
    """convex hull, counter-clockwise (Andrew's monotone chain), of mpf points"""
    with mp.workdps(50):
        pts = sorted(set(points))
        cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])  # noqa: E731
        lower, upper = [], []
        for p in pts:
            while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
                lower.pop()
            lower.append(p)
        for p in reversed(pts):
            while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
                upper.pop()
            upper.append(p)
        return lower[:-1] + upper[:-1]


def polygon_margin_mp(vertices, x, y):
    """signed distance of (x, y) to the boundary lines of the counter-clockwise convex polygon: positive inside, least over edges"""
    with mp.workdps(50):
        best = mp.inf
        X, Y = mp.mpf(x), mp.mpf(y)
        for i, (px, py) in enumerate(vertices):
            qx, qy = vertices[(i + 1) % len(vertices)]
            ex, ey = qx - px, qy - py
            d = (ex * (Y - py) - ey * (X - px)) / mp.sqrt(ex * ex + ey * ey)
            best = min(best, d)
        return best
