"""Seeded wg_model_t values and velocity references for the model sweeps (test infrastructure, no tests in this file).

tests/test_models_oracle.py runs what this module generates on the portable-trig oracle alone (CPU) and asserts that the
sweep covers what it is meant to cover; tests/test_models_gpu.py runs the same models and gaits through the tick kernels
and compares bytes.  Nothing here loads the product library or touches the GPU: the binding is imported for its POD
layouts only, the start state comes from the oracle's wgo_gait_init (byte-identical to wg_gait_init: both memset the
struct and write the same fields from the same arguments).

A model is VALID here when the tick is defined for it and stays finite:
  * T / Tctrl == 20 and t_double == T (the ABI's cadence);
  * the CoP polygon is not empty (margins below half the sole);
  * t_single < step_period and t_single <= 8 T: the swing polynomials are laid out over 0.9 t_single - (time passed), and
    the feet are interpolated while time + 1.5 T < time_limit, which leaves 0.5 T - 0.05 t_single of the swing -- positive
    only below 10 T (the reference's 0.7 s at T = 0.1 s);
  * the horizon previews at most four steps (max_previewed_steps below; the kernels hold kSMax = 4).

Previewed steps.  SupportFSM::set_support_state changes the previewed support at the first instant pi with
time + 1e-6 + pi T >= time_limit, and every change sets time_limit = time + pi T + step_period - T / 10.  Two changes are
therefore k = ceil((step_period - T / 10 - 1e-6) / T) instants apart.  A change at pi = 1 does not count as a step
(`if (pi != 1) ++StepNumber`) and a change at pi = 0 is the current support's, so the earliest counted change is at
pi = 2 and the most a horizon of N instants can hold is 1 + floor((N - 2) / k)."""
import ctypes as C
import importlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workload as w  # noqa: E402

_wg = importlib.import_module("jrl-walkgen_amd")                # POD layouts only
Model, GaitState, TickOut = _wg.Model, _wg.GaitState, _wg.TickOut

S_MAX = 4                                                       # kSMax of the tick kernels
FLAG_NO_STOP_CENTERING = 1
# descending; 0.75, 0.65, ... are not multiples of T = 0.1
STEP_PERIOD_GRID = (2.0, 1.6, 1.2, 1.0, 0.9, 0.8, 0.75, 0.7, 0.65, 0.6, 0.55, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25, 0.2)
HIP_VMAX_ROBOT = 3.5                                            # rad/s: the kinematic robot of host/test_herdt2010_robot.cpp


# ----------------------------------------------------------------------------------------------------------------- models
def defaults(N=16, T=0.1):
    """the oracle's wgo_model_defaults (== wg_model_defaults) at horizon N and sampling period T"""
    import oraclelib as ol
    m = Model()
    ol.oracle().wgo_model_defaults(C.byref(m))
    m.N = N; m.T = T; m.Tctrl = T / 20.0; m.t_double = T
    return m


def copy_model(m):
    return Model.from_buffer_copy(bytes(m))


def step_gap(T, step_period):
    """previewed instants between two support changes (module docstring), never more than the FSM's own figure: the
    1e-9 guards the quotient's rounding"""
    return max(1, int(math.ceil((step_period - T / 10.0 - 1e-6) / T - 1e-9)))


def max_previewed_steps(N, T, step_period):
    return 1 + (N - 2) // step_gap(T, step_period)


def compact_view(m):
    """the model takes the compact view (N = 16, at most two previewed steps)"""
    return m.N == 16 and m.N * m.T <= 2.0 * m.step_period + 1e-12


def step_periods_for(N, T=0.1, lo=0.0, hi=1.2):
    """the grid values in [lo, hi] a horizon of N instants can preview within S_MAX steps"""
    return [p for p in STEP_PERIOD_GRID if lo <= p <= hi and max_previewed_steps(N, T, p) <= S_MAX]


def set_step_period(m, step_period, frac=1.0):
    """step_period with the swing time that goes with it: the default's t_single = step_period - t_double, capped at 8 T
    (module docstring), times frac"""
    m.step_period = step_period
    m.t_single = min(step_period - m.t_double, 8.0 * m.T) * frac


def random_model(seed, N=16, T=0.1, step_periods=None):
    """one valid model, every field but N / T / Tctrl / t_double drawn around the default"""
    rng = np.random.default_rng([seed, N])
    d = defaults(N, T)
    m = defaults(N, T)
    m.com_height_qp = rng.uniform(0.6, 1.0)
    m.alpha, m.beta, m.gamma = (getattr(d, k) * 10.0 ** rng.uniform(-1, 1) for k in ("alpha", "beta", "gamma"))
    m.sole_w = d.sole_w * rng.uniform(0.7, 1.3); m.sole_h = d.sole_h * rng.uniform(0.7, 1.3)
    m.margin_x = rng.uniform(0.0, 0.95) * 0.5 * m.sole_w; m.margin_y = rng.uniform(0.0, 0.95) * 0.5 * m.sole_h
    m.ds_feet_distance = rng.uniform(0.16, 0.26); m.feet_distance = rng.uniform(0.16, 0.26)
    deg = math.pi / 180.0
    m.hip_l_lo, m.hip_r_lo = -rng.uniform(6, 20) * deg, -rng.uniform(6, 20) * deg
    m.hip_l_hi, m.hip_r_hi = rng.uniform(6, 25) * deg, rng.uniform(6, 25) * deg
    m.hip_vmax = (0.0, HIP_VMAX_ROBOT)[int(rng.integers(2))] * 2.0 ** rng.uniform(-1, 1)       # the default is 0: feet never turn
    m.hip_amax = d.hip_amax * 2.0 ** rng.uniform(-1, 1)
    m.feet_cross_max = d.feet_cross_max * 2.0 ** rng.uniform(-1, 1)
    grid = step_periods if step_periods is not None else step_periods_for(N, T)
    set_step_period(m, grid[int(rng.integers(len(grid)))], (1.0, rng.uniform(0.7, 1.0))[int(rng.integers(2))])
    m.ds_period = (1e9, rng.uniform(0.3, 1.5))[int(rng.integers(2))]
    m.dsss_period = rng.uniform(0.4, 1.2)
    m.step_height = rng.uniform(0.03, 0.08)
    m.flags = int(rng.integers(2)) * FLAG_NO_STOP_CENTERING
    check_valid(m)
    return m


def check_valid(m):
    assert int(m.T / m.Tctrl) == 20 and m.t_double == m.T
    assert 0.0 <= m.margin_x < 0.5 * m.sole_w and 0.0 <= m.margin_y < 0.5 * m.sole_h
    assert 0.0 < m.t_single < m.step_period and m.t_single <= 8.0 * m.T + 1e-12
    assert max_previewed_steps(m.N, m.T, m.step_period) <= S_MAX, (m.N, m.T, m.step_period)
    assert m.hip_l_lo < 0.0 < m.hip_l_hi and m.hip_r_lo < 0.0 < m.hip_r_hi


def corner_models(N=16, T=0.1):
    """named models at the edges of the ranges; step_period stays the default's unless the horizon cannot take it"""
    def base():
        m = defaults(N, T)
        if max_previewed_steps(N, T, m.step_period) > S_MAX:
            set_step_period(m, step_periods_for(N, T)[0])
        return m
    out = {}
    m = base(); m.margin_x = m.margin_y = 0.0; m.hip_vmax = HIP_VMAX_ROBOT; out["no_margins_feet_turn"] = m
    m = base(); m.margin_x = 0.47 * m.sole_w; m.margin_y = 0.47 * m.sole_h; out["sliver_polygon"] = m
    m = base(); m.alpha *= 10; m.beta *= 0.1; m.gamma *= 10; m.com_height_qp = 0.6; out["stiff_weights_low_com"] = m
    m = base(); m.alpha *= 0.1; m.beta *= 10; m.gamma *= 0.1; m.com_height_qp = 1.0; out["soft_weights_high_com"] = m
    m = base(); m.hip_l_lo = m.hip_r_lo = -6 * math.pi / 180; m.hip_l_hi = m.hip_r_hi = 6 * math.pi / 180
    m.hip_amax *= 2; m.feet_cross_max *= 0.5; out["tight_hips"] = m           # hip_vmax = 0: the feet never turn
    m = base(); m.ds_period = 0.3; m.dsss_period = 0.45; m.flags = FLAG_NO_STOP_CENTERING; m.step_height = 0.08
    m.ds_feet_distance = 0.16; m.feet_distance = 0.26; out["short_double_support"] = m
    for v in out.values():
        check_valid(v)
    return out


# ------------------------------------------------------------------------------------------------------------------ gaits
STRETCHES = ("walk", "turn", "stop", "stop", "stop", "walk")


def stretch_ticks(m):
    """ticks per stretch of the references: two step periods, so that three stretches of zero reference see the gait
    through the steps the FSM still takes (NbStepsSSDS = 2, three more after a rotation) and into double support"""
    return max(8, int(math.ceil(2.0 * m.step_period / m.T)))


def gait_velocity(seed, g, stretches=STRETCHES):
    """[len(stretches), 3] references of gait g: "walk" drawn as the horizon tests draw them, "turn" the same with
    |w| in 0.4 .. 0.6 rad/s (reaches the generator's hip limits within a stretch), "stop" zero"""
    rng = np.random.default_rng(list(np.atleast_1d(seed)) + [g, 77])
    v = np.zeros((len(stretches), 3))
    for k, kind in enumerate(stretches):
        if kind == "stop":
            continue
        v[k] = rng.uniform(-0.1, 0.3), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2)
        if kind == "turn":
            v[k, 2] = rng.uniform(0.4, 0.6) * (1.0, -1.0)[int(rng.integers(2))]
    return v


def gaits(seed, n_gaits, stretches=STRETCHES):
    """[n_gaits][len(stretches), 3]"""
    return [gait_velocity(seed, g, stretches) for g in range(n_gaits)]


def start_state(m):
    import herdt_replay as hr
    return w.start_state(hr.init_state, m)


# ----------------------------------------------------------------------------------------------------------------- oracle
def oracle_trace(pt, m, vel, n_ticks, redraw, last_out=None):
    """One gait on the oracle library pt (tests/workload.py:ptrig): per tick (rc, ifail, nb_prw_steps, n, phase,
    nb_steps_left, hip, n_iter, nact, m) and the state bytes after it.  hip: 0, or -- on a tick whose trunk velocity verify_angle_hip_joint
    rewrote -- (trunk yaw - support-foot yaw) / the hip limit on that side.  rc != 0 ends the trace.  last_out: a TickOut that receives the last tick's."""
    s = GaitState.from_buffer_copy(w.state_bytes(start_state(m)))
    out = TickOut()
    rows, states = [], []
    for t in range(n_ticks):
        if t % redraw == 0:
            s.vref[0], s.vref[1], s.vref[2] = vel[t // redraw]
        w.advance_clock(s, m, w.advance_calls(t))
        C.memset(C.byref(out), 0, C.sizeof(out))
        w0, wref = s.trunk_yaw[1], s.vref[2]
        rc = pt.wgo_mpc_tick(C.byref(m), C.byref(s), C.byref(out), None)
        hip = 0.0
        if rc == 0 and s.phase == 0:
            # verify_acceleration_hip_joint's trunk velocity, in its own evaluation order; verify_angle_hip_joint rewrites it
            # where the trunk would leave the support foot's hip limit behind
            dw = 2.0 / 3.0 * m.T * m.hip_amax
            want = wref if abs(wref - w0) <= dw else w0 + (-1.0 if wref - w0 < 0.0 else 1.0) * 2.0 / 3.0 * m.T * m.hip_amax
            if s.trunkT_yaw[1] != want:
                lo, hi = (m.hip_l_lo, m.hip_l_hi) if s.foot == 0 else (m.hip_r_lo, m.hip_r_hi)
                rel = s.trunk_yaw[0] - s.sup_yaw
                hip = rel / (hi if rel >= 0.0 else -lo)
        rows.append((rc, out.ifail, out.nb_prw_steps, out.n, s.phase, s.nb_steps_left, hip, out.n_iter, out.nact, out.m))
        states.append(w.state_bytes(s))
        if rc != 0:
            break
    if last_out is not None:
        C.memmove(C.byref(last_out), C.byref(out), C.sizeof(out))
    return np.array(rows, dtype=np.float64), states


def scan_previewed_steps(pt, N, T=0.1, grid=STEP_PERIOD_GRID):
    """{step_period: largest nb_prw_steps the oracle previews over three step periods of straight walking from the start
    pose}; 99 where the oracle itself gives up (more than its SMAX = 6 previewed steps: wgo_mpc_tick returns -3)"""
    res = {}
    for p in grid:
        m = defaults(N, T)
        set_step_period(m, p)
        n_ticks = int(math.ceil((m.dsss_period + 3.0 * p) / T)) + 2
        rows, _ = oracle_trace(pt, m, np.array([[0.2, 0.0, 0.0]]), n_ticks, n_ticks)
        res[p] = 99 if rows[-1, 0] != 0 else int(rows[:, 2].max())
    return res


# ------------------------------------------------------------------------------------------------------------------ sweeps
# (name, N, step-period range, seeds of random_model, corner models).  "16c": the compact view; "16e": N = 16 sent to the
# element view by the model (more than two previewed steps); 12 / 13 / 14: around TickLds::elem_overlay_apart; 20: the
# any-horizon kernel above the compact horizon; 32: the fixed-horizon kernel.  The seeds were chosen on the oracle alone
# (tests/test_models_oracle.py asserts what they were chosen for): at most a tenth of the (model, gait) pairs may hold a
# tick whose QP fails -- the "sliver_polygon" corner fails on most ticks, seeds 10 at N = 12 and 19 at N = 32 on a few.
SWEEP = (("16c", 16, (0.8, 1.2), (3, 14, 15, 19), ("no_margins_feet_turn", "sliver_polygon", "tight_hips")),
         ("16e", 16, (0.0, 0.75), (6, 11, 15, 18), ("stiff_weights_low_com", "soft_weights_high_com", "short_double_support")),
         ("12", 12, (0.0, 1.2), (5, 6, 10, 12), ("no_margins_feet_turn", "tight_hips", "short_double_support")),
         ("13", 13, (0.0, 1.2), (0, 2, 6, 8), ("stiff_weights_low_com", "soft_weights_high_com", "tight_hips")),
         ("14", 14, (0.0, 1.2), (0, 2, 5, 7), ("no_margins_feet_turn", "short_double_support", "stiff_weights_low_com")),
         ("20", 20, (0.0, 1.2), (0, 2, 3, 10), ("soft_weights_high_com", "tight_hips", "short_double_support")),
         ("32", 32, (0.0, 1.2), (6, 13, 17, 19), ("sliver_polygon", "no_margins_feet_turn", "tight_hips")))
SWEEP_GAITS = 2
SWEEP_NAMES = tuple(c[0] for c in SWEEP)


def sweep_models(name):
    """[(model name, model)] of one row of SWEEP"""
    k = SWEEP_NAMES.index(name)
    _, N, (lo, hi), seeds, corners = SWEEP[k]
    grid = step_periods_for(N, lo=lo, hi=hi)
    out = [("seed%d" % s, random_model(s, N, step_periods=grid)) for s in seeds]
    cm = corner_models(N)
    for c in corners:
        if name == "16e":
            set_step_period(cm[c], 0.5)                          # three previewed steps: the element view
        out.append((c, cm[c]))
    for _, m in out:
        check_valid(m)
        assert compact_view(m) == (name == "16c"), (name, m.step_period)
    return out


def sweep_gaits(name, model_index, n_gaits=SWEEP_GAITS):
    return gaits([SWEEP_NAMES.index(name), model_index], n_gaits)


def horizon_model(N):
    """the default model at horizon N with a hip-yaw velocity bound, so that the feet turn with the trunk"""
    m = defaults(N)
    m.hip_vmax = HIP_VMAX_ROBOT
    check_valid(m)
    return m


HORIZON_STRETCHES = ("walk", "turn")
HORIZON_STRETCH_TICKS = 14                                      # 28 ticks: double support (0.8 s), then two steps and a half


def view_model(step_period):
    """N = 16 with the step period alone deciding the view (tests/test_models_gpu.py)"""
    m = defaults(16)
    set_step_period(m, step_period)
    m.hip_vmax = HIP_VMAX_ROBOT
    check_valid(m)
    return m


VIEW_STEP_PERIODS = (2.0, 1.6, 1.0, 0.8, 0.75, 0.7, 0.5, 0.4)
assert VIEW_STEP_PERIODS[4] == STEP_PERIOD_GRID[STEP_PERIOD_GRID.index(0.8) + 1]      # the grid's next value below 0.8
