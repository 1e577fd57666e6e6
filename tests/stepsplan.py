"""What the step-stack tests share (test_steps_plan_host.py, test_steps_plan_gpu.py): the oracle's answer to a command list --
wgo_steps_support_foot / wgo_steps_arc / wgo_steps_last_support of the portable-trigonometry build, and a three-line float64
statement for the ops the oracle has no restatement of -- and the command lists themselves.  Computed once per process."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oraclelib as ol  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")

NONE, SF, ARC, LS, ADD, ONLINE, IDLE = range(7)
BAD, CAPACITY = -1, -2
STEP_BYTES = C.sizeof(wg.RelStep)
CMD_BYTES = C.sizeof(wg.StepCmd)
SS, DS = 0.78, 0.02
ORACLE_CAP = 1024

_pt = None


def ptrig():
    global _pt
    if _pt is None:
        subprocess.check_call(["make", "-s", "-C", ol.ORACLE_DIR, "libwg_oracle_ptrig.so"])
        _pt = C.CDLL(os.path.join(ol.ORACLE_DIR, "libwg_oracle_ptrig.so"))
        _pt.wgo_steps_arc.argtypes = [C.c_double] * 3 + [C.c_int] + [C.c_double] * 2 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _pt.wgo_steps_support_foot.argtypes = [C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
        _pt.wgo_steps_last_support.argtypes = [C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int]
    return _pt


def oracle_list(cmds, keep=1, ss=SS, ds=DS):
    """the steps a list of valid commands gives: (rows uint8 [n, STEP_BYTES], keep behind it)"""
    lib = ptrig()
    steps = (wg.RelStep * ORACLE_CAP)(); n = C.c_int(0)
    at, cap = C.addressof(steps), ORACLE_CAP
    for op, foot, a0, a1, a2 in cmds:
        if op == SF:
            assert lib.wgo_steps_support_foot(foot, ss, ds, at, C.byref(n), cap) == 0
        elif op == ARC:
            k = C.c_int(0)
            assert lib.wgo_steps_arc(a0, a1, a2, foot, ss, ds, at, C.byref(n), cap, C.byref(k)) == 0
            keep = k.value
        elif op == LS:
            assert lib.wgo_steps_last_support(keep, ss, ds, at, C.byref(n), cap) == 0
        elif op in (ADD, ONLINE, IDLE):
            # AddStepInTheStack / AddStandardOnLineStep (src/StepStackHandler.cpp:850-863, 791-832), in float64
            sx, sy, th = (np.float64(a0), np.float64(a1), np.float64(a2)) if op != IDLE else (np.float64(0), np.float64(0), np.float64(0))
            sy = sy + np.float64(keep) * np.float64(0.19) if op != ADD else sy
            keep = keep if op == ADD else -keep
            steps[n.value] = wg.RelStep(sx, sy, th, ss, ds, 0, 0)
            n.value += 1
        else:
            assert op == NONE
    rows = np.frombuffer(steps, dtype=np.uint8).reshape(ORACLE_CAP, STEP_BYTES)[:n.value].copy()
    return rows, keep


def arc_numbers(x, y, deg):
    """(NumberOfStep, LastStep) of CreateArcInStepStack in float64 (the sign flip of LastStep for x < 0 does not matter here)"""
    ot = np.float64(deg) * np.float64(np.pi) / np.float64(180.0)
    r = np.sqrt(np.float64(x) * np.float64(x) + np.float64(y) * np.float64(y))
    n = int(np.floor(ot * r / np.float64(0.15)))
    return n, float(ot * r - n * np.float64(0.15))


def random_arc(rng, max_steps):
    """R in [0.05, 3], both signs of x and y (the axes included), 0 .. 360 degrees, at most max_steps steps"""
    R = float(rng.choice([0.05, 0.15, 0.75, 3.0])) if rng.random() < 0.3 else float(rng.uniform(0.05, 3.0))
    phi = float(rng.choice([0.0, 0.5, 1.0, 1.5]) * np.pi) if rng.random() < 0.3 else float(rng.uniform(0, 2 * np.pi))
    x, y = R * np.cos(phi), R * np.sin(phi)
    if rng.random() < 0.3:                                   # exactly on an axis
        x, y = ((0.0, R), (0.0, -R), (R, 0.0), (-R, 0.0))[int(rng.integers(4))]
    r = float(np.hypot(x, y))
    most = min(360.0, max(max_steps - 1, 0) * 0.15 / r * 180.0 / np.pi)
    deg = float(rng.uniform(0.0, most))
    foot = int(rng.choice([-1, 1]))
    return (ARC, foot, float(x), float(y), deg)


def special_arcs():
    """count-0 arcs, and arcs whose LastStep is exactly 0.0 (whole steps only)"""
    out = [(ARC, 1, 0.0, 0.0, 40.0), (ARC, -1, 0.0, 0.0, 0.0), (ARC, -1, 0.3, -0.4, 0.0), (ARC, 1, -0.2, 0.0, 0.0), (ARC, 1, 0.0, 0.75, 5.0)]
    for k in range(1, 7):
        for R, x, y in ((0.15, 0.0, 0.15), (0.15, -0.15, 0.0), (0.3, 0.0, -0.3), (0.75, 0.75, 0.0)):
            out.append((ARC, 1 if k & 1 else -1, x, y, float(np.degrees(np.float64(k) * 0.15 / R))))
            out.append((ARC, -1, x, y, float(np.float64(k) * 0.15 / R * 180.0 / np.pi)))
    return out


def random_list(rng, max_cmds=8, max_steps=64):
    """a valid command list that gives at most max_steps steps"""
    n = int(rng.integers(1, max_cmds + 1))
    left = max_steps
    cmds = []
    spec = special_arcs()
    for _ in range(n):
        op = int(rng.choice([NONE, SF, ARC, ARC, LS, ADD, ONLINE, IDLE]))
        if op == ARC:
            c = spec[int(rng.integers(len(spec)))] if rng.random() < 0.25 else random_arc(rng, min(left, 24))
            cnt = len(oracle_list([c])[0])
        else:
            c = (op, int(rng.choice([-1, 1])) if op == SF else 0) + tuple(float(v) for v in (rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-20, 20)))
            cnt = 0 if op == NONE else 1
        if cnt > left:
            c, cnt = (NONE, 0, 0.0, 0.0, 0.0), 0
        cmds.append(c)
        left -= cnt
    return cmds


CIRCLE = [(SF, 1, 0.0, 0.0, 0.0), (ARC, -1, 0.0, 0.75, 30.0), (LS, 0, 0.0, 0.0, 0.0)]   # TurningOnTheCircle (tests/TestKajita2003.cpp:68-93)

_family = {}


def family(seed, count, max_cmds=8, max_steps=64):
    """`count` random lists with their oracle answers, computed once: [(cmds, rows, keep0, keep1)]"""
    key = (seed, count, max_cmds, max_steps)
    if key not in _family:
        rng = np.random.default_rng(seed)
        out = []
        for _ in range(count):
            cmds = random_list(rng, max_cmds, max_steps)
            keep0 = int(rng.choice([-1, 1]))
            rows, keep1 = oracle_list(cmds, keep0)
            out.append((cmds, rows, keep0, keep1))
        _family[key] = out
    return _family[key]


def cmd_bytes(lists, ccap):
    """[B][ccap] wg_step_cmd_t as uint8 [B, ccap, CMD_BYTES] and n_cmds [B]"""
    B = len(lists)
    arr = (wg.StepCmd * (B * ccap))()
    n = np.zeros(B, np.int32)
    for b, cmds in enumerate(lists):
        assert len(cmds) <= ccap
        n[b] = len(cmds)
        for i, (op, foot, a0, a1, a2) in enumerate(cmds):
            arr[b * ccap + i] = wg.StepCmd(op, foot, (a0, a1, a2))
    return np.frombuffer(arr, dtype=np.uint8).reshape(B, ccap, CMD_BYTES).copy(), n


def host_plan(cmds, keep=1, smax=64, ss=SS, ds=DS, stack=None, canary=0xA5):
    """wg_steps_plan on one list: (row bytes [smax + 2, STEP_BYTES] with a guard record either side, n_steps, stack)"""
    stack = stack if stack is not None else wg.StepStack(keep, 0, 0, 0)
    buf = np.full((smax + 2, STEP_BYTES), canary, np.uint8)
    arr = wg.step_cmds(cmds)
    n = C.c_int(-7)
    rc = wg.lib().wg_steps_plan(C.addressof(arr), len(cmds), ss, ds, C.addressof(stack), smax, buf[1:].ctypes.data, C.addressof(n))
    assert rc == 0
    return buf, n.value, stack
