"""The step stack on the host (wg_steps_plan, wg_steps_count): whole wg_rel_step_t records and m_KeepLastCorrectSupportFoot, byte
for byte, against the oracle's restatement of StepStackHandler's generators in its portable-trigonometry build (wgo_steps_*),
and against a float64 statement for AddStepInTheStack / AddStandardOnLineStep; every refusal, with canary bytes around the row.
Runs without a GPU: the kernel's twin of the same arithmetic is held to these in test_steps_plan_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oraclelib as ol  # noqa: E402
import stepsplan as sp  # noqa: E402
from stepsplan import ADD, ARC, BAD, CAPACITY, IDLE, LS, NONE, ONLINE, SF, wg  # noqa: E402

CANARY = 0xA5


def check_against_oracle(cmds, rows, keep0, keep1, smax=64):
    buf, n, stack = sp.host_plan(cmds, keep0, smax)
    assert stack.error == 0 and n == len(rows) == wg.steps_count(wg.step_cmds(cmds), len(cmds)), cmds
    assert np.array_equal(buf[1:1 + n], rows), cmds                            # whole records: times, step_type, pad_
    assert (buf[0] == CANARY).all() and (buf[1 + n:] == CANARY).all()          # the row past n_steps, and its surroundings
    assert (stack.keep, stack.n_given, stack.pad_) == (keep1, n, 0), cmds


def test_abi_structs():
    assert C.sizeof(wg.StepCmd) == 32 and C.sizeof(wg.StepStack) == 16 and C.sizeof(wg.RelStep) == 48
    hdr = open(os.path.join(ROOT, "include", "wg_mpc.h")).read()
    assert "WG_STEP_NONE = 0, WG_STEP_SUPPORT_FOOT, WG_STEP_ARC, WG_STEP_LAST_SUPPORT, WG_STEP_ADD, WG_STEP_ONLINE, WG_STEP_ONLINE_IDLE" in hdr
    assert (wg.STEP_NONE, wg.STEP_SUPPORT_FOOT, wg.STEP_ARC, wg.STEP_LAST_SUPPORT, wg.STEP_ADD, wg.STEP_ONLINE, wg.STEP_ONLINE_IDLE) == \
        (NONE, SF, ARC, LS, ADD, ONLINE, IDLE)
    assert wg.lib().wg_abi_version() == 5


def test_turning_on_the_circle():
    """":supportfoot 1", ":arc 0.0 0.75 30.0 -1", ":lastsupport": the step stack the circle tests walk"""
    steps, S = ol.circle_steps(wg.RelStep, sp.SS, sp.DS, lib=sp.ptrig())
    rows = np.frombuffer(steps, dtype=np.uint8).reshape(64, sp.STEP_BYTES)[:S]
    assert S == 5
    check_against_oracle(sp.CIRCLE, rows, 1, 1)
    check_against_oracle(sp.CIRCLE, rows, 1, 1, smax=5)                         # exactly full


def test_random_command_lists_byte_for_byte():
    fam = sp.family(2008, 3000)
    arcs = [c for cmds, _, _, _ in fam for c in cmds if c[0] == ARC]
    numbers = [sp.arc_numbers(*c[2:]) for c in arcs]
    assert sum(1 for n, last in numbers if n > 0 and last == 0.0) > 20           # whole steps only: no closing step
    assert sum(1 for n, last in numbers if n == 0 and last == 0.0) > 20           # arcs of no step at all
    assert sum(1 for n, last in numbers if last != 0.0) > 1000
    for sx in (-1, 0, 1):
        for sy in (-1, 0, 1):
            assert any(np.sign(c[2]) == sx and np.sign(c[3]) == sy for c in arcs), (sx, sy)
    assert max(len(rows) for _, rows, _, _ in fam) > 40
    for cmds, rows, keep0, keep1 in fam:
        check_against_oracle(cmds, rows, keep0, keep1)


def test_every_special_arc_alone():
    """R = 0, a zero angle, and radius / angle pairs chosen to divide into whole 0.15 m steps"""
    exact = 0
    for c in sp.special_arcs():
        for foot in (1, -1):
            cmd = (ARC, foot) + c[2:]
            rows, keep1 = sp.oracle_list([cmd], keep=-foot)
            n, last = sp.arc_numbers(*c[2:])
            assert len(rows) == n + (last != 0.0)
            exact += n > 0 and last == 0.0
            if n == 0 and last == 0.0:
                assert keep1 == foot                                              # no step, and keep = foot
            check_against_oracle([cmd], rows, -foot, keep1)
    assert exact >= 4


def test_add_online_and_idle_against_the_float64_statement():
    rng = np.random.default_rng(11)
    for _ in range(500):
        keep = int(rng.choice([-1, 1]))
        x, y, th = rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), rng.uniform(-30, 30)
        for op in (ADD, ONLINE, IDLE):
            buf, n, stack = sp.host_plan([(op, 0, x, y, th)], keep, smax=1, ss=0.7, ds=0.1)
            got = buf[1].view(np.float64)[:5]
            sx, sy, t = (x, y, th) if op != IDLE else (0.0, 0.0, 0.0)
            sy = np.float64(sy) + np.float64(keep) * np.float64(0.19) if op != ADD else sy
            assert n == 1 and got.tolist() == [sx, float(sy), t, 0.7, 0.1] and not buf[1, 40:].any()
            assert stack.keep == (keep if op == ADD else -keep) and stack.n_given == 1


def test_cutting_a_list_changes_nothing():
    """keep is carried by the stack alone: one call, one command per call, uneven cuts"""
    rng = np.random.default_rng(5)
    for cmds, rows, keep0, keep1 in sp.family(77, 300):
        for cuts in ([len(cmds)], [1] * len(cmds), None):
            if cuts is None:
                cuts, left = [], len(cmds)
                while left:
                    cuts.append(int(rng.integers(0, left + 1)))
                    left -= cuts[-1]
            stack = wg.StepStack(keep0, 0, 0, 0)
            got, at = [], 0
            for k in cuts:
                buf, n, stack = sp.host_plan(cmds[at:at + k], smax=64, stack=stack)
                got.append(buf[1:1 + n])
                at += k
            assert np.array_equal(np.concatenate(got), rows) and (stack.keep, stack.n_given, stack.error) == (keep1, len(rows), 0)


REFUSED = [
    ("unknown op", [(7, 1, 0.0, 0.0, 0.0)], BAD), ("negative op", [(-1, 1, 0.0, 0.0, 0.0)], BAD),
    ("support foot 0", [(SF, 0, 0.0, 0.0, 0.0)], BAD), ("support foot 2", [(SF, 2, 0.0, 0.0, 0.0)], BAD),
    ("arc foot 0", [(ARC, 0, 0.0, 0.75, 30.0)], BAD), ("arc foot -2", [(ARC, -2, 0.0, 0.75, 30.0)], BAD),
    ("negative arc", [(ARC, 1, 0.0, 0.75, -30.0)], BAD), ("tiny negative arc", [(ARC, 1, 0.0, 0.75, -1e-300)], BAD),
    ("nan x", [(ARC, 1, float("nan"), 0.75, 30.0)], BAD), ("inf y", [(ONLINE, 0, 0.0, float("inf"), 0.0)], BAD),
    ("-inf theta", [(ADD, 0, 0.0, 0.1, float("-inf"))], BAD), ("nan angle", [(ARC, 1, 0.0, 0.75, float("nan"))], BAD),
    ("nan in an op that takes none", [(LS, 0, float("nan"), 0.0, 0.0)], BAD),
    ("radius overflows", [(ARC, 1, 1e200, 1e200, 0.0)], BAD),
    ("bad after good", [(SF, 1, 0.0, 0.0, 0.0), (ADD, 0, 0.1, 0.2, 0.0), (9, 0, 0.0, 0.0, 0.0)], BAD),
    ("five steps into four", sp.CIRCLE, CAPACITY),
    ("an arc of 10^9 steps", [(ARC, 1, 1e6, 0.0, 9000.0)], CAPACITY), ("an arc of 10^300 steps", [(ARC, 1, 1e150, 0.0, 1e150)], CAPACITY),
    ("one step too many", [(ADD, 0, 0.1, 0.2, 0.0)] * 5, CAPACITY),
]


@pytest.mark.parametrize("name,cmds,code", REFUSED, ids=[r[0] for r in REFUSED])
def test_refusals_write_nothing_and_stick(name, cmds, code):
    stack = wg.StepStack(-1, 0, 3, 0)
    buf, n, stack = sp.host_plan(cmds, smax=4, stack=stack)
    assert n == 0 and (buf == CANARY).all()
    assert (stack.keep, stack.error, stack.n_given, stack.pad_) == (-1, code, 3, 0)
    buf, n, stack = sp.host_plan([(ADD, 0, 0.1, 0.2, 0.0)], smax=4, stack=stack)      # a good call afterwards: still refused
    assert n == 0 and (buf == CANARY).all() and (stack.keep, stack.error, stack.n_given) == (-1, code, 3)
    if code == BAD or len(cmds) == 1:
        assert wg.steps_count(wg.step_cmds(cmds), len(cmds)) == code
    else:
        assert wg.steps_count(wg.step_cmds(cmds), len(cmds)) == 5                      # fits a wider row


def test_more_refusals_and_host_side_errors():
    lib = wg.lib()
    one = wg.step_cmds([(ADD, 0, 0.1, 0.2, 0.0)])
    stack, steps, n = wg.StepStack(1, 0, 0, 0), (wg.RelStep * 4)(), C.c_int(-7)
    a = C.addressof
    # a negative count and a stack that was never initialised are the gait's own refusals
    assert lib.wg_steps_plan(a(one), -1, 0.7, 0.1, a(stack), 4, a(steps), a(n)) == 0 and (n.value, stack.error) == (0, BAD)
    zero = wg.StepStack(0, 0, 0, 0)
    assert lib.wg_steps_plan(a(one), 1, 0.7, 0.1, a(zero), 4, a(steps), a(n)) == 0 and (n.value, zero.error) == (0, BAD)
    assert wg.steps_count(one, -1) == BAD and lib.wg_steps_count(None, 1) == BAD and lib.wg_steps_count(None, 0) == 0
    # no commands: nothing happens, whatever the stack holds
    idle = wg.StepStack(-1, 0, 9, 0)
    assert lib.wg_steps_plan(None, 0, 0.7, 0.1, a(idle), 4, a(steps), a(n)) == 0
    assert (n.value, idle.keep, idle.error, idle.n_given) == (0, -1, 0, 9)
    # 65 steps: more than any call can hold
    many = wg.step_cmds([(ADD, 0, 0.1, 0.2, 0.0)] * 65)
    assert wg.steps_count(many, 64) == 64 and wg.steps_count(many, 65) == CAPACITY
    # the call's own arguments
    ok = wg.StepStack(1, 0, 0, 0)
    for args in ((a(one), 1, 0.7, 0.1, None, 4, a(steps), a(n)), (a(one), 1, 0.7, 0.1, a(ok), 4, None, a(n)),
                 (a(one), 1, 0.7, 0.1, a(ok), 4, a(steps), None), (None, 1, 0.7, 0.1, a(ok), 4, a(steps), a(n)),
                 (a(one), 1, 0.7, 0.1, a(ok), 0, a(steps), a(n)), (a(one), 1, 0.7, 0.1, a(ok), 65, a(steps), a(n)),
                 (a(one), 1, float("nan"), 0.1, a(ok), 4, a(steps), a(n)), (a(one), 1, 0.7, float("inf"), a(ok), 4, a(steps), a(n))):
        assert lib.wg_steps_plan(*args) == -2
    assert (ok.keep, ok.error, ok.n_given) == (1, 0, 0)


def test_capacity_edge():
    """an arc that gives exactly smax steps passes; smax + 1 is refused before its first step"""
    for smax, cmd in ((1, (ARC, 1, 0.0, 0.75, 5.0)), (7, (ARC, -1, 0.0, -0.75, 75.0)), (64, (ARC, 1, -3.0, 0.0, 182.0))):
        rows, keep1 = sp.oracle_list([cmd])
        assert len(rows) == smax, (smax, len(rows))
        check_against_oracle([cmd], rows, 1, keep1, smax=smax)
        if smax > 1:
            buf, n, stack = sp.host_plan([cmd], smax=smax - 1)
            assert n == 0 and stack.error == CAPACITY and (buf == CANARY).all()
