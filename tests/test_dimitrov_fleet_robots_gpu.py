"""host/dimitrov_fleet.cpp --robots LO:HI: a robot of its own size per gait from plain C++ -- CoM height, walk model, support times
and sole per gait through the producers' fleet forms (wg_steps_plan_fleet_dev, wg_zmpdisc_*_fleet_dev,
wg_foot_constraints_fleet_dev / _append_fleet_dev) and the Dimitrov fleet forms, all on one stream -- in the program's modes.  The
program itself holds gaits 0 and B - 1 to the one-model producers and a context configured with that gait's own models."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "jrl-walkgen_amd", "bin", "dimitrov_fleet")
pytestmark = pytest.mark.gpu

MODES = {"plain": [], "online-follow": ["--online", "3", "--follow"], "plan": ["--plan"]}
CHECKED = "gaits 0 and 69 == the one-model producers with their own model and sole"


def run(extra):
    r = subprocess.run([EXE, "--batch", "70", "--steps", "8"] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def checksum(out):
    return re.search(r"checksum ([0-9a-f]{16})", out).group(1)


@pytest.fixture(scope="module")
def spread():
    """--robots 0.8:1.2 in every mode, run once: {mode: output}"""
    assert os.path.exists(EXE)
    return {mode: run(extra + ["--robots", "0.8:1.2"]) for mode, extra in MODES.items()}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_robots_in_every_mode_print_the_self_check_and_a_checksum(spread, mode):
    out = spread[mode]
    assert "robots of size 0.8000 .. 1.2000" in out and CHECKED in out
    assert "the constants of 70 models made on the device, all status 0" in out
    assert "gaits 0 and 69 == a context configured with their own model" in out
    assert checksum(out)


def test_one_walk_one_checksum_however_it_is_fed(spread):
    """the built-in fleet whole and fed on line with a follow behind every feeding; --plan walks the steps of its command lists,
    which are not the built-in fleet's, so it is held to itself fed on line and to its host-fed twin"""
    assert checksum(spread["plain"]) == checksum(spread["online-follow"])
    plan = checksum(spread["plan"])
    assert plan != checksum(spread["plain"])
    assert plan == checksum(run(["--plan", "--online", "3", "--follow", "--robots", "0.8:1.2"]))
    assert plan == checksum(run(["--plan-host", "--robots", "0.8:1.2"]))


@pytest.mark.parametrize("mode", sorted(MODES))
def test_robots_of_size_one_walk_as_without_the_flag_and_a_spread_does_not(spread, mode):
    none, one = run(MODES[mode]), run(MODES[mode] + ["--robots", "1:1"])
    assert CHECKED in one and CHECKED not in none
    assert checksum(one) == checksum(none) != checksum(spread[mode])


def test_a_bad_range_is_refused():
    for bad in ("1.2:0.8", "0:1", "1"):
        r = subprocess.run([EXE, "--batch", "4", "--robots", bad], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "FAILED: need --robots LO:HI" in r.stderr and "checksum" not in r.stdout, bad
    r = subprocess.run([EXE, "--batch", "4", "--robots", "0.9:1.1", "--heights", "0.7:0.8"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "FAILED" in r.stderr
