"""host/kajita_fleet.cpp --heights LO:HI: a CoM height per gait from plain C++ -- the gains made by wg_riccati_gains_batch_dev on
the walk's stream, the preview through the fleet forms -- in the program's four modes.  The program itself checks every gait's
status and holds gaits 0 and B - 1 to the one-gait host path configured with that gait's own wg_riccati_gains."""
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "jrl-walkgen_amd", "bin", "kajita_fleet")
wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu

MODES = {"plain": [], "online": ["--online", "3"], "online-ragged": ["--online", "3", "--ragged"], "plan": ["--plan"]}


def run(extra):
    r = subprocess.run([EXE, "--batch", "70", "--steps", "8"] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("mode", sorted(MODES))
def test_heights_in_every_mode(mode):
    assert os.path.exists(EXE)
    out = run(MODES[mode] + ["--heights", "0.6:0.9"])
    assert "CoM heights 0.6000 .. 0.9000 m" in out and "gaits 0 and 69 == host entry points with their own gains" in out
    assert re.search(r"checksum ([0-9a-f]{16})", out)


def test_heights_change_the_walk_and_one_height_does_not():
    """LO = HI = the program's own height: the fleet forms print the checksum of the configured path; a spread of heights another"""
    sums = [re.search(r"checksum ([0-9a-f]{16})", run(extra)).group(1)
            for extra in ([], ["--heights", "0.8078:0.8078"], ["--heights", "0.6:0.9"], ["--online", "3", "--heights", "0.6:0.9"])]
    assert sums[0] == sums[1] and sums[2] != sums[0] and sums[3] == sums[2]


def test_a_bad_range_is_refused():
    r = subprocess.run([EXE, "--batch", "4", "--heights", "0.9:0.6"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "FAILED" in r.stderr
