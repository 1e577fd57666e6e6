"""The N = 16 solver's seeded norm chain on the device (jrl-walkgen_amd/csrc/wg_ql_norms.hpp): whichever way the
rotation norms of a sweep are formed, the tick computes the oracle's bytes -- and the seeded chain really is the one that runs.

The sample of tests/test_iteration_paths_gpu.py (B = 64 gaits x 48 ticks of the benchmark's recipe, velocity references x 1, 3
and 7) runs under each setting of WG_QL_NORMS, read when the model is configured:
  unset     the chain from lane-parallel seeds, every rotation checked against the exact form afterwards, the exact chain again on
            a mismatch;
  exact     the exact chain throughout (the parent's behaviour);
  doubt     the check reports a mismatch in every sweep: the seeded chain AND the exact one, everywhere.
Each through one wg_mpc_tick_batch_dev launch per tick with EVERY tick's add / drop history, and through the staged multi-tick
launch.  Diag rows, histories and final states must equal the oracle's (computed once per scale by that module and shared) byte
for byte.  One case doubts the sums as well (WG_QL_SUMS=doubt): the solve that is entered again must keep the norms' mode.

The counters of the profile build (lib/libwg_mpc_prof.so, in a fresh child process): at scale 1 at least 90 % of the sweeps take
the seeded chain and at most 1 in 10 000 of those falls back; under `doubt` every seeded sweep falls back."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import test_guarded_sums_gpu as gs
import test_iteration_paths_gpu as ip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROF_LIB = os.path.join(ROOT, "jrl-walkgen_amd", "lib", "libwg_mpc_prof.so")
MODES = (None, "exact", "doubt")


@pytest.fixture
def knobs():
    """Sets WG_QL_NORMS / WG_QL_SUMS for the configuration the test makes; afterwards the context is configured again without."""
    old = {k: os.environ.get(k) for k in ("WG_QL_NORMS", "WG_QL_SUMS")}

    def put(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def set_modes(norms, sums=None):
        put({"WG_QL_NORMS": norms, "WG_QL_SUMS": sums})
    yield set_modes
    put(old)
    wg = ip._wg()
    wg.mpc_configure(wg.model_defaults())


def _one_launch_per_tick(what, scale):
    import fleet_oracle as fo
    wg = ip._binding()
    ref = ip._oracle(scale)
    final, diag, hist, hlen = gs._per_tick_with_histories(scale)
    fo.assert_diag_equal(ref["diag"], diag, what)
    for t in range(ip.T):
        for g in range(ip.B):
            h = ref["hists"][t][g]
            assert int(hlen[t, g]) == len(h) and tuple(int(v) for v in hist[t, g, :len(h)]) == h, (what, "history", t, g)
    fo.assert_records_equal(ref["final"], final, C.sizeof(wg.GaitState), what + ": final states", names=fo.word_names(wg.GaitState))
    assert final == ref["final"], what


@pytest.mark.parametrize("scale", ip.SCALES)
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m or "unset")
def test_one_launch_per_tick_every_history(mode, scale, knobs):
    knobs(mode)
    _one_launch_per_tick("WG_QL_NORMS=%s, scale %g, wg_mpc_tick_batch_dev" % (mode, scale), scale)


@pytest.mark.parametrize("scale", ip.SCALES)
@pytest.mark.parametrize("mode", MODES, ids=lambda m: m or "unset")
def test_staged_multi_tick_launch(mode, scale, knobs):
    knobs(mode)
    ip._compare(scale, True)


@pytest.mark.parametrize("scale", ip.SCALES)
def test_a_solve_entered_again_keeps_the_mode(scale, knobs):
    knobs("doubt", "doubt")
    _one_launch_per_tick("WG_QL_NORMS=doubt WG_QL_SUMS=doubt, scale %g, wg_mpc_tick_batch_dev" % scale, scale)
    ip._compare(scale, True)


def test_an_unknown_setting_is_refused(knobs):
    wg = ip._wg()
    knobs("sometimes")
    with pytest.raises(Exception):
        wg.mpc_configure(wg.model_defaults())


_COUNT = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_iteration_paths_gpu as ip
wg = ip._wg()
buf = (C.c_ulonglong * 48)()
assert wg.lib().wg_prof_read(buf) == 0
ip._gpu(1.0, True)
assert wg.lib().wg_prof_read(buf) == 0
print(json.dumps({"sweeps": int(buf[45]), "seeded": int(buf[46]), "fallbacks": int(buf[47])}))
"""


def _counters(norms):
    env = dict(os.environ, WG_LIB_PATH=PROF_LIB)
    env.pop("WG_QL_SUMS", None)
    env.pop("WG_QL_NORMS", None)
    if norms:
        env["WG_QL_NORMS"] = norms
    r = subprocess.run([sys.executable, "-c", _COUNT, ROOT, os.path.join(ROOT, "tests")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    c = json.loads(r.stdout.strip().splitlines()[-1])
    print("WG_QL_NORMS=%s" % norms, c)
    return c


@pytest.mark.skipif(not os.path.exists(PROF_LIB), reason="lib/libwg_mpc_prof.so is not built (make lib/libwg_mpc_prof.so)")
def test_the_seeded_chain_is_the_one_that_runs():
    c = _counters(None)
    assert c["sweeps"] > 0, c
    assert c["seeded"] >= 0.9 * c["sweeps"], c
    assert c["fallbacks"] * 10000 <= c["seeded"], c


@pytest.mark.skipif(not os.path.exists(PROF_LIB), reason="lib/libwg_mpc_prof.so is not built (make lib/libwg_mpc_prof.so)")
def test_doubt_sends_every_seeded_sweep_through_the_fallback():
    c = _counters("doubt")
    assert c["seeded"] > 0 and c["fallbacks"] == c["seeded"], c
