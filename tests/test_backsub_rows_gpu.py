"""The back substitution of the N = 16 solver (compact view) runs its bottom eight rows at their own lengths (bs_row's kExact,
jrl-walkgen_amd/csrc/wg_ql_phases.hpp): the r-th row from the bottom adds r terms and requests r LDS-borne terms for the
row above it, where it used to add and read a head rounded up to four or eight (+0.0 entries beyond the row).  Every row length
0 .. 8 is a code path of its own now, followed by the general rows with a tail.

The bytes are held to the oracle by tests/test_iteration_paths_gpu.py (every tick's diag row, final states, the last tick's
history) and tests/test_guarded_sums_gpu.py (every tick's history) on the sample of B = 64 gaits x 48 ticks at three scales.  This
module asserts, from the oracle alone, that the sample runs back substitutions of EVERY size 1 .. 9 and of sizes with a tail of
one, two and three groups (10 .. 13, 14 .. 17, 18 and more), so that a change of the recipe cannot hollow those tests out; and it
runs the sample once more through one launch per tick with every history at the scale that reaches the largest active sets."""
import ctypes as C

import pytest

import test_guarded_sums_gpu as gs
import test_iteration_paths_gpu as ip

pytestmark = pytest.mark.gpu


def _sizes(scale):
    """Active-set sizes at which a solve of the sample adds or drops a constraint, i.e. sizes of triangular systems it solved: the
    step's back substitution runs at the size before every add, the multipliers' at the size before every drop."""
    seen = set()
    for row in ip._oracle(scale)["hists"]:
        for h in row:
            nact = 0
            for e in h:
                if nact > 0:
                    seen.add(nact)
                nact += 1 if e > 0 else -1
                assert nact >= 0, h
    return seen


def test_sample_solves_triangular_systems_of_every_unrolled_size_and_with_tails():
    seen = set()
    for scale in ip.SCALES:
        s = _sizes(scale)
        print("scale %g: sizes" % scale, sorted(s))
        seen |= s
    assert set(range(1, 10)) <= seen, sorted(seen)
    assert any(10 <= n <= 13 for n in seen) and any(14 <= n <= 17 for n in seen) and any(n >= 18 for n in seen), sorted(seen)


def test_one_launch_per_tick_every_history_at_the_largest_scale():
    import fleet_oracle as fo
    scale = ip.SCALES[-1]
    wg = ip._binding()
    ref = ip._oracle(scale)
    final, diag, hist, hlen = gs._per_tick_with_histories(scale)
    what = "scale %g, wg_mpc_tick_batch_dev, every history" % scale
    fo.assert_diag_equal(ref["diag"], diag, what)
    for t in range(ip.T):
        for g in range(ip.B):
            h = ref["hists"][t][g]
            assert int(hlen[t, g]) == len(h) and tuple(int(v) for v in hist[t, g, :len(h)]) == h, (what, "history", t, g)
    fo.assert_records_equal(ref["final"], final, C.sizeof(wg.GaitState), what + ": final states", names=fo.word_names(wg.GaitState))
    assert final == ref["final"], what
