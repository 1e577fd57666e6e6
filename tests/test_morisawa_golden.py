"""The Morisawa-2007 short walk of the reference (TestMorisawa2007, ":stepseq" of seven steps) against its own golden files,
tests/golden/morisawa_shortwalk_datref.npz (made by tests/golden/make_golden_morisawa.py): the float64 restatement
(tests/morisawa.py) and the library's host twin (wg_morisawa_solve + wg_morisawa_sample).  No GPU.

Start CoM.  The reference takes it from its HRP-2 model, which is not in its data.  The trajectory is affine in the start x and
y, so the two numbers are fitted by least squares on the six CoM / dCoM / ZMP columns; the fit gives 0.0316054587 and -1.2e-8.
The height is the file's column 4.

Alignment.  Golden row k is trajectory time 2 t_single + k additions of T.

Length.  FillQueues' loop (AnalyticalMorisawaCompact.cpp:2242) runs while t <= the sum of the interval times, 9.5 here.  The
sample at exactly that sum would be the 1589th; the float64 additions from 1.56 end at 9.500000000000098 > 9.499999999999998
(the sum as the reference adds it), so it is NOT produced: 1588 samples, the files' 1588 rows.

Tolerance.  2e-7 absolute on every compared entry: the files are written with 7 decimals and differ from each other by 1e-7
in places; the restatement alone stays within 1.3e-7 (CoM, ZMP) and 1.0e-7 (feet).  Compared: all 1588 rows of the 32-bit file,
every recorded column.  Of the 64-bit file every column but the feet's x and y: that file is older than the reference's sources
-- its feet move on the cubic 3u^2 - 2u^3 where the sources (FootTrajectoryGenerationStandard.cpp:199-203) and the 32-bit file
have the quintic 10u^3 - 15u^4 + 6u^5 -- which test_the_older_file_has_cubic_feet pins down instead of assuming."""
import numpy as np
import pytest

import morisawa as mo
import morisawa_fleets as mf

TOL = 2e-7
COM_COLS = ("com_x", "dcom_x", "com_y", "dcom_y", "zmp_x", "zmp_y")
FOOT_COLS = tuple("%s_%s" % (f, a) for f in ("left", "right") for a in mo.AXES)


@pytest.fixture(scope="module")
def golden():
    g = np.load(mf.GOLDEN)
    names = [str(n) for n in g["names"]]
    model = dict(zip(("T", "t_single", "t_double", "step_height", "omega"), (float(v) for v in g["model"])))
    return dict(names=names, d32=g["data32"], d64=g["data64"], steps=[tuple(s) for s in g["steps"]], model=model,
                map32=g["map32"], map64=g["map64"])


def _columns(g, which, cols):
    return g[which][:, [g["names"].index(c) for c in cols]]


def _restated(g, com):
    K = len(g["d32"])
    w = mo.Walk(mo.F64, g["model"], g["steps"], mf.GOLDEN_FEET, com)
    rows = []
    for t in mo.clock(2 * g["model"]["t_single"], g["model"]["T"], K):
        s = w.sample(t)
        rows.append([s["com"][0], s["com"][1], s["com"][2], s["com"][3]] + s["zmp"] + s["left"] + s["right"])
    return np.array(rows)


@pytest.fixture(scope="module")
def fit(golden):
    """the start CoM x, y by least squares, and the restated walk from it [1588, 18]"""
    h = float(golden["d32"][0, golden["names"].index("com_z")])
    base, ex, ey = (_restated(golden, c)[:, :6] for c in ([0.0, 0.0, h], [1.0, 0.0, h], [0.0, 1.0, h]))
    A = np.stack([(ex - base).ravel(), (ey - base).ravel()], 1)
    x, y = np.linalg.lstsq(A, (_columns(golden, "d32", COM_COLS) - base).ravel(), rcond=None)[0]
    return dict(com=[float(x), float(y), h], walk=_restated(golden, [float(x), float(y), h]))


def test_fixture_is_what_the_maker_records(golden):
    assert golden["d32"].shape == golden["d64"].shape == (1588, 20)
    assert len(golden["steps"]) == 7 and golden["steps"][0] == (0.0, -0.105, 0.0)
    assert list(golden["map32"][:8]) == [0, 1, 2, 3, 5, 6, 8, 9] and golden["map32"][-1] == 33 and golden["map64"][-1] == 21
    assert golden["model"] == dict(T=0.005, t_single=0.78, t_double=0.02, step_height=0.07, omega=0.0)
    assert np.all(golden["d32"][:, 3] == golden["d32"][0, 3])              # the height never moves on this path


def test_fitted_start_com(fit):
    assert abs(fit["com"][0] - 0.0316054587) < 1e-9 and abs(fit["com"][1] + 1.2e-8) < 1e-9
    assert abs(fit["com"][0] - mf.GOLDEN_COM[0]) < 1e-9 and abs(fit["com"][1] - mf.GOLDEN_COM[1]) < 1e-9 and fit["com"][2] == mf.GOLDEN_COM[2]


def test_length_is_the_files_1588_rows(golden):
    wg = mf.wg()
    m = wg.morisawa_defaults()
    assert mf.model_dict(m) == golden["model"]
    assert mo.length(golden["model"], 7, 2 * m.t_single) == 1588
    assert wg.morisawa_length(m, 7, 2 * m.t_single) == 1588
    assert wg.morisawa_length(m, 7, 0.0) == 1588 + 312                     # 2 t_single / T more, the same end
    assert wg.morisawa_length(m, 1, 0.0) == wg.MORISAWA_BAD_INPUT and wg.morisawa_length(m, 15, 0.0) == wg.MORISAWA_BAD_INPUT


def test_restatement_against_both_files(golden, fit):
    w = fit["walk"]
    e_com = np.abs(w[:, :6] - _columns(golden, "d32", COM_COLS)).max()
    e_feet = np.abs(w[:, 6:] - _columns(golden, "d32", FOOT_COLS)).max()
    print("restatement vs the 32-bit file: CoM / ZMP %.3g, feet %.3g" % (e_com, e_feet))
    assert e_com <= TOL and e_feet <= TOL
    assert e_com <= 1.35e-7 and e_feet <= 1.05e-7                          # what the restatement alone was measured at
    keep = [i for i, c in enumerate(FOOT_COLS) if c[-2:] not in ("_x", "_y")]
    assert np.abs(w[:, :6] - _columns(golden, "d64", COM_COLS)).max() <= TOL
    assert np.abs(w[:, 6:][:, keep] - _columns(golden, "d64", FOOT_COLS)[:, keep]).max() <= TOL


def test_the_older_file_has_cubic_feet(golden):
    """first swing of each foot, x: the 64-bit file on 3u^2 - 2u^3, the 32-bit file on 10u^3 - 15u^4 + 6u^5, each to the print"""
    for foot in ("left", "right"):
        up = _columns(golden, "d32", (foot + "_z",))[:, 0] > 0
        k0 = int(np.argmax(up))
        k1 = k0 + int(np.argmin(up[k0:]))
        k0 -= 1
        u = (np.arange(k0, k1 + 1) - k0) / (k1 - k0)
        for which, shape in (("d64", 3 * u ** 2 - 2 * u ** 3), ("d32", 10 * u ** 3 - 15 * u ** 4 + 6 * u ** 5)):
            x = _columns(golden, which, (foot + "_x",))[k0:k1 + 1, 0]
            assert x[-1] - x[0] > 0.19 and np.abs(x - (x[0] + (x[-1] - x[0]) * shape)).max() <= TOL, (foot, which)


def test_host_twin_against_the_fixture(golden, fit):
    wg = mf.wg()
    m = wg.morisawa_defaults()
    smax, K = 7, 1588
    steps = wg.rel_steps(golden["steps"], 0.0, 0.0)
    blocks, status = wg.morisawa_solve(m, steps, [7], [mf.GOLDEN_FEET], [fit["com"]], smax)
    assert list(status) == [0]
    r = wg.morisawa_sample(blocks, status, smax, 2 * m.t_single, m.T, K)
    assert list(r["length"]) == [K]
    twin = np.concatenate([r["com"][:, :, 0], r["zmp_x"], r["zmp_y"], r["left"][:, :, 0], r["right"][:, :, 0]], 1)
    e32 = np.abs(twin - np.concatenate([_columns(golden, "d32", COM_COLS), _columns(golden, "d32", FOOT_COLS)], 1)).max()
    e_re = np.abs(twin - fit["walk"]).max()
    print("host twin vs the 32-bit file %.3g, vs the restatement %.3g" % (e32, e_re))
    assert e32 <= TOL
    assert e_re <= 1e-9
    keep = [i for i, c in enumerate(FOOT_COLS) if c[-2:] not in ("_x", "_y")]
    assert np.abs(twin[:, :6] - _columns(golden, "d64", COM_COLS)).max() <= TOL
    assert np.abs(twin[:, 6:][:, keep] - _columns(golden, "d64", FOOT_COLS)[:, keep]).max() <= TOL
    # the natures of the intervals (SetNatureInterval): support -1, flying 1, the double supports between steps 11 left / 9 right
    assert set(r["left_type"][:, 0]) == {-1, 1, 11} and set(r["right_type"][:, 0]) == {-1, 1, 9}
    for foot in ("left", "right"):                                         # a foot the file shows in the air is flying here
        assert np.all(r[foot + "_type"][_columns(golden, "d32", (foot + "_z",))[:, 0] > 0, 0] == 1)
