"""The ctypes mirrors of wg_sole_t and wg_zmpdisc_fleet_t have the sizes include/wg_mpc.h asserts, and the fields where the
header puts them (no GPU needed)."""
import ctypes as C
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
wg = importlib.import_module("jrl-walkgen_amd")
HEADER = open(os.path.join(ROOT, "include", "wg_mpc.h")).read()


def header_bytes(macro, struct):
    n = int(re.search(r"#define %s (\d+)" % macro, HEADER).group(1))
    assert re.search(r"static_assert\(sizeof\(%s\) == %s," % (struct, macro), HEADER)
    return n


def test_sole_mirror():
    assert C.sizeof(wg.Sole) == wg.SOLE_BYTES == header_bytes("WG_SOLE_BYTES", "wg_sole_t") == 32
    assert [f[0] for f in wg.Sole._fields_] == ["sole_w", "sole_h", "constraint_x", "constraint_y"]
    assert [getattr(wg.Sole, k).offset for k in ("sole_w", "sole_h", "constraint_x", "constraint_y")] == [0, 8, 16, 24]


def test_zmpdisc_fleet_mirror():
    n = header_bytes("WG_ZMPDISC_FLEET_BYTES", "wg_zmpdisc_fleet_t")
    assert C.sizeof(wg.ZmpDiscFleet) == wg.ZMPDISC_FLEET_BYTES == n == C.sizeof(wg.ZmpDiscModel) + 8 + 2 * C.sizeof(C.c_void_p)
    F = wg.ZmpDiscFleet
    assert (F.base.offset, F.M.offset, F.models.offset, F.model_of.offset) == (0, 128, 136, 144)
    f = wg.zmpdisc_fleet(wg.ZmpDiscModel(), 3, 4096)
    assert (f.M, f.models, f.model_of) == (3, 4096, None)
