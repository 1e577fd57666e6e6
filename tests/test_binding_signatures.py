"""The ctypes binding takes every argtypes / restype from include/wg_mpc.h (wgmpc.header_signatures, wgmpc.bind): no prototype
is skipped, every context form is its base behind the handle, one prototype per type of the ABI is pinned literally (read off the
header's text, so the parser cannot pass by agreeing with itself), an unknown type is an error that names the prototype, and the
header -- list of context forms included -- is still C99 and C++17.  No GPU, no device call."""
import ctypes as C
import importlib
import os
import shutil
import subprocess
import sys

import pytest

from test_capi_load import _declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wg_mpc.h")
wg = importlib.import_module("jrl-walkgen_amd")
P, I, D = C.c_void_p, C.c_int, C.c_double


def test_every_declared_name_has_a_signature():
    sigs = wg.header_signatures(open(HEADER).read())
    assert sorted(sigs) == _declared_symbols() and len(sigs) >= 178
    assert os.path.samefile(wg.HEADER_PATH, HEADER)


def test_context_forms_are_their_base_behind_the_handle():
    lib = wg.lib()
    twins = [n for n in _declared_symbols() if n.endswith("_ctx")]
    assert len(twins) >= 69
    for n in twins:
        base, fn = getattr(lib, n[:-4]), getattr(lib, n)
        assert fn.argtypes == [P] + list(base.argtypes), n
        assert fn.restype == base.restype, n
    # every name of the header is bound on the loaded library, not only the context forms
    for n, (restype, argtypes) in wg.header_signatures(open(HEADER).read()).items():
        assert (getattr(lib, n).restype, getattr(lib, n).argtypes) == (restype, argtypes), n


def test_one_prototype_per_type_of_the_abi():
    lib = wg.lib()
    assert (lib.wg_dimitrov_walk_time.argtypes, lib.wg_dimitrov_walk_time.restype) == ([D, I], D)
    assert lib.wg_shard_range.argtypes == [C.c_longlong, I, I, P, P] and lib.wg_shard_range.restype == I
    assert lib.wg_overlap_serialised.restype == C.c_longlong and lib.wg_overlap_serialised.argtypes == []
    assert lib.wg_host_alloc.argtypes == [P, C.c_size_t]
    assert lib.wg_host_free.restype is None and lib.wg_host_free.argtypes == [P]
    assert lib.wg_last_error.restype == C.c_char_p and lib.wg_last_error.argtypes == []
    assert lib.wg_mpc_tick_lds_bytes_for.restype == C.c_size_t
    assert lib.wg_gait_init.argtypes == [P] * 5 and lib.wg_gait_init.restype is None          # the last three are double [3]
    follow = lib.wg_dimitrov_follow_dev.argtypes
    assert len(follow) == 20 and [i for i, t in enumerate(follow) if t is I] == [0, 1, 6, 10, 13, 14, 18]
    assert all(t is P for i, t in enumerate(follow) if i not in (0, 1, 6, 10, 13, 14, 18))
    # (models, T, B, smax, steps, n_steps, init_feet, com0, blocks, status, t_start, lcap, 7 outputs, length, hip_stream): the doubles
    # are T and t_start, parameters 1 and 10 of the prototype and 2 and 11 behind the context
    walk = lib.wg_morisawa_walk_fleet_dev.argtypes
    assert len(walk) == 21 and [i for i, t in enumerate(walk) if t is D] == [1, 10]
    assert [i for i, t in enumerate(walk) if t is I] == [2, 3, 11]
    assert [i for i, t in enumerate(lib.wg_morisawa_walk_fleet_dev_ctx.argtypes) if t is D] == [2, 11]
    # the discrepancies the hand-written lists had
    assert lib.wg_dimitrov_configure.argtypes == [P] and lib.wg_dimitrov_configure_ctx.argtypes == [P, P]
    assert lib.wg_zmpdisc_defaults.restype is None and lib.wg_morisawa_defaults.restype is None


@pytest.mark.parametrize("text,name", [("int wg_x(float a);", "wg_x"), ("struct foo wg_y(void);", "wg_y"),
                                       ("int wg_z(int a, unsigned b);", "wg_z"), ("void *wg_w(void);", "wg_w")])
def test_an_unknown_type_is_an_error_that_names_the_prototype(text, name):
    with pytest.raises(wg.WgError, match=name):
        wg.header_signatures("int wg_ok(int a, const double *b);\n" + text)


def test_a_missing_header_fails_as_a_missing_library_does(monkeypatch, tmp_path):
    monkeypatch.setattr(sys.modules[wg.bind.__module__], "HEADER_PATH", str(tmp_path / "wg_mpc.h"))
    with pytest.raises(wg.WgError, match="wg_mpc.h missing"):
        wg.bind(object())


def test_the_parser_on_a_small_header():
    sigs = wg.header_signatures("""
        /* int wg_in_a_comment(int); */
        #define WG_MACRO(x) wg_not_a_prototype(x)
        typedef struct wg_s { int a; double b[3]; } wg_s_t;
        const char *wg_a(void);
        long long wg_b(size_t n, const wg_s_t *s,
                       double v[3] /* an array */);
        #define WG_LIST(X) \\
          X(long long, wg_b, (size_t n, const wg_s_t *s, double v[3]), (n, s, v))
        """)
    assert sigs == {"wg_a": (C.c_char_p, []), "wg_b": (C.c_longlong, [C.c_size_t, P, P]),
                    "wg_b_ctx": (C.c_longlong, [P, C.c_size_t, P, P])}


@pytest.mark.parametrize("lang", [("c", "-std=c99"), ("c++", "-std=c++17")])
def test_the_header_is_still_c_and_cxx(lang):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    r = subprocess.run([cc, lang[1], "-pedantic", "-Wall", "-fsyntax-only", "-x", lang[0], HEADER], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the header's own _Static_assert of its struct sizes is C11: the one thing -pedantic has to say under -std=c99
    notes = [l for l in r.stderr.splitlines() if ("warning" in l or "error" in l) and "_Static_assert" not in l]
    assert not notes, r.stderr
