"""Host side of the Morisawa-2007 analytic walks (wg_morisawa_solve, _sample, _system, _coshsinh: the arithmetic the kernels compile
too, jrl-walkgen_amd/csrc/wg_morisawa_math.hpp) against the restatement tests/morisawa.py in float64 and in 50-digit mpmath.  No GPU.

Measured here (figures also in DESIGN.md 3.13):
  cosh / sinh against 50-digit values, 100 000 seeded arguments in [0, 40]: at most 1.24 ulp (cosh), 1.52 ulp (sinh); cap 4 ulp.
  samples against the 50-digit restatement, fleets of this file: the float64 restatement (libm, numpy's LAPACK solve) is within
  d_ref = 9.6e-12 m, the host twin within 9.6e-12 m; the bound is 16 x d_ref, and 16 x d_ref = 1.5e-10 m is below 1e-8 m."""
import ctypes as C
import math

import numpy as np
import pytest

import morisawa as mo
import morisawa_fleets as mf

U = 2.0 ** -53
ULP_CAP = 4.0
D_REF_FACTOR = 16.0          # the host twin may be this many times as far from the truth as the float64 restatement:
D_REF_CEILING = 1e-8         # its cosh / sinh may be at 4 ulp where libm's are below 1, its elimination rounds in another order;
                             # 16 x d_ref itself must stay below a tenth of the golden files' print precision
SHAPES = (2, 3, 7, 14)


@pytest.fixture(scope="module")
def wg():
    return mf.wg()


# ---- hyperbolic pair ----
def test_cosh_sinh_within_4_ulp_of_mpmath(wg):
    """measured maximum: 1.24 ulp (cosh), 1.52 ulp (sinh) over these 100 000 arguments"""
    import mpmath
    mpmath.mp.dps = 50
    rng = np.random.default_rng(2007)
    xs = np.concatenate([rng.uniform(0.0, 40.0, 60000), rng.uniform(0.0, 2.0, 20000), 10.0 ** rng.uniform(-12.0, 0.0, 19990),
                         [0.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 40.0, 0.5 * math.log(2.0), 1e-300, 2.0 ** -30,
                          39.999999, 0.3465735902799727]])
    assert len(xs) == 100000
    lib = wg.lib()
    c, s = C.c_double(), C.c_double()
    worst = [0.0, 0.0]
    for x in xs:
        assert lib.wg_morisawa_coshsinh(float(x), C.byref(c), C.byref(s)) == 0
        mx = mpmath.mpf(float(x))
        for i, (got, true) in enumerate(((c.value, mpmath.cosh(mx)), (s.value, mpmath.sinh(mx)))):
            if true == 0:
                assert got == 0.0
                continue
            ulp = mpmath.ldexp(1, math.frexp(float(true))[1] - 53)
            worst[i] = max(worst[i], float(abs(mpmath.mpf(got) - true) / ulp))
    print("cosh %.3f ulp, sinh %.3f ulp" % tuple(worst))
    assert worst[0] <= ULP_CAP and worst[1] <= ULP_CAP


def test_cosh_sinh_refuse_what_they_are_not_made_for(wg):
    lib = wg.lib()
    c, s = C.c_double(7.0), C.c_double(7.0)
    for x in (-1e-9, 40.000001, float("nan"), float("inf")):
        assert lib.wg_morisawa_coshsinh(x, C.byref(c), C.byref(s)) == wg.MORISAWA_BAD_INPUT
    assert c.value == 7.0 and s.value == 7.0


# ---- fleets, solved once ----
@pytest.fixture(scope="module")
def solved(wg):
    out = {}
    for smax in SHAPES:
        f = mf.Fleet(6, smax, 100 + smax)
        blocks, status = wg.morisawa_solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, smax)
        assert list(status) == [0] * f.B
        out[smax] = (f, blocks, [mo.Walk(mo.F64, mf.model_dict(f.models[b]), *f.gait(b)) for b in range(f.B)])
    return out


def test_struct_sizes_and_block_size(wg):
    import os
    import re
    hdr = open(os.path.join(mf.ROOT, "include", "wg_mpc.h")).read()
    assert C.sizeof(wg.MorisawaModel) == int(re.search(r"#define WG_MORISAWA_MODEL_BYTES (\d+)", hdr).group(1)) == 40
    assert C.sizeof(wg.MorisawaView) == int(re.search(r"#define WG_MORISAWA_VIEW_BYTES (\d+)", hdr).group(1))
    assert int(re.search(r"#define WG_MORISAWA_MAX_STEPS (\d+)", hdr).group(1)) == wg.MORISAWA_MAX_STEPS == 14
    for smax in range(2, 15):
        b = wg.morisawa_block_bytes(smax)
        n = 4 * smax + 8
        assert b % 128 == 0 and b >= 8 * (n * n + 102 * (2 * smax + 1))
    assert wg.morisawa_block_bytes(1) == 0 and wg.morisawa_block_bytes(15) == 0


@pytest.mark.parametrize("smax", SHAPES)
def test_blocks_unpack_to_the_restatement(wg, solved, smax):
    f, blocks, walks = solved[smax]
    close = lambda a, b, rtol=1e-13, atol=1e-13: np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float), rtol=rtol, atol=atol)  # noqa: E731
    for b in range(f.B):
        v, w = wg.morisawa_view(blocks[b], smax), walks[b]
        S, I = int(f.n_steps[b]), 2 * int(f.n_steps[b]) + 1
        assert (v["n_steps"], v["n_int"], v["n"], v["smax"]) == (S, I, 4 * S + 8, smax)
        assert v["com_height"] == f.com0[b, 2] and v["t_total"] == w.total
        assert list(v["dT"]) == w.dT and list(v["tref"]) == w.tref          # the same additions: the same doubles
        close(v["omega"], w.om, 1e-15, 0)
        close(v["support"], w.support)                                       # the chain of rotations, turning steps included
        close(v["profile_x"], w.axes[0]["profile"]); close(v["profile_y"], w.axes[1]["profile"])
        assert list(v["left_type"]) == w.ltype and list(v["right_type"]) == w.rtype
        for foot, ref in ((v["left"], w.left), (v["right"], w.right)):
            for j in range(I):
                for a in range(6):
                    c = ref[j][a]
                    close(foot[j, a, :len(c)], c, 1e-11, 1e-11)
                    assert not foot[j, a, len(c):].any()
        # Z and w entry by entry: Z's entries are closed forms (4 ulp of cosh / sinh at the most); w's interior entries are differences
        # of the cubics' values, so absolute
        Z, wx, wy = wg.morisawa_system(f.models[b], (wg.RelStep * S).from_buffer_copy(f.steps_bytes()[b * smax * 48:(b * smax + S) * 48]),
                                       f.init_feet[b], f.com0[b])
        Zr = np.array(w.Z(), float)
        assert np.array_equal(Z == 0, Zr == 0) and (np.count_nonzero(Z, axis=1) <= 7).all()
        close(Z, Zr, 8 * U * ULP_CAP, 0)
        close(wx, w.axes[0]["w"], 0, 1e-14); close(wy, w.axes[1]["w"], 0, 1e-14)
        assert np.array_equal(v["wx"], wx) and np.array_equal(v["wy"], wy)
        for ax, (zk, ck, vk, wk) in enumerate((("zmp_x", "cog_x", "Vx", "Wx"), ("zmp_y", "cog_y", "Vy", "Wy"))):
            for j in range(1, I - 1):                                        # the cubics do not depend on the solve
                close(v[zk][j, :4], w.axes[ax]["zmp"][j]); close(v[ck][j, :4], w.axes[ax]["cog"][j])
                assert v[zk][j, 4] == 0 and v[ck][j, 4] == 0


@pytest.mark.parametrize("smax", SHAPES)
def test_residual_factor_and_continuity(wg, solved, smax):
    """|| Z y - w ||_inf <= 8 n u (|| Z ||_inf || y ||_inf + || w ||_inf), u = 2^-53: the backward-error form of a pivoted LU with the
    small growth this matrix shows; P Z = L U from the block; CoM, dCoM and ZMP continuous at every junction to the same scale"""
    import mpmath
    mpmath.mp.dps = 50
    f, blocks, walks = solved[smax]
    for b in range(f.B):
        v = wg.morisawa_view(blocks[b], smax)
        S, I, n = v["n_steps"], v["n_int"], v["n"]
        Z, wx, wy = wg.morisawa_system(f.models[b], (wg.RelStep * S).from_buffer_copy(f.steps_bytes()[b * smax * 48:(b * smax + S) * 48]),
                                       f.init_feet[b], f.com0[b])
        Zl = Z.astype(np.longdouble)
        nz = np.abs(Z).sum(1).max()
        for w_, y_ in ((wx, v["yx"]), (wy, v["yy"])):
            bound = 8 * n * U * (nz * np.abs(y_).max() + np.abs(w_).max())
            res = float(np.abs(Zl @ y_.astype(np.longdouble) - w_.astype(np.longdouble)).max())
            assert res <= bound, (b, res, bound)
        L_, U_ = np.tril(v["lu"], -1) + np.eye(n), np.triu(v["lu"])
        PZ = Z.copy()
        for k in range(n):
            assert k <= v["piv"][k] < n
            PZ[[k, v["piv"][k]]] = PZ[[v["piv"][k], k]]
        assert np.abs(L_).max() <= 1.0                                       # partial pivoting
        assert np.abs(L_.astype(np.longdouble) @ U_.astype(np.longdouble) - PZ).max() <= 8 * n * U * np.abs(U_).max()
        for zk, ck, vk, wk, w_, y_ in (("zmp_x", "cog_x", "Vx", "Wx", wx, v["yx"]), ("zmp_y", "cog_y", "Vy", "Wy", wy, v["yy"])):
            scale = 8 * n * U * (nz * np.abs(y_).max() + np.abs(w_).max())
            for j in range(I - 1):
                T, om = mpmath.mpf(float(v["dT"][j])), mpmath.mpf(float(v["omega"][j]))
                ch, sh = mpmath.cosh(om * T), mpmath.sinh(om * T)
                V, W = mpmath.mpf(float(v[vk][j])), mpmath.mpf(float(v[wk][j]))
                cog, zmp = [mpmath.mpf(float(c)) for c in v[ck][j]], [mpmath.mpf(float(c)) for c in v[zk][j]]
                end = (ch * V + sh * W + mo.poly(cog, T), om * sh * V + om * ch * W + mo.dpoly(cog, T), mo.poly(zmp, T))
                om1 = float(v["omega"][j + 1])
                start = (float(v[vk][j + 1]) + float(v[ck][j + 1][0]), om1 * float(v[wk][j + 1]) + float(v[ck][j + 1][1]), float(v[zk][j + 1][0]))
                for e, s_, what in zip(end, start, ("CoM", "dCoM", "ZMP")):
                    assert abs(float(e - s_)) <= scale * (float(om) if what == "dCoM" else 1.0), (b, j, what, float(e - s_), scale)


def test_samples_against_the_mpmath_truth(wg, solved):
    """d_ref: the largest distance of the float64 restatement from the 50-digit one over these fleets; the host twin stays within
    16 x d_ref, and 16 x d_ref is below 1e-8 m.  Measured: d_ref = 9.6e-12 m, host twin 9.6e-12 m."""
    d_ref = d_twin = 0.0
    for smax in SHAPES:
        f, blocks, walks = solved[smax]
        for b in (0, 1, 2):                                                  # S = smax, S = 2 and a ragged one; six 50-digit solves
            m, w64 = f.models[b], walks[b]
            truth = mo.Walk(mo.MP, mf.model_dict(m), *f.gait(b))
            t0 = mf.t_start_of(m)
            L = wg.morisawa_length(m, int(f.n_steps[b]), t0)
            assert L == mo.length(mf.model_dict(m), int(f.n_steps[b]), t0) > 100
            r = wg.morisawa_sample(blocks[b:b + 1], None, smax, t0, m.T, L)
            assert list(r["length"]) == [L]
            clk = mo.clock(t0, m.T, L)
            ks = sorted(set(list(range(0, L, max(1, L // 40))) + [L - 1] + [k for k in range(1, L) if w64.interval(clk[k]) != w64.interval(clk[k - 1])]))
            for k in ks:
                t, s64 = mo.Walk.sample(truth, clk[k]), w64.sample(clk[k])
                tv = [float(x) for x in t["com"] + t["zmp"] + t["left"] + t["right"]]
                v64 = s64["com"] + s64["zmp"] + s64["left"] + s64["right"]
                tw = list(r["com"][k, :, 0]) + [r["zmp_x"][k, 0], r["zmp_y"][k, 0]] + list(r["left"][k, :, 0]) + list(r["right"][k, :, 0])
                d_ref = max(d_ref, max(abs(a - c) for a, c in zip(v64, tv)))
                d_twin = max(d_twin, max(abs(a - c) for a, c in zip(tw, tv)))
                assert (r["left_type"][k, 0], r["right_type"][k, 0]) == (t["ltype"], t["rtype"])
    print("d_ref %.3g, host twin %.3g, bound %.3g" % (d_ref, d_twin, D_REF_FACTOR * d_ref))
    assert D_REF_FACTOR * d_ref < D_REF_CEILING
    assert d_twin <= D_REF_FACTOR * d_ref


def test_fleet_form_is_the_one_model_call_per_gait(wg, solved):
    """gait b of wg_morisawa_solve_fleet has the bytes of wg_morisawa_solve handed model b; a fleet of one model is the one-model call"""
    f, blocks, _ = solved[7]
    for b in range(f.B):
        one, st = wg.morisawa_solve(f.models[b], f.steps, f.n_steps, f.init_feet, f.com0, 7)
        assert st[b] == 0 and one[b].tobytes() == blocks[b].tobytes()
    same = (wg.MorisawaModel * f.B)(*[f.model] * f.B)
    a, _ = wg.morisawa_solve(same, f.steps, f.n_steps, f.init_feet, f.com0, 7)
    c, _ = wg.morisawa_solve(f.model, f.steps, f.n_steps, f.init_feet, f.com0, 7)
    assert a.tobytes() == c.tobytes()


def test_ragged_tail_repeats_the_last_sample_and_capacity(wg, solved):
    f, blocks, _ = solved[3]
    t0 = mf.t_start_of(f.model)
    lens = [wg.morisawa_length(f.model, int(n), t0) for n in f.n_steps]
    one, st = wg.morisawa_solve(f.model, f.steps, f.n_steps, f.init_feet, f.com0, 3)
    lcap = max(lens) + 3
    r = wg.morisawa_sample(one, st, 3, t0, f.model.T, lcap)
    assert list(r["length"]) == lens and len(set(lens)) > 1
    for b, L in enumerate(lens):
        for k in ("zmp_x", "zmp_y", "left_type", "right_type"):
            assert (r[k][L:, b] == r[k][L - 1, b]).all()
        for k in ("com", "left", "right"):
            assert (r[k][L:, :, b] == r[k][L - 1, :, b]).all()
    # a walk that does not fit: its code, its columns untouched; the others as before
    short = min(lens)
    canary = {k: np.full_like(r[k][:short], 77) for k in wg.MORISAWA_OUTPUTS}
    canary["length"] = np.full(f.B, 77, np.int32)
    q = wg.morisawa_sample(one, st, 3, t0, f.model.T, short, into=canary)
    for b, L in enumerate(lens):
        if L > short:
            assert q["length"][b] == wg.MORISAWA_CAPACITY and (q["zmp_x"][:, b] == 77).all() and (q["left"][:, :, b] == 77).all()
        else:
            assert q["length"][b] == L and np.array_equal(q["com"][:, :, b], r["com"][:short, :, b])


REFUSALS = ("one step", "too many steps", "t_double = 0", "NaN height", "omega dT > 40")


def refusal_fleet(wg, smax=14, B=5, seed=5):
    """a fleet whose gait 1 .. B - 1 are fine and whose gait 0 is broken in one of REFUSALS' ways by `spoil`"""
    return mf.Fleet(B, smax, seed)


def spoil(f, what):
    if what == "one step":
        f.n_steps[0] = 1
    elif what == "too many steps":
        f.n_steps[0] = f.smax + 1
    elif what == "t_double = 0":
        f.models[0].t_double = 0.0
    elif what == "NaN height":
        f.com0[0, 2] = float("nan")
    elif what == "omega dT > 40":
        f.com0[0, 2] = 0.01                     # omega = sqrt(9.86 / 0.01) = 31.4, times 3 t_single
    else:
        raise KeyError(what)


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_block_and_outputs_alone(wg, what):
    f = refusal_fleet(wg)
    good, st0 = wg.morisawa_solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, f.smax)
    assert list(st0) == [0] * f.B
    lcap = mf.lcap_for(f, True)
    spoil(f, what)
    blocks = np.full_like(good, 3.25)
    _, st = wg.morisawa_solve(f.models, f.steps, f.n_steps, f.init_feet, f.com0, f.smax, blocks=blocks)
    assert st[0] == wg.MORISAWA_BAD_INPUT and list(st[1:]) == [0] * (f.B - 1)
    assert (blocks[0] == 3.25).all() and blocks[1:].tobytes() == good[1:].tobytes()
    t0 = mf.t_start_of(f.model)
    ref = wg.morisawa_sample(good, st0, f.smax, t0, f.model.T, lcap)
    canary = {k: np.full_like(ref[k], 77) for k in wg.MORISAWA_OUTPUTS}
    canary["length"] = np.full(f.B, 77, np.int32)
    r = wg.morisawa_sample(blocks, st, f.smax, t0, f.model.T, lcap, into=canary)
    assert r["length"][0] == wg.MORISAWA_BAD_INPUT
    for k in wg.MORISAWA_OUTPUTS:
        assert (r[k][..., 0] == 77).all() and np.array_equal(r[k][..., 1:], ref[k][..., 1:]), k
    # without the statuses the sampler still refuses what is not a block
    r2 = wg.morisawa_sample(blocks, None, f.smax, t0, f.model.T, lcap, want=("zmp_x",))
    assert r2["length"][0] == wg.MORISAWA_BAD_INPUT and (r2["zmp_x"][:, 0] == 0).all()
