"""tests/gramref.py on the CPU: the reference, the bound and the model of the kernel's arithmetic that tests/test_gramian_gpu.py
holds wg_gramian_kernel to.  Three things are shown here, without a GPU:

  * the np.longdouble reference agrees with exact rational arithmetic to 2^-60 of the sum of its terms' magnitudes;
  * arithmetic of the kernel's kind -- operand type, one accumulator per entry, k in blocks of 4, the float64 epilogue -- stays
    within the bound for every N in 1 .. 32, both precisions and every weight set, so the bound does not refuse a correct kernel;
  * each way of breaking that arithmetic (gramref.FAULTS) leaves the bound, so the bound does refuse a wrong one."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gramref as gr  # noqa: E402

MODELS = (gr.REF_MODEL, (0.02, 0.5), (0.2, 1.0))          # the reference's, and the corners of the GPU test's (T, h) box
NS = range(1, 33)
PREC = {gr.F64: "f64", gr.F32: "f32"}


def excess(q, N, model, w, prec):
    """max over the entries of |q - exact| / bound (<= 1: within the bound)"""
    err = np.abs(q.astype(np.longdouble) - gr.exact(N, *model, *w, prec))
    bnd = gr.bound(N, *model, *w, prec)
    zero = bnd == 0                                         # e.g. off the diagonal under (0, 1, 0): nothing but an exact zero passes
    return float(np.where(zero, np.where(err == 0, 0.0, np.inf), err / np.where(zero, 1, bnd)).max())


def test_operands_are_the_reference_expressions():
    """spot values, written out as rigid-body-system.cpp:407 and :440 write them"""
    T, h = gr.REF_MODEL
    uv, uz = gr.operands(5, T, h, gr.F64)
    assert uv[3, 1] == (2 * (3 - 1) + 1) * T * T * 0.5 and uv[1, 3] == 0.0 and uv[0, 0] == 1 * T * T * 0.5
    assert uz[4, 1] == (1 + 3 * (4 - 1) + 3 * (4 - 1) * (4 - 1)) * T * T * T / 6.0 - T * h / 9.81 and uz[1, 4] == 0.0
    uv32, uz32 = gr.operands(5, T, h, gr.F32)
    assert uv32[3, 1] == float(np.float32(uv[3, 1])) and uz32[4, 1] == float(np.float32(uz[4, 1])) and uz32[4, 1] != uz[4, 1]
    many = gr.operands(5, np.array([T, 0.05]), np.array([h, 0.6]), gr.F64)
    assert many[0].shape == (2, 5, 5) and np.array_equal(many[0][0], uv) and np.array_equal(many[1][0], uz)


@pytest.mark.parametrize("prec", [gr.F64, gr.F32], ids=PREC.values())
def test_longdouble_reference_agrees_with_rational_arithmetic(prec):
    """N = 32, the reference's model and weights: |longdouble - Fraction| <= 2^-60 (beta delta + alpha |Uv|'|Uv| + gamma |Uz|'|Uz|),
    entrywise -- relative to the magnitudes that are summed, the only scale on which a sum with cancellation can be accurate"""
    N, w = 32, gr.WEIGHTS[3]
    assert np.finfo(np.longdouble).nmant >= 63
    ld = gr.exact(N, *gr.REF_MODEL, *w, prec)
    fr = gr.exact_fraction(N, *gr.REF_MODEL, *w, prec)
    uv, uz = (np.abs(u).astype(np.longdouble) for u in gr.operands(N, *gr.REF_MODEL, prec))
    scale = w[1] * np.eye(N) + w[0] * (uv.T @ uv) + w[2] * (uz.T @ uz)
    worst = 0.0
    for i in range(N):
        for j in range(N):
            err = abs(Fraction(*ld[i, j].as_integer_ratio()) - fr[i][j])
            worst = max(worst, float(err / Fraction(float(scale[i, j]))))
    print("%s: longdouble against Fraction, worst relative difference 2^%.1f" % (PREC[prec], np.log2(worst) if worst else -np.inf))
    assert worst <= 2.0 ** -60


@pytest.mark.parametrize("prec", [gr.F64, gr.F32], ids=PREC.values())
def test_arithmetic_of_the_kernels_kind_is_within_the_bound(prec):
    worst = (0.0, None)
    for model in MODELS:
        for N in NS:
            for w in gr.WEIGHTS:
                q = gr.emulate(N, *model, *w, prec)
                assert q.shape == (N, N) and np.isfinite(q).all()
                x = excess(q, N, model, w, prec)
                assert x <= 1.0, (x, model, N, w)
                if x >= worst[0]:
                    worst = (x, (model, N, w))
    print("%s: the clean emulation uses at most %.3f of the bound (%s)" % (PREC[prec], worst[0], worst[1]))


def caught(fault, prec):
    """{weights: [N at which the fault leaves the bound for the reference's model]}"""
    return {w: [N for N in NS if excess(gr.emulate(N, *gr.REF_MODEL, *w, prec, fault=fault), N, gr.REF_MODEL, w, prec) > 1.0]
            for w in gr.WEIGHTS}


@pytest.mark.parametrize("fault", gr.FAULTS)
def test_every_fault_leaves_the_bound(fault):
    """Each fault is outside the bound for at least one (N, weights), in every precision it exists in; "no_uz" and "short_k" also
    under the reference's own weights (1, 1e-5, 1e-6).

    What the bound can and cannot see of "no_uz" under those weights in f32: gamma Uz'Uz is 1e-6 of a term that is itself smaller
    than Uv'Uv, and the f32 bound is (2 N + 2) 2^-23 of alpha |Uv|'|Uv|, so a missing CoP term is visible only while N is small
    (the N printed below); at N = 16, the benchmark's horizon, it is not, and only the weights (0, 0, 1) show it there.  This is
    the arithmetic's resolution, not the test's: the f32 form cannot tell either.  The f64 bound sees it at every N."""
    ref_w = gr.WEIGHTS[3]
    for prec in (gr.F64, gr.F32):
        got = caught(fault, prec)
        print("%s, %s: caught at %s" % (fault, PREC[prec], {w: (ns if len(ns) < 8 else "%d N: %s .. %s" % (len(ns), ns[:3], ns[-3:]))
                                                            for w, ns in got.items()}))
        if fault == "f64_rows_in_f32" and prec == gr.F64:
            assert not any(got.values())                   # the fault is in the f32 path only
            continue
        assert any(got.values()), (fault, prec)
        # the identity term alone passes through every fault but the row permutation, which moves the diagonal
        assert got[(0.0, 1.0, 0.0)] == (list(range(2, 33)) if fault == "f64_rows_in_f32" else [])
        if fault in ("no_uz", "short_k"):
            assert got[ref_w], (fault, prec)
        if fault == "no_uz":
            assert got[(0.0, 0.0, 1.0)] == list(NS)        # the CoP term alone: at every N
            if prec == gr.F64:
                assert got[ref_w] == list(NS)
        if fault == "short_k":                             # every N that is no multiple of 4, under the reference's weights too
            assert got[(1.0, 0.0, 0.0)] == got[ref_w] == [N for N in NS if N % 4]
        if fault == "transposed_tile":                     # visible once there is a second tile
            assert got[(1.0, 0.0, 0.0)] == list(range(17, 33))
        if fault == "f64_rows_in_f32":
            assert got[(1.0, 0.0, 0.0)] == list(range(2, 33))
