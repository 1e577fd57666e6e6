"""The horizon-condensing Gramian on the matrix cores (wg_gramian_batch, SURVEY 8(a) a2 / BASELINE config 5's MFMA
path) against the oracle's loop in the reference's summation order.  MFMA fuses and reorders the sums, so this is a
floating-point check with a stated tolerance: 1e-14 of the block's largest entry for v_mfma_f64, 1e-6 for the
f32-operand form (operands are rounded to float).

Those tolerances are of the block's largest entry and hide the CoP term under the reference's weights (gamma Uz'Uz is 3e-7 of
max |Q_b| at N = 16).  The sweep below holds every entry to tests/gramref.py instead: a reference of the same operation on the
same operands in np.longdouble, and an entrywise bound derived from the number of roundings (its docstring; shown on the CPU in
tests/test_gramian_ref.py, where each way of breaking the kernel's arithmetic leaves it) -- every N in 1 .. 32, both precisions,
and weight sets that take the three terms one at a time."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gramref as gr  # noqa: E402
import oraclelib as ol  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu
TOL = {wg.GRAMIAN_F64: 1e-14, wg.GRAMIAN_F32: 1e-6}


def _oracle_qb(N, T, h, alpha, beta, gamma):
    lib = ol.oracle()
    m = wg.Model()
    lib.wgo_model_defaults(C.byref(m))
    m.N, m.T, m.com_height_qp, m.alpha, m.beta, m.gamma = N, T, h, alpha, beta, gamma
    Qb = np.zeros((N, N))
    assert lib.wgo_invariant_hessian(C.byref(m), Qb.ctypes.data_as(C.c_void_p)) == 0
    return Qb


@pytest.mark.parametrize("N", [16, 32, 8, 20, 1])
@pytest.mark.parametrize("prec", [wg.GRAMIAN_F64, wg.GRAMIAN_F32])
def test_gramian_matches_reference_order_loop(N, prec):
    wg.init(0)
    rng = np.random.default_rng(N)
    B = 37
    T = rng.uniform(0.02, 0.2, B); h = rng.uniform(0.5, 1.0, B)
    T[0], h[0] = 0.1, 0.814                                      # the reference's model
    alpha, beta, gamma = 1.0, 1e-5, 1e-6                         # ZMPVelocityReferencedQP.cpp:94-96 weights
    Qb = wg.gramian_batch(N, T, h, alpha, beta, gamma, prec)
    for b in range(B):
        want = _oracle_qb(N, T[b], h[b], alpha, beta, gamma)
        assert np.abs(Qb[b] - want).max() <= TOL[prec] * np.abs(want).max(), (b, N)
        assert np.array_equal(Qb[b], Qb[b].T) or np.abs(Qb[b] - Qb[b].T).max() <= TOL[prec] * np.abs(want).max()


def test_gramian_weights_enter_like_the_reference():
    """beta only on the diagonal, alpha / gamma scale the two products (generator-vel-ref.cpp:592-613)"""
    wg.init(0)
    T = np.array([0.1]); h = np.array([0.814])
    q_v = wg.gramian_batch(16, T, h, 1.0, 0.0, 0.0)[0]
    q_z = wg.gramian_batch(16, T, h, 0.0, 0.0, 1.0)[0]
    q_j = wg.gramian_batch(16, T, h, 0.0, 1.0, 0.0)[0]
    assert np.array_equal(q_j, np.eye(16))
    q = wg.gramian_batch(16, T, h, 2.0, 3.0, 5.0)[0]
    assert np.abs(q - (3.0 * q_j + 2.0 * q_v + 5.0 * q_z)).max() <= 1e-14 * np.abs(q).max()
    assert wg.lib().wg_gramian_batch(1, 33, T.ctypes.data, h.ctypes.data, 1.0, 1.0, 1.0, 0, q.ctypes.data) == -2


# ---- every entry against a reference of the same operation, within a derived bound ---------------------------------------------
B_SWEEP = 37


def sweep_models():
    """T in [0.02, 0.2], h in [0.5, 1.0]; model 0 is the reference's"""
    rng = np.random.default_rng(2025)
    T = rng.uniform(0.02, 0.2, B_SWEEP); h = rng.uniform(0.5, 1.0, B_SWEEP)
    T[0], h[0] = gr.REF_MODEL
    return T, h


@pytest.mark.parametrize("weights", gr.WEIGHTS, ids=["alpha", "gamma", "beta", "reference"])
@pytest.mark.parametrize("prec", [wg.GRAMIAN_F64, wg.GRAMIAN_F32], ids=["f64", "f32"])
def test_gramian_every_entry_within_the_derived_bound(prec, weights):
    """|Q_gpu - exact| <= bound entrywise (tests/gramref.py), and Q_gpu == Q_gpu' exactly: entries (i, j) and (j, i) are sums of the
    same products of the same operands -- a product does not depend on the order of its factors -- taken in the same order of k."""
    wg.init(0)
    assert (wg.GRAMIAN_F64, wg.GRAMIAN_F32) == (gr.F64, gr.F32)
    T, h = sweep_models()
    worst = (0.0, None)
    for N in range(1, 33):
        Qb = wg.gramian_batch(N, T, h, *weights, prec)
        assert Qb.shape == (B_SWEEP, N, N)
        err = np.abs(Qb.astype(np.longdouble) - gr.exact(N, T, h, *weights, prec))
        bnd = gr.bound(N, T, h, *weights, prec)
        used = np.where(bnd == 0, np.where(err == 0, 0.0, np.inf), err / np.where(bnd == 0, 1, bnd))
        b, i, j = np.unravel_index(np.argmax(used), used.shape)
        if used[b, i, j] >= worst[0]:
            worst = (float(used[b, i, j]), (N, int(b), int(i), int(j), float(Qb[b, i, j]), float(err[b, i, j]), float(bnd[b, i, j])))
        assert used[b, i, j] <= 1.0, "N %d model %d entry (%d, %d): %r, off by %.3e, bound %.3e" % (
            N, b, i, j, Qb[b, i, j], err[b, i, j], bnd[b, i, j])
        assert np.array_equal(Qb, Qb.transpose(0, 2, 1)), N
    print("largest |Q_gpu - exact| / bound: %.3f at (N, model, i, j, value, error, bound) = %s" % worst)


@pytest.mark.parametrize("prec", [wg.GRAMIAN_F64, wg.GRAMIAN_F32], ids=["f64", "f32"])
def test_gramian_dev_entry_on_a_stream_gives_the_bytes_of_the_host_entry(prec):
    """wg_gramian_batch_dev: device pointers, a stream that is not the default one"""
    import torch
    wg.init(0)
    T, h = sweep_models()
    w = gr.WEIGHTS[3]
    dT, dh = torch.from_numpy(T).cuda(), torch.from_numpy(h).cuda()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    for N in (1, 17, 32):
        want = wg.gramian_batch(N, T, h, *w, prec)
        dQ = torch.full((B_SWEEP, N, N), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()                       # the inputs and the fill are there before the side stream reads them
        rc = wg.lib().wg_gramian_batch_dev(B_SWEEP, N, dT.data_ptr(), dh.data_ptr(), *w, prec, dQ.data_ptr(), side.cuda_stream)
        assert rc == 0, wg.lib().wg_last_error()
        side.synchronize()
        assert dQ.cpu().numpy().tobytes() == want.tobytes(), N


def test_gramian_dev_entry_empty_batch_and_refusals():
    import torch
    wg.init(0)
    T, h = sweep_models()
    dT, dh = torch.from_numpy(T).cuda(), torch.from_numpy(h).cuda()
    dQ = torch.full((B_SWEEP, 32, 32), -7.25, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    fn = wg.lib().wg_gramian_batch_dev
    assert fn(0, 16, dT.data_ptr(), dh.data_ptr(), 1.0, 1.0, 1.0, wg.GRAMIAN_F64, dQ.data_ptr(), stream) == 0      # B = 0: nothing to do
    assert fn(B_SWEEP, 33, dT.data_ptr(), dh.data_ptr(), 1.0, 1.0, 1.0, wg.GRAMIAN_F64, dQ.data_ptr(), stream) == -2
    assert fn(B_SWEEP, 0, dT.data_ptr(), dh.data_ptr(), 1.0, 1.0, 1.0, wg.GRAMIAN_F64, dQ.data_ptr(), stream) == -2
    assert fn(B_SWEEP, 16, dT.data_ptr(), dh.data_ptr(), 1.0, 1.0, 1.0, 2, dQ.data_ptr(), stream) == -2            # unknown precision
    assert fn(B_SWEEP, 16, None, dh.data_ptr(), 1.0, 1.0, 1.0, wg.GRAMIAN_F64, dQ.data_ptr(), stream) == -2
    torch.cuda.synchronize()
    assert (dQ == -7.25).all().item()                  # none of them wrote anything
