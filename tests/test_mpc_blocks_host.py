"""wg_mpc_block / wg_mpc_block_unpack on the host (no GPU): the tick tables of a model as an opaque block.

1. The host keeps its bits: tests/golden/tick_tables_host_bits.npz holds SHA-256 digests of every table for 81 models (all
   seven sweeps of tests/modelgen.py, the default model at every horizon 2 .. 32, the all-weights-zero model), recorded by
   tools/record_tick_tables_bits.py from the serial loops of wg::build_tables as they stood BEFORE the arithmetic moved to
   csrc/wg_tick_tables_math.hpp.  Every digest must match; for a failed factor R2 / Z2 / the sign words are zero (what the
   fixture records for them).
2. Q_b against the oracle's wgo_invariant_hessian (the reference of tests/test_gramian_gpu.py): bit equality.
3. Refusals: WG_ERR_BAD_ARG and an all-zero block.
4. All weights zero: accepted, blocks_ok == 0, R2 / Z2 / sign words zero.
5. Block shape: zeros behind the tables (and between the model and them), a multiple of 128 bytes, two calls the same bytes."""
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import modelgen as mg  # noqa: E402
import oraclelib as ol  # noqa: E402
import record_tick_tables_bits as rec  # noqa: E402
from test_models_oracle import FIRST_REFUSED  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
BAD_ARG = -2
GRAMIAN_FLAGS = (2, 4)                  # WG_FLAG_GRAMIAN_MFMA_F64, _F32


@pytest.fixture(scope="module")
def golden():
    g = np.load(rec.PATH)
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def blocks():
    """[(name, model, rc, block)] of the fixture's models, made once"""
    return [(name, m) + wg.mpc_block(m) for name, m in rec.models()]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_the_host_keeps_its_bits(golden, blocks):
    assert [n for n, _, _, _ in blocks] == list(golden["names"]) and len(blocks) == 81
    assert tuple(golden["arrays"]) == rec.ARRAYS
    failed = 0
    for k, (name, m, rc, blk) in enumerate(blocks):
        assert rc == 0, name
        assert hashlib.sha256(bytes(m)).hexdigest() == golden["model_sha"][k], "tests/modelgen.py changed model %s" % name
        u = wg.mpc_block_unpack(blk)
        assert bytes(u["model"]) == bytes(m), name
        for a, want in zip(rec.ARRAYS, golden["digests"][k]):
            assert _sha(u[a]) == want, (name, a)
        assert u["blocks_ok"] == golden["blocks_ok"][k], name
        assert np.float64(u["diag_b"]).tobytes() == golden["diag_b"][k].tobytes(), name
        if not u["blocks_ok"]:
            failed += 1
            assert not u["R2"].any() and not u["Z2"].any() and not u["sign"].any(), name
            assert not np.signbit(u["R2"]).any() and not np.signbit(u["Z2"]).any(), name
    assert failed == 1                                              # the all-weights-zero model alone


def test_qb_is_the_oracles_invariant_hessian_bit_for_bit(blocks):
    """wgo_invariant_hessian (oracle/herdt_oracle.c) sums in the reference's order, as the tables do: every entry of Q_b of
    every fixture model has the same bits (checked here on the CPU; largest relative difference 0)."""
    lib = ol.oracle()
    for name, m, rc, blk in blocks:
        N = m.N
        ref = np.zeros((N, N))
        assert lib.wgo_invariant_hessian(C.byref(m), ref.ctypes.data_as(C.c_void_p)) == 0
        got = wg.mpc_block_unpack(blk)["Qb"]
        assert got.tobytes() == ref.tobytes(), (name, np.abs(got - ref).max())


def refused_models():
    out = []
    for N in (1, 33):
        m = mg.defaults(16); m.N = N; out.append(("N = %d" % N, m))
    m = mg.defaults(16); m.Tctrl = m.T / 10.0; out.append(("T / Tctrl = 10", m))
    for N in (16, 32):
        m = mg.defaults(N); mg.set_step_period(m, FIRST_REFUSED[N]); out.append(("N = %d, five previewed steps" % N, m))
    m = mg.defaults(16); m.com_height_qp = float("nan"); out.append(("NaN com_height_qp", m))
    m = mg.defaults(16); m.alpha = float("inf"); out.append(("infinite alpha", m))
    for f in GRAMIAN_FLAGS:
        m = mg.defaults(16); m.flags |= f; out.append(("Gramian flag %d" % f, m))
    return out





def test_refused_models_give_bad_arg_and_an_all_zero_block():
    cases = refused_models()
    assert len(cases) == 9
    for what, m in cases:
        blk = np.full(wg.mpc_block_bytes(), 0xA5, dtype=np.uint8)
        rc = wg.lib().wg_mpc_block(C.byref(m), blk.ctypes.data_as(C.c_void_p))
        assert rc == BAD_ARG, (what, rc)
        assert not blk.any(), what
        assert wg.lib().wg_mpc_block_unpack(blk.ctypes.data_as(C.c_void_p), *([None] * 10)) == BAD_ARG, what


def weights_zero_model():
    m = mg.defaults(16)
    m.alpha = m.beta = m.gamma = 0.0
    return m


def test_all_weights_zero_is_accepted_without_a_factor():
    rc, blk = wg.mpc_block(weights_zero_model())
    assert rc == 0
    u = wg.mpc_block_unpack(blk)
    assert u["blocks_ok"] == 0 and u["diag_b"] == 1e-8
    assert not u["Qb"].any() and u["Uv"].any() and u["Uz"].any()
    for k in ("R2", "Z2", "sign"):
        assert not np.ascontiguousarray(u[k]).view(np.uint8).any(), k


def test_block_shape(blocks):
    nbytes = wg.mpc_block_bytes()
    assert nbytes % 128 == 0 and nbytes == 76032
    end = wg.MPC_BLOCK_TABLES + wg.MPC_BLOCK_TABLES_BYTES
    assert end <= nbytes < end + 128
    for name, m, rc, blk in blocks:
        assert blk.size == nbytes
        assert bytes(blk[:C.sizeof(wg.Model)]) == bytes(m), name
        assert not blk[C.sizeof(wg.Model):wg.MPC_BLOCK_TABLES].any() and not blk[end:].any(), name
        rc2, again = wg.mpc_block(m)
        assert rc2 == 0 and again.tobytes() == blk.tobytes(), name
    # the tables of a short horizon are zero behind the parts its N uses: nothing of a larger model can show through
    _, small = wg.mpc_block(mg.horizon_model(2))
    tabs = small[wg.MPC_BLOCK_TABLES:end].view(np.float64)
    assert np.count_nonzero(tabs[:2 * 96].reshape(2, 32, 3)[:, 2:]) == 0            # Sv, Sz rows >= N
    sq = tabs[2 * 96:2 * 96 + 3 * 1024].reshape(3, 32, 32)
    assert np.count_nonzero(sq[:, 2:, :]) == 0 and np.count_nonzero(sq[:, :, 2:]) == 0
