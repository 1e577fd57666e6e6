"""wg_mpc_blocks_batch_dev / wg_mpc_blocks_batch: the blocks of many models made on the device, one wavefront per model, against
the host's wg_mpc_block -- as bytes.  csrc/wg_tick_tables_math.hpp is one text for both sides; these tests say that the 64
lanes of a wave give what the host's single lane gives, for models at every layout edge, refused ones included."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modelgen as mg  # noqa: E402
from test_mpc_blocks_host import refused_models, weights_zero_model  # noqa: E402

wg = importlib.import_module("jrl-walkgen_amd")
pytestmark = pytest.mark.gpu
CANARY = 0xA5


def good_models():
    """the 14 models of sweeps "16c" and "16e", the default model at the horizons tests/test_models_gpu.py names as layout edges,
    and the all-weights-zero model (accepted, no factor)"""
    out = [("%s/%s" % (s, n), m) for s in ("16c", "16e") for n, m in mg.sweep_models(s)]
    out += [("horizon/%d" % N, mg.horizon_model(N)) for N in (2, 3, 12, 13, 16, 29, 32)]
    out.append(("weights_zero", weights_zero_model()))
    return out


def _device_blocks(models, pad=256):
    """one launch of wg_mpc_blocks_batch_dev over `models` into a canary-filled buffer with `pad` bytes in front and behind:
    (blocks [M, bytes] uint8, status [M], the two pads)"""
    M, nb = len(models), wg.mpc_block_bytes()
    arr = (wg.Model * M)(*models)
    d_models = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    buf = torch.full((pad + M * nb + pad,), CANARY, dtype=torch.uint8, device="cuda")
    status = torch.full((M + 2,), 77, dtype=torch.int32, device="cuda")
    wg.mpc_blocks_batch_dev(M, d_models.data_ptr(), buf.data_ptr() + pad, status.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    st = status.cpu().numpy()
    assert st[0] == 77 and st[-1] == 77
    return h[pad:pad + M * nb].reshape(M, nb), st[1:-1], (h[:pad], h[pad + M * nb:])


def test_device_blocks_are_the_hosts_bytes():
    wg.init(0)
    ms = good_models()
    assert len(ms) == 22
    dev, status, pads = _device_blocks([m for _, m in ms])
    assert (status == 0).all(), status
    for k, (name, m) in enumerate(ms):
        rc, host = wg.mpc_block(m)
        assert rc == 0, name
        if dev[k].tobytes() != host.tobytes():
            bad = np.flatnonzero(dev[k].view(np.uint64) != host.view(np.uint64))
            raise AssertionError("%s: %d words differ, first at byte %d" % (name, bad.size, 8 * bad[0]))
    assert (pads[0] == CANARY).all() and (pads[1] == CANARY).all()
    assert wg.mpc_block_unpack(dev[-1])["blocks_ok"] == 0 and wg.mpc_block_unpack(dev[0])["blocks_ok"] == 1


def test_refused_models_between_good_ones():
    """M = 9, good and refused models interleaved: status is the host's return code, a refused block is all zero, and no wave
    writes outside its block -- the pads in front of and behind the blocks keep their canary, and every block's own padding
    (behind the tables, between the model and the tables) is zero, not a neighbour's bytes."""
    wg.init(0)
    bad = dict(refused_models())
    good = good_models()
    ms = [good[0][1], bad["N = 33"], good[9][1], bad["NaN com_height_qp"], bad["N = 16, five previewed steps"], good[20][1],
          bad["Gramian flag 2"], bad["infinite alpha"], good[14][1]]
    assert len(ms) == 9
    dev, status, pads = _device_blocks(ms)
    host = [wg.mpc_block(m) for m in ms]
    assert list(status) == [rc for rc, _ in host] and sorted(set(status)) == [-2, 0]
    end = wg.MPC_BLOCK_TABLES + wg.MPC_BLOCK_TABLES_BYTES
    for k, (rc, blk) in enumerate(host):
        assert dev[k].tobytes() == blk.tobytes(), k
        if rc:
            assert not dev[k].any(), k
        assert not dev[k][end:].any() and not dev[k][C.sizeof(wg.Model):wg.MPC_BLOCK_TABLES].any(), k
    assert (pads[0] == CANARY).all() and (pads[1] == CANARY).all()


def test_the_host_pointer_form_gives_the_same_bytes():
    wg.init(0)
    ms = [m for _, m in good_models()[:3]] + [refused_models()[0][1]]
    blocks, status = wg.mpc_blocks_batch(ms)
    assert list(status) == [0, 0, 0, -2]
    for k, m in enumerate(ms):
        assert blocks[k].tobytes() == wg.mpc_block(m)[1].tobytes(), k
