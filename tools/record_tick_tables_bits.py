#!/usr/bin/env python3
"""Records tests/golden/tick_tables_host_bits.npz: SHA-256 digests of the tick tables the HOST forms for a list of models
(tests/test_mpc_blocks_host.py holds wg_mpc_block to them).

    python tools/record_tick_tables_bits.py [--check]

The file in the tree was written from the serial loops of wg::build_tables as they stood before the arithmetic moved to
csrc/wg_tick_tables_math.hpp (wg_mpc_block on top of the untouched function): it is what says that the move kept every bit.
Re-record only when the tables are MEANT to change.  --check recomputes and compares without writing.

Per model: the digests of Sv, Sz, Uv, Uz, Qb, R2, Z2 (at the model's own N, as wg_mpc_block_unpack gives them) and of the sign
words; diag_b and blocks_ok as values; the digest of the wg_model_t itself (so that a change of tests/modelgen.py shows as
that, not as a change of the tables).  For a failed factor (blocks_ok == 0) R2, Z2 and the sign words are zero.  No GPU needed."""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PATH = os.path.join(ROOT, "tests", "golden", "tick_tables_host_bits.npz")
ARRAYS = ("Sv", "Sz", "Uv", "Uz", "Qb", "R2", "Z2", "sign")


def models():
    """[(name, model)]: every model of the seven sweeps, the default model at every horizon, and the model whose weights are all
    zero (accepted, but its constant block has no factor)"""
    import modelgen as mg
    out = []
    for name in mg.SWEEP_NAMES:
        out += [("%s/%s" % (name, mname), m) for mname, m in mg.sweep_models(name)]
    out += [("horizon/%d" % N, mg.horizon_model(N)) for N in range(2, 33)]
    z = mg.defaults(16)
    z.alpha = z.beta = z.gamma = 0.0
    out.append(("weights_zero", z))
    return out


def digests(wg, model):
    rc, blk = wg.mpc_block(model)
    assert rc == 0, rc
    u = wg.mpc_block_unpack(blk)
    return [hashlib.sha256(np.ascontiguousarray(u[k]).tobytes()).hexdigest() for k in ARRAYS], u["diag_b"], u["blocks_ok"]


def record():
    wg = importlib.import_module("jrl-walkgen_amd")
    ms = models()
    rows = [digests(wg, m) for _, m in ms]
    return dict(names=np.array([n for n, _ in ms]), arrays=np.array(ARRAYS), digests=np.array([r[0] for r in rows]),
                diag_b=np.array([r[1] for r in rows], dtype=np.float64), blocks_ok=np.array([r[2] for r in rows], dtype=np.int32),
                model_sha=np.array([hashlib.sha256(bytes(m)).hexdigest() for _, m in ms]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    new = record()
    if args.check:
        old = np.load(PATH)
        bad = [k for k in new if not np.array_equal(old[k], new[k])]
        print("differs: %s" % bad if bad else "%d models: same digests" % len(new["names"]))
        return 1 if bad else 0
    np.savez_compressed(PATH, **new)
    print("%s: %d models, %d with a failed factor" % (PATH, len(new["names"]), int((new["blocks_ok"] == 0).sum())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
