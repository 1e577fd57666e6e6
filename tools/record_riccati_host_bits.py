#!/usr/bin/env python3
"""Record what the host call wg_riccati_gains returns, bit for bit, into tests/golden/riccati_host_bits.npz.

The fixture was recorded from the library as it stood BEFORE the Riccati arithmetic moved into csrc/wg_riccati_math.hpp (the
text the fleet kernel shares); tests/test_riccati_batch_host.py holds every later build to it.  Run it again only against a
build whose host results are known to be right:

    python tools/record_riccati_host_bits.py [path/to/libwg_mpc.so] [out.npz]

Eight cases: T in {0.005, 0.01} x zc in {0.6, 0.814} x both modes, Nl = 320, Q = 1 and the reference's R per mode.
No device is needed: wg_riccati_gains is host arithmetic.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 320
CASES = [(T, zc, mode) for T in (0.005, 0.01) for zc in (0.6, 0.814) for mode in (0, 1)]


def r_of(mode):
    return 1e-6 if mode == 1 else 1e-5           # PreviewControl.cpp: R of WITHOUT_INITIALPOS / WITH_INITIALPOS


def record(lib_path):
    sys.path.insert(0, ROOT)
    lib = importlib.import_module("jrl-walkgen_amd").bind(C.CDLL(lib_path))      # signatures from include/wg_mpc.h
    K = np.zeros((len(CASES), 4))
    F = np.zeros((len(CASES), NL))
    for i, (T, zc, mode) in enumerate(CASES):
        rc = lib.wg_riccati_gains(T, zc, 1.0, r_of(mode), NL, mode, K[i].ctypes.data, F[i].ctypes.data)
        assert rc == 0, (T, zc, mode, rc)
    return K, F


if __name__ == "__main__":
    lib_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "jrl-walkgen_amd", "lib", "libwg_mpc.so")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "riccati_host_bits.npz")
    K, F = record(lib_path)
    np.savez(out, cases=np.array(CASES, dtype=np.float64), K=K.view(np.uint64), F=F.view(np.uint64))
    print("recorded %d cases of Nl = %d from %s into %s" % (len(CASES), NL, lib_path, out))
