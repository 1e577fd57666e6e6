#!/usr/bin/env python3
"""Record what DimitrovHost::build (the host arithmetic of wg_dimitrov_configure) produces, bit for bit, into
tests/golden/dimitrov_host_bits.npz.

The fixture was recorded from csrc/wg_dimitrov_device.hpp as it stood BEFORE the arithmetic of InitConstants moved into
csrc/wg_dimitrov_math.hpp (the text the constants kernel shares); tests/test_dimitrov_constants_host.py holds every later build
to it.  Run it again only against a tree whose host results are known to be right:

    python tools/record_dimitrov_host_bits.py [path/to/csrc] [out.npz]

No device and no library are needed: a small stand-alone program is compiled against the header (hipcc, the library's own
flags -- contraction off) and calls wg::DimitrovHost::build for every model of MODELS.

The fixture: `models` [n][6] (N, T, Tctrl, com_height, alpha, beta), `ok` [n], `sha256` [n][11][32] -- the digest of each
array's little-endian doubles, in the order of ARRAYS, at the size the model uses -- and, for the models of `full`, the arrays
themselves as `m<i>_<name>` (uint64 views).
"""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
         "-Wno-pass-failed"]

# name, rows, columns as functions of N (n = 2N); the first six are wg_dimitrov_get_constants', the next four
# wg_dimitrov_get_qld_constants', the last PLDPSolver::PrecomputeiPuPx
ARRAYS = [("iLQ", lambda N: (2 * N, 2 * N)), ("OptB", lambda N: (2 * N, 6)), ("OptC", lambda N: (2 * N, 2 * N)),
          ("Pu", lambda N: (N, N)), ("iPu", lambda N: (N, N)), ("Px", lambda N: (N, 3)),
          ("Q", lambda N: (2 * N, 2 * N)), ("OptBq", lambda N: (2 * N, 6)), ("OptCq", lambda N: (2 * N, 2 * N)),
          ("PuT", lambda N: (N, N)), ("iPuPx", lambda N: (2 * N, 6))]


def models():
    """The defaults first, then N x height x (alpha, beta) x T; Tctrl = T / 20."""
    out = [(16, 0.1, 0.005, 0.80, 200.0, 1000.0)]
    for N in (1, 2, 7, 15, 16):
        for h in (0.6, 0.8, 0.95):
            for a, b in ((200.0, 1000.0), (1.0, 1.0), (1e4, 10.0)):
                for T in (0.05, 0.1):
                    out.append((N, T, T / 20, h, a, b))
    return out


MODELS = models()
# the arrays in full: the defaults, a small odd horizon with flat weights, a long one with heavy velocity weight
FULL = [0, MODELS.index((7, 0.05, 0.05 / 20, 0.6, 1.0, 1.0)), MODELS.index((15, 0.1, 0.1 / 20, 0.95, 1e4, 10.0))]

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include <hip/hip_runtime.h>
#include "wg_dimitrov_device.hpp"

// stdin: one model per line (N T Tctrl h alpha beta, doubles in hex float).  stdout, binary, per model: int ok, then the
// arrays at the model's own sizes in the recorder's order.
static void put(const double *p, size_t rows, size_t cols, size_t) { fwrite(p, sizeof(double), rows * cols, stdout); }
int main() {
  std::unique_ptr<wg::DimitrovConst> K(new wg::DimitrovConst);
  int N;
  double T, Tc, h, a, b;
  while (scanf("%d %la %la %la %la %la", &N, &T, &Tc, &h, &a, &b) == 6) {
    wg_dimitrov_model_t m;
    memset(&m, 0, sizeof m);
    m.N = N; m.solver = 0; m.T = T; m.Tctrl = Tc; m.com_height = h; m.alpha = a; m.beta = b;
    memset(K.get(), 0, sizeof *K);
    const int ok = wg::DimitrovHost::build(m, *K) ? 1 : 0;
    fwrite(&ok, sizeof ok, 1, stdout);
    const size_t n = 2 * (size_t)N;
    put(K->iLQ, n, n, 0); put(K->OptB, n, 6, 0); put(K->OptC, n, n, 0);
    put(K->pldp.Pu, N, N, 0); put(K->pldp.iPu, N, N, 0); put(K->pldp.Px, N, 3, 0);
    put(K->Qq, n, n, 0); put(K->OptBq, n, 6, 0); put(K->OptCq, n, n, 0); put(K->PuTq, N, N, 0);
    put(K->pldp.iPuPx, n, 6, 0);
  }
  return 0;
}
"""


def run_build(csrc, model_list):
    """[(ok, {name: float64 array})] of DimitrovHost::build as the header under `csrc` defines it."""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "dimitrov_bits.hip"), os.path.join(tmp, "dimitrov_bits")
        with open(src, "w") as f:
            f.write(PROGRAM)
        subprocess.run([HIPCC] + FLAGS + ["-I", csrc, "-o", exe, src], check=True)
        text = "".join("%d %s %s %s %s %s\n" % ((m[0],) + tuple(float(x).hex() for x in m[1:])) for m in model_list)
        raw = subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout
    out, at = [], 0
    for m in model_list:
        ok = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=at)[0])
        at += 4
        arrays = {}
        for name, shape in ARRAYS:
            r, c = shape(m[0])
            arrays[name] = np.frombuffer(raw, dtype="<f8", count=r * c, offset=at).reshape(r, c).copy()
            at += 8 * r * c
        out.append((ok, arrays))
    assert at == len(raw), (at, len(raw))
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).digest(), dtype=np.uint8)


if __name__ == "__main__":
    csrc = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "jrl-walkgen_amd", "csrc")
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "dimitrov_host_bits.npz")
    res = run_build(csrc, MODELS)
    sha = np.zeros((len(MODELS), len(ARRAYS), 32), dtype=np.uint8)
    for i, (ok, arrays) in enumerate(res):
        for j, (name, _) in enumerate(ARRAYS):
            sha[i, j] = digest(arrays[name])
    data = {"models": np.array(MODELS, dtype=np.float64), "ok": np.array([r[0] for r in res], dtype=np.int32), "sha256": sha,
            "full": np.array(FULL, dtype=np.int32)}
    for i in FULL:
        for name, _ in ARRAYS:
            data["m%d_%s" % (i, name)] = res[i][1][name].view(np.uint64)
    np.savez_compressed(out, **data)
    print("recorded %d models (%d built) from %s into %s" % (len(MODELS), int(sum(r[0] for r in res)), csrc, out))
