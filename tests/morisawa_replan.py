"""Plans for tests/test_morisawa_resolve_host.py and tests/test_morisawa_resolve_gpu.py: the gaits of tests/morisawa_fleets.py put on
one timing -- one model, one CoM height, S steps each -- so that they differ in what a re-plan may change (steps, initial feet,
start CoM x and y) and in nothing that Z depends on."""
import numpy as np

import morisawa_fleets as mf

HEIGHT = 0.7116911                # the golden walk's
PATTERN = 3.25                    # what blocks hold before a call that may refuse them


class Family:
    """the short or the long family's wrappers under one set of names"""

    def __init__(self, long_):
        w = mf.wg()
        p = "morisawa_long_" if long_ else "morisawa_"
        self.long = long_
        self.name = "wg_" + p
        for k in ("solve", "resolve", "view", "block_bytes", "sample", "solve_dev", "resolve_dev", "sample_dev", "walk_dev", "length"):
            setattr(self, k, getattr(w, p + k))

    def words(self, smax):
        return self.block_bytes(smax) // 8


def plans(B, smax, S, seed, height=HEIGHT):
    """B plans of S steps at one height on the default model; f.models: the same times with a step height and an omega per gait"""
    f = mf.Fleet(B, smax, seed)
    f.n_steps[:] = S
    f.com0[:, 2] = height
    for b in range(B):
        f.models[b].t_single, f.models[b].t_double = f.model.t_single, f.model.t_double
    return f


def swaps(view):
    return int(sum(int(p) != k for k, p in enumerate(view["piv"])))


def ulp_up(x):
    return float(np.nextafter(x, np.inf))
