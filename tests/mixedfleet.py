"""Herdt fleets with a model per gait at queue-loading sizes, stated once (test infrastructure, no tests in this file).

Four kinds of fleet, each larger than the waves the device keeps resident, so that the launchers of wg_mpc_tick_fleet_dev and
wg_mpc_run_fleet_dev leave their trivial branches: several gaits per wave, rings that fill, the keep rule, the start order.

    kind       base (launch shape)    good models                                                     M    B     ticks, redraw
    compact    mg.defaults(16)        sweep "16c" + 57 random models on the 16c grid                  64   2600  32, 8
    element16  sweep "16e" model 0    sweep "16e" + 9 random (16e grid) + sweep "16c" + 9 random (16c) 32   3300  32, 8
    n12        sweep "12" model 0     sweep "12" + 9 random                                           16   3300  32, 8
    n32        sweep "32" model 0     sweep "32" + 9 random                                           16   3300  24, 6

Gait g runs with model (29 g) % M: 29 is coprime to every M, so neighbours differ and any M consecutive gaits hold every model
once.  It starts from the start pose of its own model and follows mg.gait_velocity([900, (29 g) % M], g, STRETCHES), set
every `redraw` ticks; the clock advances by w.advance_calls(t).

Every gait with g % 101 == 50 is refused, in turn by each way wg_mpc_fleet_block knows: model_of = -1; model_of = the number of
blocks; an all-zero block; a good block of another N; and, in the compact launch only, a good block of the four-step class.  The
extra blocks stand behind the M good ones.  A refused gait keeps the start pose and the references of the model it would have
had.

The seeds of the random models were chosen on the oracle alone (tests/test_mpc_fleet_scale_oracle.py asserts what they were
chosen for): at most a tenth of the (model, gait) pairs of a kind hold a tick whose QP fails, and any two models that follow
each other in a kind's list take one gait to different states.

Nothing here touches the GPU: the binding is imported for its POD layouts only, start poses come from the oracle's
wgo_gait_init (byte-identical to wg_gait_init, see tests/modelgen.py)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import modelgen as mg  # noqa: E402
import workload as w  # noqa: E402

KINDS = ("compact", "element16", "n12", "n32")
STRETCHES = ("walk", "turn", "stop", "walk")
WALKING = (0, 1, 3)                                             # the stretches with a reference other than zero
STRIDE = 29                                                     # model_of[g] = (STRIDE * g) % M
REFUSE_EVERY, REFUSE_AT = 101, 50                               # gait g is refused when g % 101 == 50
VEL_SEED = 900
# (sweep whose step-period grid the models are drawn on): the seeds of mg.random_model, from 100 upwards
SEEDS = {"compact": {"16c": tuple(range(100, 157))},
         "element16": {"16e": tuple(range(100, 109)), "16c": tuple(range(100, 109))},
         "n12": {"12": tuple(range(100, 109))},
         "n32": {"32": tuple(range(100, 109))}}
_SHAPE = {"compact": (2600, 32, 8), "element16": (3300, 32, 8), "n12": (3300, 32, 8), "n32": (3300, 24, 6)}   # B, ticks, redraw


def _grid(sweep):
    _, N, (lo, hi), _, _ = mg.SWEEP[mg.SWEEP_NAMES.index(sweep)]
    return N, mg.step_periods_for(N, lo=lo, hi=hi)


def _models(sweep, seeds):
    """the seven models of a sweep, then one random model per seed on that sweep's step-period grid"""
    N, grid = _grid(sweep)
    return [m for _, m in mg.sweep_models(sweep)] + [mg.random_model(s, N, step_periods=grid) for s in seeds]


class Kind:
    """One kind of fleet: base, models [M] (the good ones), extras [(way of refusal, model or None for an all-zero block)],
    model_of [B] int32 as the launch gets it, own [B] (the good model a gait has, or would have had), accepted [B] bool,
    refusal {g: way}, vel [ticks / redraw, B, 3], and the start states."""

    def __init__(self, name):
        self.name = name
        self.B, self.ticks, self.redraw = _SHAPE[name]
        self.models = [m for sweep, seeds in SEEDS[name].items() for m in _models(sweep, seeds)]
        self.M = M = len(self.models)
        self.base = mg.defaults(16) if name == "compact" else self.models[0]
        self.N = self.base.N
        other_n = mg.defaults(16) if self.N == 12 else mg.horizon_model(12)
        self.extras = [("zero block", None), ("another N", other_n)]
        if name == "compact":
            self.extras.append(("four-step class", mg.sweep_models("16e")[0][1]))
        self.n_blocks = M + len(self.extras)
        ways = [("model_of = -1", -1), ("model_of = number of blocks", self.n_blocks)] + \
               [(what, M + k) for k, (what, _) in enumerate(self.extras)]
        g = np.arange(self.B)
        self.own = (STRIDE * g) % M
        self.accepted = g % REFUSE_EVERY != REFUSE_AT
        self.model_of = self.own.astype(np.int32)
        self.refusal = {}
        for j, r in enumerate(np.flatnonzero(~self.accepted)):
            what, mo = ways[j % len(ways)]
            self.model_of[r] = mo
            self.refusal[int(r)] = what
        self.n_seg = self.ticks // self.redraw
        assert self.n_seg == len(STRETCHES) and self.n_seg * self.redraw == self.ticks
        self.vel = np.stack([mg.gait_velocity([VEL_SEED, int(self.own[k])], int(k), STRETCHES) for k in g], 1)     # [n_seg, B, 3]

    @functools.cached_property
    def model_starts(self):
        """the start state's bytes of every good model"""
        return [w.state_bytes(mg.start_state(m)) for m in self.models]

    def start_of(self, g):
        return self.model_starts[int(self.own[g])]

    def starts(self, gaits=None):
        """the start states of the listed gaits (default: all), one after the other"""
        return b"".join(self.start_of(g) for g in (range(self.B) if gaits is None else gaits))

    def oracle_models(self):
        """what fleet_oracle.submit_fleet takes: the bytes of every good model, None for the blocks no gait may run with"""
        return [bytes(m) for m in self.models] + [None] * len(self.extras)

    def two_per_model(self):
        """the first two accepted gaits of every model, in gait order: gaits 0 .. 2 M - 1, but for a refused gait among them,
        whose model's next gait (M further on) stands in"""
        picked = []
        for k in range(self.M):
            picked += [int(x) for x in np.flatnonzero(self.accepted & (self.own == k))[:2]]
        return sorted(picked)

    def walking_ticks(self):
        return np.array([t for t in range(self.ticks) if t // self.redraw in WALKING])


@functools.lru_cache(maxsize=None)
def kind(name):
    return Kind(name)
