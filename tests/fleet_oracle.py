"""CPU checker pool for the fleet parity tests (test infrastructure, no tests in this file).

Every gait of a workload advanced on oracle/libwg_oracle_ptrig.so (the C restatement with the portable trigonometry: the
bit-exact partner of the kernels), split into chunks over spawned worker processes -- the QL restatement keeps statics, so
separate processes, never threads, and never fork.  A test queues the oracle first (submit), runs the GPU meanwhile and
collects the results afterwards (FleetJob.result).  A fleet with a model per gait goes through submit_fleet: grouped by model,
one or more chunks per model, the result back in gait order.

Workers are fresh interpreters that see only this module, numpy and ctypes: they never import torch, bench.py or the product's
binding, and never load libwg_mpc.so or the HIP runtime.  The parent builds the oracle once (build_oracle) and hands the
workers the model, the start states and the velocity references as bytes / arrays, and the struct layout as plain numbers
(layout_of).

Comparison is on 8-byte words of the raw structs: plain equality for healthy fleets; NaN-aware (a word matches if it is equal,
or if both words are NaNs, whatever their sign or payload: x86 gives 0xFFF8..., gfx950 0x7FF8...) where gaits are lost.  An
inf matches only the same inf.  Mismatches are reported by gait index, with the tick and the field where known."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
PTRIG_SO = os.path.join(ORACLE_DIR, "libwg_oracle_ptrig.so")
MAX_WORKERS = 16

_EXP = np.uint64(0x7FF0000000000000)
_MANT = np.uint64(0x000FFFFFFFFFFFFF)
CANONICAL_NAN = np.uint64(0x7FF8000000000000)


# ---------------------------------------------------------------------------------------------------------- parent side
def build_oracle():
    """Build both oracle libraries if a source is newer (parent only, before anything is submitted: no concurrent make)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oraclelib as ol
    ol.build_oracle()
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR, "libwg_oracle_ptrig.so"])
    return PTRIG_SO


def layout_of(wg):
    """The few offsets a worker needs, from the binding's ctypes structs (read in the parent)."""
    assert C.sizeof(wg.GaitState) % 8 == 0 and C.sizeof(wg.TickOut) % 8 == 0
    return {"state_size": C.sizeof(wg.GaitState), "out_size": C.sizeof(wg.TickOut),
            "clock_off": wg.GaitState.clock.offset, "vref_off": wg.GaitState.vref.offset,
            "diag_off": wg.TickOut.ifail.offset, "tctrl_off": wg.Model.Tctrl.offset}


def pool_size(bench):
    return max(1, min(MAX_WORKERS, bench.usable_cores()[0]))


def make_pool(workers):
    assert 1 <= workers <= MAX_WORKERS, workers
    return mp.get_context("spawn").Pool(workers)


class FleetJob:
    """Chunks of one workload in flight on a pool; result() gathers them in gait order."""

    def __init__(self, asyncs, n_gaits, n_ticks, keep_ticks, outs):
        self._asyncs, self.n_gaits, self.n_ticks, self.keep_ticks, self.outs = asyncs, n_gaits, n_ticks, keep_ticks, outs

    def done(self):
        """(chunks finished, chunks in all)"""
        return sum(a.ready() for a in self._asyncs), len(self._asyncs)

    def result(self, timeout=None):
        parts = [a.get(timeout) for a in self._asyncs]
        parts.sort(key=lambda p: p["g0"])
        assert sum(p["ng"] for p in parts) == self.n_gaits
        res = {"states": b"".join(p["states"] for p in parts),
               "diag": np.concatenate([p["diag"] for p in parts], axis=1),
               "workers": [p["worker"] for p in parts]}
        if self.outs == "raw":
            res["outs"] = {t: b"".join(p["outs"][t] for p in parts) for t in self.keep_ticks}
        else:
            res["outs"] = {t: np.concatenate([p["outs"][t] for p in parts]) for t in self.keep_ticks}
        return res


def submit(pool, layout, model_bytes, start, vel, redraw, n_ticks, keep_ticks=(), outs="raw", nan_aware=False, chunks=None):
    """Queue gaits [0, B) of a workload, B = vel.shape[1].  start: one state's bytes (every gait starts there) or B states'.
    vel: [n_seg, B, 3] references, gait g's stretch k at vel[k, g].  chunks: list of chunk sizes summing to B (default: four
    per MAX_WORKERS, so that a chunk of lost, slow gaits does not hold up the others).  outs: "raw" ships the kept ticks'
    wg_tick_out_t bytes, "digest" one digest per (tick, gait) -- NaNs canonicalised first with nan_aware."""
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    B = vel.shape[1]
    sz = layout["state_size"]
    assert len(start) in (sz, B * sz)
    assert outs in ("raw", "digest")
    if chunks is None:
        n = min(B, 4 * MAX_WORKERS)
        chunks = [B // n + (k < B % n) for k in range(n)]
    assert sum(chunks) == B and all(c > 0 for c in chunks)
    asyncs = []
    g0 = 0
    for ng in chunks:
        st = start if len(start) == sz else start[g0 * sz:(g0 + ng) * sz]
        args = (layout, bytes(model_bytes), bytes(st), np.ascontiguousarray(vel[:, g0:g0 + ng]), int(redraw), int(n_ticks),
                tuple(keep_ticks), outs, bool(nan_aware), g0)
        asyncs.append(pool.apply_async(advance, args))
        g0 += ng
    return FleetJob(asyncs, B, n_ticks, tuple(keep_ticks), outs)


class MixedFleetJob:
    """Chunks of a fleet with a model per gait in flight on a pool (submit_fleet); result() puts them back in gait order."""

    def __init__(self, asyncs, index, accepted, start, state_size, out_size, n_ticks, keep_ticks, outs):
        self._asyncs, self._index, self.accepted, self._start = asyncs, index, accepted, start
        self._sz, self._osz, self.n_ticks, self.keep_ticks, self.outs = state_size, out_size, n_ticks, keep_ticks, outs
        self.n_gaits = len(accepted)

    def done(self):
        """(chunks finished, chunks in all)"""
        return sum(a.ready() for a in self._asyncs), len(self._asyncs)

    def result(self, timeout=None):
        """states, diag [n_ticks, B, 6] and the kept outs of all B gaits in gait order, and `accepted` [B]: a gait that was
        not submitted holds its start state, zeros in diag and zeros in outs"""
        B, sz, osz = self.n_gaits, self._sz, self._osz
        states = np.frombuffer(self._start, dtype=np.uint8).reshape(B, sz).copy()
        diag = np.zeros((self.n_ticks, B, 6), dtype=np.int32)
        raw = self.outs == "raw"
        kept = {t: (np.zeros((B, osz), dtype=np.uint8) if raw else np.zeros(B, dtype=np.uint64)) for t in self.keep_ticks}
        workers = []
        for a in self._asyncs:
            p = a.get(timeout)
            idx = self._index[p["g0"]]
            assert p["ng"] == len(idx)
            states[idx] = np.frombuffer(p["states"], dtype=np.uint8).reshape(len(idx), sz)
            diag[:, idx] = p["diag"]
            for t in self.keep_ticks:
                kept[t][idx] = np.frombuffer(p["outs"][t], dtype=np.uint8).reshape(len(idx), osz) if raw else p["outs"][t]
            workers.append(p["worker"])
        return {"states": states.tobytes(), "diag": diag, "accepted": self.accepted.copy(), "workers": workers,
                "outs": {t: (v.tobytes() if raw else v) for t, v in kept.items()}}


def submit_fleet(pool, layout, models, model_of, start, vel, redraw, n_ticks, keep_ticks=(), outs="raw", nan_aware=False,
                 chunk=None):
    """submit's sibling for a fleet with a model per gait.  models: the bytes of every model, None where a block is none a
    gait may run with; model_of [B]: gait g runs with models[model_of[g]].  A gait whose model_of is outside the list or names
    a None is refused: it is not submitted.  start: B states' bytes; vel: [n_seg, B, 3].  The gaits are grouped by model and
    every group is queued in chunks of at most `chunk` gaits (default: about four chunks per MAX_WORKERS over the fleet)
    through `advance`."""
    vel = np.ascontiguousarray(vel, dtype=np.float64)
    model_of = np.asarray(model_of, dtype=np.int64)
    B = vel.shape[1]
    sz = layout["state_size"]
    assert model_of.shape == (B,) and len(start) == B * sz and outs in ("raw", "digest")
    usable = np.array([m is not None for m in models], dtype=bool)
    inside = (model_of >= 0) & (model_of < len(models))
    accepted = inside.copy()
    accepted[inside] = usable[model_of[inside]]
    if chunk is None:
        chunk = max(1, -(-int(accepted.sum()) // (4 * MAX_WORKERS)))
    assert chunk >= 1
    st = np.frombuffer(start, dtype=np.uint8).reshape(B, sz)
    asyncs, index = [], []
    for k in np.unique(model_of[accepted]):
        group = np.flatnonzero(accepted & (model_of == k))
        for lo in range(0, len(group), chunk):
            idx = group[lo:lo + chunk]
            args = (layout, bytes(models[k]), st[idx].tobytes(), np.ascontiguousarray(vel[:, idx]), int(redraw), int(n_ticks),
                    tuple(keep_ticks), outs, bool(nan_aware), len(index))
            asyncs.append(pool.apply_async(advance, args))
            index.append(idx)
    return MixedFleetJob(asyncs, index, accepted, bytes(start), sz, layout["out_size"], n_ticks, tuple(keep_ticks), outs)


# ---------------------------------------------------------------------------------------------------------- worker side
def worker_report():
    """Whether this process holds what a checker worker must never hold."""
    maps = open("/proc/self/maps").read()
    return {"pid": os.getpid(), "torch": "torch" in sys.modules,
            "libs": sorted({ln.split()[-1] for ln in maps.splitlines()
                            if "libamdhip64" in ln or "libwg_mpc" in ln})}


def advance(layout, model_bytes, start, vel, redraw, n_ticks, keep_ticks=(), outs="raw", nan_aware=False, g0=0):
    """Advance ng = vel.shape[1] gaits n_ticks ticks on the oracle, exactly as wgo_mpc_run does (references set on redraw
    ticks, the clock advanced by 1 / 19 / 20 control periods by repeated addition), with each tick through
    wgo_mpc_tick(model, state, &out, NULL).  Returns the final state bytes, the per-tick diag [n_ticks, ng, 6] int32
    (wg_tick_out_t's six int fields: the layout of the kernels' diag), the kept ticks' outs and worker_report()."""
    lib = C.CDLL(PTRIG_SO)
    lib.wgo_mpc_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.wgo_mpc_tick.restype = C.c_int
    sz, osz = layout["state_size"], layout["out_size"]
    ng = vel.shape[1]
    model = C.create_string_buffer(bytes(model_bytes), len(model_bytes))
    tctrl = float(np.frombuffer(model.raw, dtype=np.float64, count=1, offset=layout["tctrl_off"])[0])
    states = C.create_string_buffer(bytes(start) * (ng if len(start) == sz else 1), ng * sz)
    words = np.frombuffer(states, dtype=np.float64).reshape(ng, sz // 8)          # a view: writes go to the structs
    ck, vr = layout["clock_off"] // 8, layout["vref_off"] // 8
    out = C.create_string_buffer(osz)
    dview = np.frombuffer(out, dtype=np.int32, count=6, offset=layout["diag_off"])
    diag = np.empty((n_ticks, ng, 6), dtype=np.int32)
    kept = {t: (bytearray(ng * osz) if outs == "raw" else np.empty(ng, dtype=np.uint64)) for t in keep_ticks}
    base, mp_ = C.addressof(states), C.addressof(model)
    for tick in range(n_ticks):
        adv = 1 if tick == 0 else (19 if tick == 1 else 20)
        if tick % redraw == 0:
            words[:, vr:vr + 3] = vel[tick // redraw]
        keep = kept.get(tick)
        for g in range(ng):
            c = float(words[g, ck])
            for _ in range(adv):
                c += tctrl
            words[g, ck] = c
            C.memset(out, 0, osz)
            rc = lib.wgo_mpc_tick(mp_, base + g * sz, C.addressof(out), None)
            if rc != 0:
                raise RuntimeError("wgo_mpc_tick returned %d (gait %d, tick %d)" % (rc, g0 + g, tick))
            diag[tick, g] = dview
            if keep is not None:
                if outs == "raw":
                    keep[g * osz:(g + 1) * osz] = out.raw
                else:
                    keep[g] = digest(np.frombuffer(out.raw, dtype=np.uint64), nan_aware)
    return {"g0": g0, "ng": ng, "states": states.raw, "diag": diag,
            "outs": {t: (bytes(v) if outs == "raw" else v) for t, v in kept.items()}, "worker": worker_report()}


# ---------------------------------------------------------------------------------------------------------- comparison
def _u64(a):
    if isinstance(a, (bytes, bytearray, memoryview)):
        return np.frombuffer(a, dtype=np.uint64)
    return np.ascontiguousarray(a).view(np.uint64)


def is_nan_word(w):
    w = np.asarray(w, dtype=np.uint64)
    return ((w & _EXP) == _EXP) & ((w & _MANT) != 0)


def canonical(w):
    """NaN words replaced by one canonical NaN (sign and payload dropped); everything else, infs included, kept."""
    w = np.array(w, dtype=np.uint64, copy=True)
    w[is_nan_word(w)] = CANONICAL_NAN
    return w


def digest(words, nan_aware=False):
    """uint64 digest over the last axis: a wrapping sum of word x (odd weight).  An odd weight is invertible modulo 2^64,
    so a change of any single word always changes the digest."""
    w = np.asarray(words, dtype=np.uint64)
    if nan_aware:
        w = canonical(w)
    k = (np.arange(w.shape[-1], dtype=np.uint64) * np.uint64(2) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        return (w * k).sum(axis=-1, dtype=np.uint64)


def words_match(a, b, nan_aware=False):
    """Elementwise over uint64 words: equal, or (nan_aware) both NaN whatever their sign / payload."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    eq = a == b
    if nan_aware:
        eq |= is_nan_word(a) & is_nan_word(b)
    return eq


def word_names(struct_cls):
    """Name of every 8-byte word of a ctypes struct (two ints sharing a word: 'a|b')."""
    leaves = []

    def walk(cls, base, prefix):
        for f in cls._fields_:
            name, typ = f[0], f[1]
            off = base + getattr(cls, name).offset
            _leaf(typ, off, prefix + name)

    def _leaf(typ, off, name):
        if hasattr(typ, "_fields_"):
            walk(typ, off, name + ".")
        elif hasattr(typ, "_length_"):
            el = typ._type_
            for i in range(typ._length_):
                _leaf(el, off + i * C.sizeof(el), "%s[%d]" % (name, i))
        else:
            leaves.append((off, name))
    walk(struct_cls, 0, "")
    names = [[] for _ in range(C.sizeof(struct_cls) // 8)]
    for off, name in leaves:
        names[off // 8].append(name)
    return ["|".join(n) if n else "<padding>" for n in names]


def record_mismatches(cpu, gpu, rec_size, nan_aware=False, names=None):
    """[(record index, first differing word's name or index, cpu word, gpu word)] for every differing record of two
    arrays of rec_size-byte structs."""
    a, b = _u64(cpu), _u64(gpu)
    assert a.size == b.size and (a.size * 8) % rec_size == 0, (a.size, b.size, rec_size)
    a, b = a.reshape(-1, rec_size // 8), b.reshape(-1, rec_size // 8)
    ok = words_match(a, b, nan_aware)
    bad = []
    for r in np.flatnonzero(~ok.all(axis=1)):
        w = int(np.argmin(ok[r]))
        bad.append((int(r), names[w] if names else w, "0x%016x" % int(a[r, w]), "0x%016x" % int(b[r, w])))
    return bad


def assert_records_equal(cpu, gpu, rec_size, what, nan_aware=False, names=None, first=0, shown=8):
    """Raise naming the first differing records (gait = first + record index) and their first differing field."""
    bad = record_mismatches(cpu, gpu, rec_size, nan_aware, names)
    if bad:
        raise AssertionError("%s: %d of %d gaits differ from the oracle; first: %s" % (
            what, len(bad), _u64(cpu).size * 8 // rec_size,
            "; ".join("gait %d field %s (oracle %s, GPU %s)" % (first + r, f, x, y) for r, f, x, y in bad[:shown])))


DIAG_FIELDS = ("ifail", "n_iter", "nact", "n", "m", "nb_prw_steps")


def assert_diag_equal(cpu, gpu, what, first_tick=0, first_gait=0, shown=8):
    """Per-tick diag [T, B, 6] int32, exact: raise naming the first differing gaits with their first differing tick/field."""
    cpu, gpu = np.asarray(cpu), np.asarray(gpu)
    assert cpu.shape == gpu.shape, (what, cpu.shape, gpu.shape)
    ne = cpu != gpu
    if ne.any():
        gaits = np.flatnonzero(ne.any(axis=(0, 2)))
        msg = []
        for g in gaits[:shown]:
            t, f = np.argwhere(ne[:, g, :])[0]
            msg.append("gait %d tick %d %s (oracle %d, GPU %d)" % (first_gait + g, first_tick + t, DIAG_FIELDS[f],
                                                                   cpu[t, g, f], gpu[t, g, f]))
        raise AssertionError("%s: %d of %d gaits differ from the oracle; first: %s" % (what, len(gaits), cpu.shape[1],
                                                                                       "; ".join(msg)))


def nan_gaits(states, state_size):
    """Number of gaits with a NaN word in their state."""
    w = _u64(states).reshape(-1, state_size // 8)
    return int(is_nan_word(w).any(axis=1).sum())
