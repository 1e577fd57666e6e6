"""ctypes binding of include/wg_mpc.h (no compute here)."""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WG_LIB_PATH", os.path.join(_HERE, "lib", "libwg_mpc.so"))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "wg_mpc.h")     # the one statement of every signature

SAMPLES = 20   # WG_SAMPLES_PER_TICK


class FootSample(C.Structure):          # wg_foot_sample_t
    _fields_ = [(k, C.c_double) for k in
                ("x", "y", "z", "theta", "omega", "omega2", "dx", "dy", "dz", "dtheta", "domega", "domega2",
                 "ddx", "ddy", "ddz", "ddtheta", "ddomega", "ddomega2")]


class Model(C.Structure):               # wg_model_t
    _fields_ = [("N", C.c_int), ("flags", C.c_int)] + [(k, C.c_double) for k in
                ("T", "Tctrl", "com_height_qp", "alpha", "beta", "gamma", "sole_w", "sole_h", "margin_x", "margin_y",
                 "ds_feet_distance", "hip_l_lo", "hip_l_hi", "hip_r_lo", "hip_r_hi", "hip_vmax", "hip_amax",
                 "feet_cross_max", "step_period", "ds_period", "dsss_period", "t_single", "t_double", "step_height",
                 "feet_distance")]


class GaitState(C.Structure):           # wg_gait_state_t
    _fields_ = [("clock", C.c_double), ("upper_time_limit", C.c_double), ("time_to_stop", C.c_double),
                ("tick_count", C.c_int), ("running", C.c_int), ("ending_phase", C.c_int), ("online", C.c_int),
                ("vref", C.c_double * 3),
                ("com_x", C.c_double * 3), ("com_y", C.c_double * 3), ("com_z", C.c_double),
                ("phase", C.c_int), ("foot", C.c_int), ("nb_steps_left", C.c_int), ("step_number", C.c_int),
                ("state_changed", C.c_int), ("pad0_", C.c_int),
                ("time_limit", C.c_double), ("start_time", C.c_double), ("sup_x", C.c_double), ("sup_y", C.c_double),
                ("sup_yaw", C.c_double),
                ("in_translation", C.c_int), ("in_rotation", C.c_int), ("nb_steps_after_rotation", C.c_int),
                ("rot_support_foot", C.c_int), ("post_rotation_phase", C.c_int), ("nb_steps_ssds", C.c_int),
                ("trunk_yaw", C.c_double * 3), ("trunkT_yaw", C.c_double * 3),
                ("lf", FootSample * 3), ("rf", FootSample * 3),
                ("front_com_x", C.c_double * 3), ("front_com_y", C.c_double * 3),
                ("poly_z", C.c_double * 5)]


class TickOut(C.Structure):             # wg_tick_out_t
    _fields_ = [("jerk_x", C.c_double), ("jerk_y", C.c_double),
                ("ifail", C.c_int), ("n_iter", C.c_int), ("nact", C.c_int), ("n", C.c_int), ("m", C.c_int),
                ("nb_prw_steps", C.c_int),
                ("com_x", (C.c_double * 3) * SAMPLES), ("com_y", (C.c_double * 3) * SAMPLES),
                ("com_yaw", (C.c_double * 2) * SAMPLES),
                ("zmp_x", C.c_double * SAMPLES), ("zmp_y", C.c_double * SAMPLES),
                ("lf", FootSample * SAMPLES), ("rf", FootSample * SAMPLES),
                ("lf_back", FootSample), ("rf_back", FootSample),
                ("pad_", C.c_double * 15)]          # sizeof == 7808 = 61 x 128 B (ABI 5)


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


class WgError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong}
_RETURNS = dict(_SCALARS, **{"void": None, "const char *": C.c_char_p})


def header_signatures(text):
    """{name: (restype, argtypes)} of a header's text: every prototype `RET wg_name(PARAMS);`, and NAME_ctx -- NAME's own
    signature behind the context pointer -- for every entry X(ret, NAME, (params), (args)) of its list of context forms.  A
    pointer or array parameter is a c_void_p; a type that is not one of the ABI's is an error, never a default."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S).replace("\\\n", " ")
    listed = re.findall(r"\bX\(\s*[\w ]+?,\s*(wg_\w+)\s*,", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)                      # preprocessor lines, the list among them
    text = re.sub(r"\bstruct\s+\w*\s*\{[^{}]*\}", "struct", text)         # struct bodies
    sigs = {}
    for ret, name, params in re.findall(r"([\w\s*]+?)\b(wg_\w+)\s*\(([^()]*)\)\s*;", text):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            raise WgError(f"{name}: return type '{ret}' is not one the binding knows")
        args = []
        for p in [] if params.strip() == "void" else params.split(","):
            ctype = " ".join(p.split()[:-1])
            if "*" not in p and "[" not in p and ctype not in _SCALARS:
                raise WgError(f"{name}: parameter '{p.strip()}' has a type the binding does not know")
            args.append(C.c_void_p if "*" in p or "[" in p else _SCALARS[ctype])
        sigs[name] = (_RETURNS[ret], args)
    for name in listed:
        if name not in sigs:
            raise WgError(f"{name} is in the list of context forms but has no prototype")
        sigs[name + "_ctx"] = (sigs[name][0], [C.c_void_p] + sigs[name][1])
    return sigs


def bind(cdll):
    """argtypes and restype, as include/wg_mpc.h states them, of every entry point that `cdll` exports; one it does not export
    (an older build under WG_LIB_PATH, A/B runs) is skipped"""
    if not os.path.exists(HEADER_PATH):
        raise WgError(f"{HEADER_PATH} missing: the binding takes every signature from it")
    with open(HEADER_PATH) as f:
        sigs = header_signatures(f.read())
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return cdll


def lib():
    """Load libwg_mpc.so (fails loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WgError(f"{LIB_PATH} missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  If the
        # product library were loaded first and torch later, two runtimes would coexist and the second one finds no GPU;
        # with torch first the loader binds libwg_mpc.so to the runtime already in the process, and torch tensors'
        # device pointers / streams can be handed to the _dev entry points.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def _check(rc):
    if rc != 0:
        raise WgError(f"wg error {rc}: {lib().wg_last_error().decode()}")


def _raw(name, ctx, *args):
    """NAME(*args), or NAME_ctx(ctx, *args) for a Context or a raw wg_ctx_t handle: the way every wrapper reaches the library"""
    if ctx is None:
        return getattr(lib(), name)(*args)
    return getattr(lib(), name + "_ctx")(ctx.handle if isinstance(ctx, Context) else ctx, *args)


def _call(name, ctx, *args):
    _check(_raw(name, ctx, *args))


class Context:
    """wg_ctx_t: one configured model with its device tables and workspaces (include/wg_mpc.h, "Contexts").  Two contexts
    may hold different models and run overlapping launches on different streams.  Every wrapper of an entry point with a
    context form takes ctx=; the methods here are the Herdt-tick family by its old names, `call` the raw NAME_ctx."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().wg_ctx_create(int(device), C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            lib().wg_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:            # noqa: BLE001 -- interpreter shutdown
            pass

    def call(self, name, *args):
        """NAME_ctx(ctx, *args), raw"""
        return getattr(lib(), name + "_ctx")(self.handle, *args)

    def device(self):
        return int(lib().wg_ctx_device(self.handle))

    def mpc_configure(self, model):
        mpc_configure(model, ctx=self)

    def mpc_tick_lds_bytes(self):
        return mpc_tick_lds_bytes(ctx=self)

    def mpc_tick_batch(self, states, want_out=True, advance_calls=0, hist_cap=0):
        return mpc_tick_batch(states, want_out, advance_calls, hist_cap, ctx=self)

    def mpc_tick_batch_dev(self, B, states_ptr, outs_ptr=None, diag_ptr=None, advance_calls=0, hist_ptr=None, hist_cap=0,
                           hist_len_ptr=None, stream=None):
        mpc_tick_batch_dev(B, states_ptr, outs_ptr, diag_ptr, advance_calls, hist_ptr, hist_cap, hist_len_ptr, stream, ctx=self)

    def mpc_run_batch_dev(self, B, states_ptr, n_ticks, advance_calls=20, outs_ptr=None, diag_ptr=None, stream=None):
        mpc_run_batch_dev(B, states_ptr, n_ticks, advance_calls, outs_ptr, diag_ptr, stream, ctx=self)

    def mpc_run_sched_dev(self, B, states_ptr, n_ticks, vref_sched_ptr, period, advance_calls=20, outs_ptr=None, diag_ptr=None,
                          stream=None):
        mpc_run_sched_dev(B, states_ptr, n_ticks, vref_sched_ptr, period, advance_calls, outs_ptr, diag_ptr, stream, ctx=self)

    def mpc_set_velref_dev(self, B, states_ptr, vref_ptr, stream=None):
        mpc_set_velref_dev(B, states_ptr, vref_ptr, stream, ctx=self)


def init(device=0):
    _check(lib().wg_init(int(device)))


def shutdown():
    lib().wg_shutdown()


def qp_lds_bytes(n, m):
    return int(lib().wg_qp_lds_bytes(int(n), int(m)))


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_qps(qps):
    """Pad a list of qpgen-style dicts into the strided batch layout of wg_qp_solve_batch."""
    B = len(qps)
    nmax = max(q["n"] for q in qps)
    mmax = max(q["mmax"] for q in qps)
    Cb = np.zeros((B, nmax * nmax))
    Ab = np.zeros((B, mmax * nmax))
    d = np.zeros((B, nmax)); xl = np.zeros((B, nmax)); xu = np.zeros((B, nmax))
    b = np.zeros((B, mmax))
    n = np.zeros(B, dtype=np.int32); m = np.zeros(B, dtype=np.int32); me = np.zeros(B, dtype=np.int32)
    for k, q in enumerate(qps):
        nn, mm = q["n"], q["m"]
        Cf = np.zeros((nmax, nmax), order="F"); Cf[:nn, :nn] = q["C"][:nn, :nn]
        Af = np.zeros((mmax, nmax), order="F"); Af[:mm, :nn] = q["A"][:mm, :nn]
        Cb[k] = Cf.ravel(order="F"); Ab[k] = Af.ravel(order="F")
        d[k, :nn] = q["d"]; xl[k, :nn] = q["xl"]; xu[k, :nn] = q["xu"]; b[k, :mm] = q["b"][:mm]
        n[k], m[k], me[k] = nn, mm, q["me"]
    return dict(B=B, nmax=nmax, mmax=mmax, n=n, m=m, me=me, C=Cb, d=d, A=Ab, b=b, xl=xl, xu=xu)


def qp_solve_batch(pk, eps=1e-8, hist_cap=256, ctx=None):
    """Host-pointer entry point (wg_qp_solve_batch): numpy in, numpy out."""
    B, nmax, mmax = pk["B"], pk["nmax"], pk["mmax"]
    x = np.zeros((B, nmax)); u = np.zeros((B, mmax + 2 * nmax))
    ifail = np.full(B, -99, dtype=np.int32); n_iter = np.zeros(B, dtype=np.int32)
    iact = np.zeros((B, nmax), dtype=np.int32); nact = np.zeros(B, dtype=np.int32)
    hist = np.zeros((B, hist_cap), dtype=np.int32); hist_len = np.zeros(B, dtype=np.int32)
    _call("wg_qp_solve_batch", ctx, B, nmax, mmax, _hp(pk["n"]), _hp(pk["m"]), _hp(pk["me"]), _hp(pk["C"]), _hp(pk["d"]),
          _hp(pk["A"]), _hp(pk["b"]), _hp(pk["xl"]), _hp(pk["xu"]), eps, _hp(x), _hp(u), _hp(ifail), _hp(n_iter), _hp(iact),
          _hp(nact), _hp(hist), hist_cap, _hp(hist_len))
    return dict(x=x, u=u, ifail=ifail, n_iter=n_iter, iact=iact, nact=nact, hist=hist, hist_len=hist_len)


def qp_solve_batch_dev(B, nmax, mmax, n, m, me, Cd, d, A, b, xl, xu, eps, x, u, ifail, n_iter=None, iact=None, nact=None,
                       hist=None, hist_cap=0, hist_len=None, stream=None, ctx=None):
    """Device-pointer entry point (wg_qp_solve_batch_dev).  Arguments are torch CUDA tensors or None."""
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _call("wg_qp_solve_batch_dev", ctx, B, nmax, mmax, p(n), p(m), p(me), p(Cd), p(d), p(A), p(b), p(xl), p(xu), eps, p(x),
          p(u), p(ifail), p(n_iter), p(iact), p(nact), p(hist), hist_cap, p(hist_len), C.c_void_p(stream) if stream else None)


# ---------------------------------------------------------------------------
# Herdt-2010 tick
# ---------------------------------------------------------------------------
def model_defaults():
    m = Model()
    lib().wg_model_defaults(C.byref(m))
    return m


def gait_init(model, com0, left_xyt, right_xyt):
    s = GaitState()
    a3 = lambda v: (C.c_double * 3)(*v)
    lib().wg_gait_init(C.byref(model), C.byref(s), a3(com0), a3(left_xyt), a3(right_xyt))
    return s


def mpc_configure(model, ctx=None):
    _call("wg_mpc_configure", ctx, C.byref(model))


def mpc_tick_lds_bytes_for(model):
    """LDS bytes per gait the tick kernel would use for `model` (host arithmetic, no GPU needed)."""
    return int(lib().wg_mpc_tick_lds_bytes_for(C.byref(model)))


def mpc_tick_lds_bytes(ctx=None):
    return int(_raw("wg_mpc_tick_lds_bytes", ctx))


def mpc_tick_batch(states, want_out=True, advance_calls=0, hist_cap=0, ctx=None):
    """Host-pointer entry point.  `states` is a ctypes array (GaitState * B), updated in place."""
    B = len(states)
    outs = (TickOut * B)() if want_out else None
    diag = np.zeros((B, 6), dtype=np.int32)
    hist = np.zeros((B, hist_cap), dtype=np.int32) if hist_cap else None
    hlen = np.zeros(B, dtype=np.int32) if hist_cap else None
    _call("wg_mpc_tick_batch", ctx, B, C.addressof(states), C.addressof(outs) if outs is not None else None, _hp(diag),
          advance_calls, _hp(hist), hist_cap, _hp(hlen))
    return outs, diag, hist, hlen


def mpc_assemble_batch(states, advance_calls=0, nmax=None, mmax=None, model=None, ctx=None):
    """The QP of every gait's next tick as QPProblem::solve hands it to ql0001_ (wg_mpc_assemble_batch): a pack_qps-style
    dict (C, d, A, b, xl, xu column-major with strides nmax / mmax, n, m, me) ready for qp_solve_batch.  `states` is a ctypes
    array (GaitState * B), not modified."""
    B = len(states)
    N = model.N if model is not None else 16
    nmax = nmax or 2 * N + 8
    mmax = mmax or 1 + 4 * N + 20 + 1
    Cb = np.zeros((B, nmax * nmax)); Ab = np.zeros((B, mmax * nmax)); d = np.zeros((B, nmax)); b = np.zeros((B, mmax))
    xl = np.zeros((B, nmax)); xu = np.zeros((B, nmax)); n = np.zeros(B, dtype=np.int32); m = np.zeros(B, dtype=np.int32)
    _call("wg_mpc_assemble_batch", ctx, B, C.addressof(states), int(advance_calls), nmax, mmax, _hp(Cb), _hp(d), _hp(Ab),
          _hp(b), _hp(xl), _hp(xu), _hp(n), _hp(m))
    return dict(B=B, nmax=nmax, mmax=mmax, n=n, m=m, me=np.zeros(B, dtype=np.int32), C=Cb, d=d, A=Ab, b=b, xl=xl, xu=xu)


class HostMapped:
    """A block of host-mapped memory from wg_host_alloc holding one GaitState, one TickOut and the 6 diagnostic ints: what
    wg_mpc_tick_pinned works on (the one-robot path: no staging copies, no device synchronisation)."""

    def __init__(self):
        p = C.c_void_p()
        size = C.sizeof(GaitState) + C.sizeof(TickOut) + 64
        _check(lib().wg_host_alloc(C.byref(p), size))
        self.ptr = p
        self.state = GaitState.from_address(p.value)
        self.out = TickOut.from_address(p.value + C.sizeof(GaitState))
        self.diag = (C.c_int * 6).from_address(p.value + C.sizeof(GaitState) + C.sizeof(TickOut))

    def tick(self, advance_calls=0, ctx=None):
        _call("wg_mpc_tick_pinned", ctx, C.addressof(self.state), C.addressof(self.out), C.addressof(self.diag), int(advance_calls))

    def close(self):
        if self.ptr:
            lib().wg_host_free(self.ptr)
            self.ptr = None


def mpc_tick_batch_dev(B, states_ptr, outs_ptr=None, diag_ptr=None, advance_calls=0, hist_ptr=None, hist_cap=0,
                       hist_len_ptr=None, stream=None, ctx=None):
    """Device-pointer entry point; pointers are plain ints (e.g. torch tensor.data_ptr())."""
    v = lambda p: C.c_void_p(p) if p else None
    _call("wg_mpc_tick_batch_dev", ctx, B, v(states_ptr), v(outs_ptr), v(diag_ptr), advance_calls, v(hist_ptr), hist_cap,
          v(hist_len_ptr), v(stream))


def mpc_run_batch_dev(B, states_ptr, n_ticks, advance_calls=20, outs_ptr=None, diag_ptr=None, stream=None, ctx=None):
    """n_ticks ticks of every gait in one launch (device-side work queue); device pointers as integers."""
    _call("wg_mpc_run_batch_dev", ctx, B, states_ptr, int(n_ticks), int(advance_calls), outs_ptr, diag_ptr, stream)


def mpc_run_sched_dev(B, states_ptr, n_ticks, vref_sched_ptr, period, advance_calls=20, outs_ptr=None, diag_ptr=None,
                      stream=None, ctx=None):
    """mpc_run_batch_dev with the velocity references staged ahead: block t // period of vref_sched (ceil(n_ticks / period)
    x B x 3 doubles on the device) takes effect before tick t = 0, period, 2 period, ... of the launch."""
    _call("wg_mpc_run_sched_dev", ctx, B, states_ptr, int(n_ticks), int(advance_calls), vref_sched_ptr, int(period), outs_ptr,
          diag_ptr, stream)


def mpc_set_velref_dev(B, states_ptr, vref_ptr, stream=None, ctx=None):
    v = lambda p: C.c_void_p(p) if p else None
    _call("wg_mpc_set_velref_dev", ctx, B, v(states_ptr), v(vref_ptr), v(stream))


RICCATI_WITH_INITIALPOS = 0
RICCATI_WITHOUT_INITIALPOS = 1


def riccati_solve(A, b, c, Q, R, Nl, mode):
    """OptimalControllerSolver(A,b,c,Q,R,Nl).ComputeWeights(mode) -> (K[n], F[Nl]); host-side entry point."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    n = A.shape[0]
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(n)
    c = np.ascontiguousarray(c, dtype=np.float64).reshape(n)
    K = np.zeros(n)
    F = np.zeros(max(int(Nl), 1))
    rc = lib().wg_riccati_solve(n, _hp(A), _hp(b), _hp(c), float(Q), float(R), int(Nl), int(mode), _hp(K), _hp(F))
    if rc != 0:
        raise WgError(f"wg_riccati_solve failed ({rc})")
    return K, F[:int(Nl)]


def riccati_gains(T, zc, Q, R, Nl, mode):
    """PreviewControl::ComputeOptimalWeights -> (K[4], F[Nl]); see include/wg_mpc.h for the layout of K."""
    K = np.zeros(4)
    F = np.zeros(max(int(Nl), 1))
    rc = lib().wg_riccati_gains(float(T), float(zc), float(Q), float(R), int(Nl), int(mode), _hp(K), _hp(F))
    if rc != 0:
        raise WgError(f"wg_riccati_gains failed ({rc})")
    return K, F[:int(Nl)]


PLDP_N = 16
PLDP_MMAX = 8 * PLDP_N


class PldpState(C.Structure):           # wg_pldp_state_t
    _fields_ = [("n_prev", C.c_int), ("prev_active", C.c_int * PLDP_MMAX), ("pad_", C.c_int),
                ("prev_zmp", C.c_double * (2 * PLDP_N)), ("internal_time", C.c_double)]


def pldp_configure(N, iPu, Px, Pu, ctx=None):
    iPu = np.ascontiguousarray(iPu, dtype=np.float64); Px = np.ascontiguousarray(Px, dtype=np.float64)
    Pu = np.ascontiguousarray(Pu, dtype=np.float64)
    _call("wg_pldp_configure", ctx, int(N), _hp(iPu), _hp(Px), _hp(Pu))


def pldp_lds_bytes():
    return int(lib().wg_pldp_lds_bytes())


def pldp_solve_batch(N, mcap, m, D, A, b, zmpref, xkyk, similar, n_removed, starting, states, max_iter=0, ctx=None):
    """Host-pointer batch solve.  Arrays follow include/wg_mpc.h (A: B x (mcap+1)*2N flat slots, leading dimension
    m[b]+1 inside a slot); `states` is a ctypes array of PldpState, updated in place."""
    B = len(m)
    n = 2 * N
    m = np.ascontiguousarray(m, dtype=np.int32); D = np.ascontiguousarray(D, dtype=np.float64)
    A = np.ascontiguousarray(A, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    zmpref = np.ascontiguousarray(zmpref, dtype=np.float64); xkyk = np.ascontiguousarray(xkyk, dtype=np.float64)
    similar = np.ascontiguousarray(similar, dtype=np.int32)
    n_removed = np.ascontiguousarray(n_removed, dtype=np.int32); starting = np.ascontiguousarray(starting, dtype=np.int32)
    assert A.size == B * (mcap + 1) * n and b.size == B * mcap and similar.size == B * mcap
    X = np.zeros((B, n)); ret = np.zeros(B, dtype=np.int32); nit = np.zeros(B, dtype=np.int32)
    act = np.zeros((B, mcap), dtype=np.int32); nact = np.zeros(B, dtype=np.int32)
    _call("wg_pldp_solve_batch", ctx, B, int(mcap), _hp(m), _hp(D), _hp(A), _hp(b), _hp(zmpref), _hp(xkyk), _hp(similar),
          _hp(n_removed), _hp(starting), int(max_iter), C.addressof(states), _hp(X), _hp(ret), _hp(nit), _hp(act), _hp(nact))
    return dict(X=X, ret=ret, n_iter=nit, active=[act[i, :nact[i]].copy() for i in range(B)])


POLY_MAX_ROWS = 8


class DimitrovModel(C.Structure):       # wg_dimitrov_model_t
    _fields_ = [("N", C.c_int), ("solver", C.c_int), ("T", C.c_double), ("Tctrl", C.c_double), ("com_height", C.c_double),
                ("alpha", C.c_double), ("beta", C.c_double)]       # solver: 0 = PLDP (the reference's default), 1 = QLD


class ZmpPolytope(C.Structure):         # wg_zmp_polytope_t
    _fields_ = [("nrows", C.c_int), ("pad_", C.c_int), ("similar", C.c_int * POLY_MAX_ROWS),
                ("A", (C.c_double * 2) * POLY_MAX_ROWS), ("B", C.c_double * POLY_MAX_ROWS), ("centre", C.c_double * 2)]


class DimitrovState(C.Structure):       # wg_dimitrov_state_t
    _fields_ = [("xk", C.c_double * 6), ("pldp", PldpState), ("n_removed", C.c_int), ("starting", C.c_int)]


class DimitrovOut(C.Structure):         # wg_dimitrov_out_t
    _fields_ = [("jerk_x", C.c_double), ("jerk_y", C.c_double), ("ret", C.c_int), ("n_iter", C.c_int),
                ("n_active", C.c_int), ("m", C.c_int),
                ("com_x", (C.c_double * 3) * 21), ("com_y", (C.c_double * 3) * 21),
                ("zmp_x", C.c_double * 21), ("zmp_y", C.c_double * 21), ("X", C.c_double * 32)]


def dimitrov_defaults():
    m = DimitrovModel()
    lib().wg_dimitrov_defaults(C.byref(m))
    return m


def dimitrov_configure(model, ctx=None):
    _call("wg_dimitrov_configure", ctx, C.byref(model))


def dimitrov_constants(N, ctx=None):
    n = 2 * N
    iLQ = np.zeros((n, n)); OptB = np.zeros((n, 6)); OptC = np.zeros((n, n))
    Pu = np.zeros((N, N)); iPu = np.zeros((N, N)); Px = np.zeros((N, 3))
    _call("wg_dimitrov_get_constants", ctx, _hp(iLQ), _hp(OptB), _hp(OptC), _hp(Pu), _hp(iPu), _hp(Px))
    return dict(iLQ=iLQ, OptB=OptB, OptC=OptC, Pu=Pu, iPu=iPu, Px=Px)


def dimitrov_qld_constants(N, ctx=None):
    """what mode QLD hands to ql0001_ and builds its cost vector from: Q (column-major 2N x 2N), OptB / OptC as built, Pu'"""
    n = 2 * N
    Q = np.zeros((n, n)); OptB = np.zeros((n, 6)); OptC = np.zeros((n, n)); PuT = np.zeros((N, N))
    _call("wg_dimitrov_get_qld_constants", ctx, _hp(Q), _hp(OptB), _hp(OptC), _hp(PuT))
    return dict(Q=Q, OptB=OptB, OptC=OptC, PuT=PuT)


def dimitrov_tick_batch(polys, states, want_out=True, max_iter=0, ctx=None):
    """polys: ctypes array (ZmpPolytope * (B*N)), states: (DimitrovState * B), updated in place."""
    B = len(states)
    outs = (DimitrovOut * B)() if want_out else None
    _call("wg_dimitrov_tick_batch", ctx, B, C.addressof(polys), C.addressof(states),
          C.addressof(outs) if outs is not None else None, int(max_iter))
    return outs


# ---- Kajita stage-1 preview control (PreviewControl::OneIterationOfPreview, batched) ----
class PreviewGains(C.Structure):        # wg_preview_gains_t
    _fields_ = [("T", C.c_double), ("zc", C.c_double), ("Ks", C.c_double), ("Kx", C.c_double * 3), ("nl", C.c_int),
                ("pad_", C.c_int)]


def preview_gains(T, zc, preview_time, mode=RICCATI_WITHOUT_INITIALPOS):
    """PreviewControl::ComputeOptimalWeights (PreviewControl.cpp:198-322): (PreviewGains, F[nl])."""
    nl = int(preview_time / T)
    R = 1e-6 if mode == RICCATI_WITHOUT_INITIALPOS else 1e-5
    K, F = riccati_gains(T, zc, 1.0, R, nl, mode)
    g = PreviewGains()
    g.T, g.zc, g.nl = T, zc, nl
    if mode == RICCATI_WITHOUT_INITIALPOS:
        g.Ks = K[0]; g.Kx[0], g.Kx[1], g.Kx[2] = K[1], K[2], K[3]
    else:
        g.Ks = K[0]; g.Kx[0], g.Kx[1], g.Kx[2] = K[0], K[1], K[2]
    return g, np.ascontiguousarray(F)


def preview_configure(gains, F, ctx=None):
    F = np.ascontiguousarray(F, dtype=np.float64)
    assert F.shape == (gains.nl,)
    _call("wg_preview_configure", ctx, C.byref(gains), _hp(F))


def preview_run_batch(zmp_x, zmp_y, state, L, simulation=True, want_com=True, want_zmp=True, ctx=None):
    """Host-pointer entry point: zmp_x/zmp_y [B, L+nl-1], state [B, 8] (advanced in place).  Returns (com, zmp2)."""
    zmp_x = np.ascontiguousarray(zmp_x, dtype=np.float64); zmp_y = np.ascontiguousarray(zmp_y, dtype=np.float64)
    B = zmp_x.shape[0]
    nl = int(_raw("wg_preview_window", ctx))
    assert zmp_x.shape == zmp_y.shape == (B, L + nl - 1) and state.shape == (B, 8) and state.flags.c_contiguous
    com = np.zeros((B, L, 6)) if want_com else None
    z2 = np.zeros((B, L, 2)) if want_zmp else None
    _call("wg_preview_run_batch", ctx, B, L, _hp(zmp_x), _hp(zmp_y), _hp(state), _hp(com), _hp(z2), int(bool(simulation)))
    return com, z2


def preview_run_batch_dev(B, L, zx_tm_ptr, zy_tm_ptr, state_ptr, com_tm_ptr=None, zmp2_tm_ptr=None, simulation=True,
                          stream=None, ctx=None):
    _call("wg_preview_run_batch_dev", ctx, B, L, zx_tm_ptr, zy_tm_ptr, state_ptr, com_tm_ptr, zmp2_tm_ptr,
          int(bool(simulation)), stream)


def preview_follow_dev(B, lcap, length_ptr, done_ptr, zx_tm_ptr, zy_tm_ptr, state_ptr, com_tm_ptr=None, zmp2_tm_ptr=None,
                       simulation=True, stream=None, ctx=None):
    """every gait over the rows its own queue has made safe: steps [done[b], length[b] - nl + 1), absolute rows (wg_mpc.h)"""
    _call("wg_preview_follow_dev", ctx, B, lcap, length_ptr, done_ptr, zx_tm_ptr, zy_tm_ptr, state_ptr, com_tm_ptr, zmp2_tm_ptr,
          int(bool(simulation)), stream)


# ---- Kajita fleets with a CoM height per gait: gains made on the device, preview with gains per gait ----
class PreviewFleet(C.Structure):        # wg_preview_fleet_t
    _fields_ = [("T", C.c_double), ("nl", C.c_int), ("pad_", C.c_int), ("zc", C.c_void_p), ("K_tm", C.c_void_p),
                ("F_tm", C.c_void_p)]


def preview_fleet(T, nl, zc_ptr, K_tm_ptr, F_tm_ptr):
    """wg_preview_fleet_t over device arrays zc [B], K_tm [4][B] (Ks, Kx0..2), F_tm [nl][B]"""
    f = PreviewFleet()
    f.T, f.nl, f.pad_, f.zc, f.K_tm, f.F_tm = float(T), int(nl), 0, zc_ptr, K_tm_ptr, F_tm_ptr
    return f


def riccati_gains_batch(T, zc, Q, R, Nl, mode, ctx=None):
    """wg_riccati_gains for every height of zc [B], on the device -> (K [B, 4], F [B, Nl], status [B]); host-pointer entry point."""
    zc = np.ascontiguousarray(zc, dtype=np.float64)
    B = zc.shape[0]
    K = np.zeros((B, 4))
    F = np.zeros((B, int(Nl)))
    status = np.zeros(B, dtype=np.int32)
    _call("wg_riccati_gains_batch", ctx, B, float(T), _hp(zc), float(Q), float(R), int(Nl), int(mode), _hp(K),
          _hp(F) if Nl > 0 else None, _hp(status))
    return K, F, status


def riccati_gains_batch_dev(B, T, zc_ptr, Q, R, Nl, mode, K_tm_ptr, F_tm_ptr, status_ptr, stream=None, ctx=None):
    """one lane per gait: K_tm [4][B], F_tm [Nl][B] time-major, status [B] (all device pointers)"""
    _call("wg_riccati_gains_batch_dev", ctx, B, float(T), zc_ptr, float(Q), float(R), int(Nl), int(mode), K_tm_ptr, F_tm_ptr,
          status_ptr, stream)


def preview_run_fleet_dev(B, L, fleet, zx_tm_ptr, zy_tm_ptr, state_ptr, com_tm_ptr=None, zmp2_tm_ptr=None, simulation=True,
                          stream=None, ctx=None):
    """wg_preview_run_batch_dev with the gains of `fleet` (a PreviewFleet) per gait instead of the context's"""
    _call("wg_preview_run_fleet_dev", ctx, B, L, C.addressof(fleet), zx_tm_ptr, zy_tm_ptr, state_ptr, com_tm_ptr, zmp2_tm_ptr,
          int(bool(simulation)), stream)


def preview_follow_fleet_dev(B, lcap, length_ptr, done_ptr, fleet, zx_tm_ptr, zy_tm_ptr, state_ptr, com_tm_ptr=None,
                             zmp2_tm_ptr=None, simulation=True, stream=None, ctx=None):
    """wg_preview_follow_dev with the gains of `fleet` (a PreviewFleet) per gait instead of the context's"""
    _call("wg_preview_follow_fleet_dev", ctx, B, lcap, length_ptr, done_ptr, C.addressof(fleet), zx_tm_ptr, zy_tm_ptr,
          state_ptr, com_tm_ptr, zmp2_tm_ptr, int(bool(simulation)), stream)


# ---- Kajita stage-1 inputs: ZMPDiscretization, batched; FootConstraintsAsLinearSystem (host) ----
ZMPDISC_MAX_STEPS = 64


class ZmpDiscModel(C.Structure):        # wg_zmpdisc_model_t
    _fields_ = [(k, C.c_double) for k in ("T", "preview_time", "t_single", "t_double", "step_height", "omega",
                                          "modulation")] + \
               [("zmp_neutral", C.c_double * 2), ("zmp_shift", C.c_double * 4)] + \
               [(k, C.c_double) for k in ("foot_b", "foot_h", "foot_f")]


class RelStep(C.Structure):             # wg_rel_step_t
    _fields_ = [(k, C.c_double) for k in ("sx", "sy", "theta", "ss_time", "ds_time")] + \
               [("step_type", C.c_int), ("pad_", C.c_int)]


def zmpdisc_defaults():
    m = ZmpDiscModel()
    lib().wg_zmpdisc_defaults(C.byref(m))
    return m


def rel_steps(triples, ss_time, ds_time, step_type=1):
    """(RelStep * S) from [S, 3] (sx, sy, theta in degrees), as StepStackHandler leaves a ":stepseq" (walk mode 0)."""
    t = np.asarray(triples, dtype=np.float64).reshape(-1, 3)
    steps = (RelStep * len(t))()
    for i, (sx, sy, th) in enumerate(t):
        steps[i] = RelStep(sx, sy, th, ss_time, ds_time, step_type, 0)
    return steps


def zmpdisc_length(model, steps, n_steps=None):
    return int(lib().wg_zmpdisc_length(C.byref(model), C.addressof(steps), len(steps) if n_steps is None else int(n_steps)))


def zmpdisc_batch(model, steps, n_steps, init_feet, smax, lcap, want_feet=True, ctx=None):
    """steps: (RelStep * (B*smax)); n_steps [B]; init_feet [B, 6].  Returns a dict of arrays and `length` [B]."""
    n_steps = np.ascontiguousarray(n_steps, dtype=np.int32); B = n_steps.shape[0]
    init_feet = np.ascontiguousarray(init_feet, dtype=np.float64)
    assert init_feet.shape == (B, 6) and len(steps) == B * smax
    r = dict(zmp=np.zeros((B, lcap, 2)), zmp_theta=np.zeros((B, lcap)), zmp_type=np.zeros((B, lcap), np.int32),
             length=np.zeros(B, np.int32))
    if want_feet:
        r.update(left=np.zeros((B, lcap, 6)), right=np.zeros((B, lcap, 6)), left_type=np.zeros((B, lcap), np.int32),
                 right_type=np.zeros((B, lcap), np.int32))
    g = lambda k: _hp(r[k]) if k in r else None  # noqa: E731
    _call("wg_zmpdisc_batch", ctx, C.byref(model), B, int(smax), C.addressof(steps), _hp(n_steps), _hp(init_feet), int(lcap),
          g("zmp"), g("zmp_theta"), g("zmp_type"), g("left"), g("left_type"), g("right"), g("right_type"), _hp(r["length"]))
    return r


def zmpdisc_batch_dev(model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, lcap, zx_tm_ptr, zy_tm_ptr, length_ptr,
                      stream=None, ctx=None):
    _call("wg_zmpdisc_batch_dev", ctx, C.byref(model), int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr, int(lcap),
          zx_tm_ptr, zy_tm_ptr, length_ptr, stream)


# ---- the same walk on line: begin, any number of appends, end (include/wg_mpc.h, "steps as they arrive") ----
ZMPDISC_TAIL_MAX = 52


class ZmpDiscState(C.Structure):        # wg_zmpdisc_state_t
    _fields_ = [("support", C.c_double * 6), ("prev_support", C.c_double * 2), ("prev_rel", C.c_double * 2),
                ("ang_support", C.c_double), ("ang_zmp", C.c_double), ("left", C.c_double * 6), ("right", C.c_double * 6),
                ("zmp_last", C.c_double * 3), ("zmp_first", C.c_double * 2), ("last_step", RelStep),
                ("tail", C.c_double * 2 * ZMPDISC_TAIL_MAX)] + \
               [(k, C.c_int) for k in ("left_type", "right_type", "n_samples", "n_steps", "ended", "error", "begun", "pad_")]


ZMPDISC_STATE_BYTES = 1144
ZMPDISC_OUTPUTS = ("zmp_x", "zmp_y", "zmp_theta", "zmp_type", "left", "left_type", "right", "right_type")


def zmpdisc_length_after(model, steps, n_steps, ended=False):
    """samples after the first n_steps steps of `steps` (and after the end phase if `ended`), or a negative code"""
    return int(lib().wg_zmpdisc_length_after(C.byref(model), C.addressof(steps), int(n_steps), int(bool(ended))))


def _zd_outs(outs):
    assert set(outs) <= set(ZMPDISC_OUTPUTS), outs
    return [outs.get(k) for k in ZMPDISC_OUTPUTS]


def zmpdisc_begin_dev(model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, lcap, outs, state_ptr, length_ptr=None,
                      stream=None, ctx=None):
    """InitOnLine on the first n_steps[b] >= 2 steps.  `outs`: device pointers by name (ZMPDISC_OUTPUTS, time-major as
    wg_zmpdisc_full_batch_dev writes them), absent = not wanted; the same set goes to every call of the walk."""
    _call("wg_zmpdisc_begin_dev", ctx, C.byref(model), int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr, int(lcap),
          *_zd_outs(outs), state_ptr, length_ptr, stream)


def zmpdisc_append_dev(model, B, smax, steps_ptr, n_steps_ptr, lcap, outs, state_ptr, length_ptr=None, stream=None, ctx=None):
    """OnLineAddFoot on n_steps[b] >= 0 further steps (`steps`: those of this call, [B][smax]); 0 = the gait sits it out"""
    _call("wg_zmpdisc_append_dev", ctx, C.byref(model), int(B), int(smax), steps_ptr, n_steps_ptr, int(lcap), *_zd_outs(outs),
          state_ptr, length_ptr, stream)


def zmpdisc_end_dev(model, B, lcap, outs, state_ptr, length_ptr=None, select_ptr=None, stream=None, ctx=None):
    """EndPhaseOfTheWalking for every gait, or for those with select[b] != 0"""
    _call("wg_zmpdisc_end_dev", ctx, C.byref(model), int(B), select_ptr, int(lcap), *_zd_outs(outs), state_ptr, length_ptr,
          stream)


# ---- the same walks with a model per gait (include/wg_mpc.h, "The same walks with a model per gait") ----
class ZmpDiscFleet(C.Structure):        # wg_zmpdisc_fleet_t
    _fields_ = [("base", ZmpDiscModel), ("M", C.c_int), ("pad_", C.c_int), ("models", C.c_void_p), ("model_of", C.c_void_p)]


ZMPDISC_FLEET_BYTES = 152


def zmpdisc_fleet(base, M, models_ptr, model_of_ptr=None):
    """wg_zmpdisc_fleet_t: `base` (its T fixes the launch shape), M models on the device, model_of [B] on the device or None
    (M == B, gait b walks with models[b])"""
    return ZmpDiscFleet(base, int(M), 0, models_ptr, model_of_ptr)


def zmpdisc_full_fleet_dev(fleet, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, lcap, outs, length_ptr=None, stream=None,
                           ctx=None):
    """wg_zmpdisc_full_batch_dev with a model per gait; `outs` as in zmpdisc_begin_dev"""
    _call("wg_zmpdisc_full_fleet_dev", ctx, C.byref(fleet), int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr, int(lcap),
          *_zd_outs(outs), length_ptr, stream)


def zmpdisc_begin_fleet_dev(fleet, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, lcap, outs, state_ptr, length_ptr=None,
                            stream=None, ctx=None):
    _call("wg_zmpdisc_begin_fleet_dev", ctx, C.byref(fleet), int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr,
          int(lcap), *_zd_outs(outs), state_ptr, length_ptr, stream)


def zmpdisc_append_fleet_dev(fleet, B, smax, steps_ptr, n_steps_ptr, lcap, outs, state_ptr, length_ptr=None, stream=None,
                             ctx=None):
    _call("wg_zmpdisc_append_fleet_dev", ctx, C.byref(fleet), int(B), int(smax), steps_ptr, n_steps_ptr, int(lcap),
          *_zd_outs(outs), state_ptr, length_ptr, stream)


def zmpdisc_end_fleet_dev(fleet, B, lcap, outs, state_ptr, length_ptr=None, select_ptr=None, stream=None, ctx=None):
    _call("wg_zmpdisc_end_fleet_dev", ctx, C.byref(fleet), int(B), select_ptr, int(lcap), *_zd_outs(outs), state_ptr,
          length_ptr, stream)


# ---- the step stack: command lists -> the steps the zmpdisc calls read (include/wg_mpc.h, "Where the steps come from") ----
STEP_NONE, STEP_SUPPORT_FOOT, STEP_ARC, STEP_LAST_SUPPORT, STEP_ADD, STEP_ONLINE, STEP_ONLINE_IDLE = range(7)
STEPS_BAD_INPUT, STEPS_CAPACITY = -1, -2


class StepCmd(C.Structure):             # wg_step_cmd_t
    _fields_ = [("op", C.c_int), ("foot", C.c_int), ("a", C.c_double * 3)]


class StepStack(C.Structure):           # wg_step_stack_t
    _fields_ = [(k, C.c_int) for k in ("keep", "error", "n_given", "pad_")]


def step_cmds(cmds):
    """(StepCmd * n) from [(op, foot, a0, a1, a2)]"""
    arr = (StepCmd * max(len(cmds), 1))()
    for i, (op, foot, a0, a1, a2) in enumerate(cmds):
        arr[i] = StepCmd(int(op), int(foot), (a0, a1, a2))
    return arr


def steps_count(cmds, n_cmds=None):
    """steps a command list gives (host arithmetic), or STEPS_BAD_INPUT / STEPS_CAPACITY"""
    return int(lib().wg_steps_count(C.addressof(cmds), len(cmds) if n_cmds is None else int(n_cmds)))


def steps_plan(cmds, n_cmds, ss, ds, stack, smax, steps=None):
    """wg_steps_plan for one gait: (steps (RelStep * smax), n_steps); the verdict is in stack.error.  `steps`: an array to write
    into (bytes past the count stay as they are)."""
    steps = (RelStep * int(smax))() if steps is None else steps
    n = C.c_int(-7)
    _check(lib().wg_steps_plan(C.addressof(cmds), int(n_cmds), float(ss), float(ds), C.addressof(stack), int(smax),
                               C.addressof(steps), C.addressof(n)))
    return steps, n.value


def steps_plan_dev(B, ccap, cmds_ptr, n_cmds_ptr, ss, ds, stack_ptr, smax, steps_ptr, n_steps_ptr, stream=None, ctx=None):
    """the same for B gaits on the device: cmds [B][ccap], n_cmds [B], stack [B] in/out, steps [B][smax], n_steps [B]"""
    _call("wg_steps_plan_dev", ctx, int(B), int(ccap), cmds_ptr, n_cmds_ptr, float(ss), float(ds), stack_ptr, int(smax),
          steps_ptr, n_steps_ptr, stream)


def steps_plan_fleet_dev(B, ccap, cmds_ptr, n_cmds_ptr, ss_ptr, ds_ptr, stack_ptr, smax, steps_ptr, n_steps_ptr, stream=None,
                         ctx=None):
    """steps_plan_dev with the support times of each gait: ss, ds [B] on the device"""
    _call("wg_steps_plan_fleet_dev", ctx, int(B), int(ccap), cmds_ptr, n_cmds_ptr, ss_ptr, ds_ptr, stack_ptr, int(smax),
          steps_ptr, n_steps_ptr, stream)


def foot_constraints(time, left, left_type, right, sole_w, sole_h, constraint_x, constraint_y, cap=256):
    """wg_foot_constraints: (polys (ZmpPolytope * n), t_start[n], t_end[n])."""
    time = np.ascontiguousarray(time, dtype=np.float64); left = np.ascontiguousarray(left, dtype=np.float64)
    right = np.ascontiguousarray(right, dtype=np.float64); left_type = np.ascontiguousarray(left_type, dtype=np.int32)
    n = time.shape[0]
    assert left.shape == right.shape == (n, 6) and left_type.shape == (n,)
    polys = (ZmpPolytope * cap)(); ts = np.zeros(cap); te = np.zeros(cap)
    k = lib().wg_foot_constraints(n, _hp(time), _hp(left), _hp(left_type), _hp(right), float(sole_w), float(sole_h),
                                  float(constraint_x), float(constraint_y), cap, C.addressof(polys), _hp(ts), _hp(te))
    _check(min(k, 0))
    if k > cap:
        raise WgError("foot_constraints: %d polytopes, capacity %d" % (k, cap))
    return polys, ts[:k], te[:k], k


# ---- Dimitrov fleets on the device: raw device pointers (ints, e.g. torch tensor.data_ptr()) and a stream ----
def foot_constraints_chunk():
    """samples per time chunk of wg_foot_constraints_batch_dev's kernels"""
    return int(lib().wg_foot_constraints_chunk())


def foot_constraints_batch_dev(B, lcap, length_ptr, time_ptr, left_tm_ptr, left_type_tm_ptr, right_tm_ptr, sole_w, sole_h,
                               constraint_x, constraint_y, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr, stream=None,
                               ctx=None):
    """wg_foot_constraints for B gaits whose feet wg_zmpdisc_full_batch_dev left on the device: queues / t_start / t_end
    [B][qcap], count [B]."""
    _call("wg_foot_constraints_batch_dev", ctx, int(B), int(lcap), length_ptr, time_ptr, left_tm_ptr, left_type_tm_ptr,
          right_tm_ptr, float(sole_w), float(sole_h), float(constraint_x), float(constraint_y), int(qcap), queues_ptr,
          t_start_ptr, t_end_ptr, count_ptr, stream)


def foot_constraints_append_dev(B, lcap, first_sample, done_ptr, length_ptr, time_ptr, left_tm_ptr, left_type_tm_ptr,
                                right_tm_ptr, sole_w, sole_h, constraint_x, constraint_y, qcap, queues_ptr, t_start_ptr,
                                t_end_ptr, count_ptr, stream=None, ctx=None):
    """the same queues grown on line: samples [done[b], length[b]) of every gait are added, done[b] = length[b] afterwards;
    first_sample is a host-side lower bound on every done[b] (0 is always valid)"""
    _call("wg_foot_constraints_append_dev", ctx, int(B), int(lcap), int(first_sample), done_ptr, length_ptr, time_ptr,
          left_tm_ptr, left_type_tm_ptr, right_tm_ptr, float(sole_w), float(sole_h), float(constraint_x), float(constraint_y),
          int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr, stream)


class Sole(C.Structure):                # wg_sole_t
    _fields_ = [(k, C.c_double) for k in ("sole_w", "sole_h", "constraint_x", "constraint_y")]


SOLE_BYTES = 32


def foot_constraints_fleet_dev(B, lcap, length_ptr, time_ptr, left_tm_ptr, left_type_tm_ptr, right_tm_ptr, soles_ptr, qcap,
                               queues_ptr, t_start_ptr, t_end_ptr, count_ptr, stream=None, ctx=None):
    """foot_constraints_batch_dev with a sole per gait: soles (Sole * B) on the device"""
    _call("wg_foot_constraints_fleet_dev", ctx, int(B), int(lcap), length_ptr, time_ptr, left_tm_ptr, left_type_tm_ptr,
          right_tm_ptr, soles_ptr, int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr, stream)


def foot_constraints_append_fleet_dev(B, lcap, first_sample, done_ptr, length_ptr, time_ptr, left_tm_ptr, left_type_tm_ptr,
                                      right_tm_ptr, soles_ptr, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr, stream=None,
                                      ctx=None):
    """foot_constraints_append_dev with a sole per gait"""
    _call("wg_foot_constraints_append_fleet_dev", ctx, int(B), int(lcap), int(first_sample), done_ptr, length_ptr, time_ptr,
          left_tm_ptr, left_type_tm_ptr, right_tm_ptr, soles_ptr, int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr,
          stream)


class ZmpAudit(C.Structure):            # wg_zmp_audit_t
    _fields_ = [("margin", C.c_double), ("worst_sample", C.c_int), ("worst_row", C.c_int), ("n_violated", C.c_int),
                ("n_uncovered", C.c_int), ("n_nonfinite", C.c_int), ("status", C.c_int)]


ZMP_AUDIT_BYTES = 32


def zmp_audit(time, px, py, polys, t_start, t_end, count=None, qcap=None, first_sample=0, n=None, audit=None, margin=None):
    """wg_zmp_audit, one gait on the host: (ZmpAudit, margin[n]).  polys: (ZmpPolytope * k) or its bytes' owner; count / qcap
    default to the number of intervals.  first_sample > 0 folds samples [first_sample, n) into `audit` and `margin` as an earlier
    call left them.  Raises WgError where the call refuses."""
    time = np.ascontiguousarray(time, dtype=np.float64); px = np.ascontiguousarray(px, dtype=np.float64)
    py = np.ascontiguousarray(py, dtype=np.float64)
    t_start = np.ascontiguousarray(t_start, dtype=np.float64); t_end = np.ascontiguousarray(t_end, dtype=np.float64)
    n = time.shape[0] if n is None else int(n)
    qcap = max(1, t_start.shape[0]) if qcap is None else int(qcap)
    count = t_start.shape[0] if count is None else int(count)
    audit = ZmpAudit() if audit is None else audit
    margin = np.zeros(max(n, 0)) if margin is None else margin
    _check(lib().wg_zmp_audit(int(first_sample), n, _hp(time), _hp(px), _hp(py), 1, count, qcap, C.addressof(polys), _hp(t_start),
                              _hp(t_end), C.addressof(audit), _hp(margin)))
    return audit, margin


def zmp_audit_dev(B, lcap, length_ptr, time_ptr, px_tm_ptr, py_tm_ptr, pitch, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr,
                  audit_ptr, margin_tm_ptr=None, stream=None, ctx=None):
    """the walk audit of B gaits on the device: sample k of gait b at [k * pitch + b] of px_tm / py_tm against the queues the
    foot-constraints calls wrote; audit (ZmpAudit * B), margin_tm [lcap][B] or None"""
    _call("wg_zmp_audit_dev", ctx, int(B), int(lcap), length_ptr, time_ptr, px_tm_ptr, py_tm_ptr, int(pitch), int(qcap),
          queues_ptr, t_start_ptr, t_end_ptr, count_ptr, audit_ptr, margin_tm_ptr, stream)


def zmp_audit_append_dev(B, lcap, first_sample, done_ptr, length_ptr, time_ptr, px_tm_ptr, py_tm_ptr, pitch, qcap, queues_ptr,
                         t_start_ptr, t_end_ptr, count_ptr, audit_ptr, margin_tm_ptr=None, stream=None, ctx=None):
    """the same on line: samples [done[b], length[b]) of every gait are folded into audit[b], done[b] = length[b] afterwards;
    first_sample is a host-side lower bound on every done[b] (0 is always valid)"""
    _call("wg_zmp_audit_append_dev", ctx, int(B), int(lcap), int(first_sample), done_ptr, length_ptr, time_ptr, px_tm_ptr,
          py_tm_ptr, int(pitch), int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr, audit_ptr, margin_tm_ptr, stream)


def dimitrov_select_polys_dev(B, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr, t0, polys_ptr, ran_out_ptr=None,
                              stream=None, ctx=None):
    """the queue walk of one tick: polys [B][N] for wg_dimitrov_tick_batch_dev, ran_out [B] or None"""
    _call("wg_dimitrov_select_polys_dev", ctx, int(B), int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr, float(t0),
          polys_ptr, ran_out_ptr, stream)


def dimitrov_tick_batch_dev(B, polys_ptr, states_ptr, outs_ptr=None, max_iter=0, stream=None, ctx=None):
    _call("wg_dimitrov_tick_batch_dev", ctx, int(B), polys_ptr, states_ptr, outs_ptr, int(max_iter), stream)


def dimitrov_walk_dev(B, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr, t0, n_ticks, states_ptr, outs_ptr=None,
                      ran_out_ptr=None, max_iter=0, stream=None, ctx=None):
    """n_ticks x { select at t; tick; t += T } on one stream; outs [n_ticks][B] or None, ran_out [B] or None"""
    _call("wg_dimitrov_walk_dev", ctx, int(B), int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr, float(t0),
          int(n_ticks), states_ptr, outs_ptr, ran_out_ptr, int(max_iter), stream)


DIMITROV_FOLLOW_ALL_FINAL = 1


def dimitrov_follow_dev(B, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr, lcap, time_ptr, have_ptr, walk_ptr, flags,
                        clock_ptr, ticks_ptr, tick_cap, max_ticks, states_ptr, outs_ptr=None, ran_out_ptr=None, max_iter=0,
                        stream=None, ctx=None):
    """max_ticks rounds of { select; tick } in which gait b ticks at its own clock[b] while its own queue covers the tick
    (or is final: walk[b] ended, or DIMITROV_FOLLOW_ALL_FINAL) and ticks[b] < tick_cap; outs [tick_cap][B], absolute rows;
    ran_out is ORed, never cleared (wg_mpc.h)"""
    _call("wg_dimitrov_follow_dev", ctx, int(B), int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr, int(lcap), time_ptr,
          have_ptr, walk_ptr, int(flags), clock_ptr, ticks_ptr, int(tick_cap), int(max_ticks), states_ptr, outs_ptr,
          ran_out_ptr, int(max_iter), stream)


# ---- Dimitrov fleets with a model per gait: the constants as blocks, the fleet launches (wg_mpc.h) ----
class DimitrovFleet(C.Structure):       # wg_dimitrov_fleet_t
    _fields_ = [("N", C.c_int), ("solver", C.c_int), ("M", C.c_int), ("pad_", C.c_int), ("T", C.c_double), ("Tctrl", C.c_double),
                ("blocks", C.c_void_p), ("model_of", C.c_void_p)]


DIMITROV_BLOCK_ARRAYS = ("iLQ", "OptB", "OptC", "Pu", "iPu", "Px", "Q", "OptBq", "OptCq", "PuT", "iPuPx")


def dimitrov_constants_bytes():
    return int(lib().wg_dimitrov_constants_bytes())


def dimitrov_constants_block(model):
    """(rc, block): the model's block as a uint8 array, made on the host; all zeros when rc != 0"""
    blk = np.zeros(dimitrov_constants_bytes(), dtype=np.uint8)
    return int(lib().wg_dimitrov_constants(C.byref(model), _hp(blk))), blk


def dimitrov_constants_unpack(block):
    """the arrays of a host copy of a block, by the names of DIMITROV_BLOCK_ARRAYS, and `model` (N, solver, T, Tctrl, com_height)"""
    blk = np.ascontiguousarray(block, dtype=np.uint8)
    N = int(blk[:4].view(np.int32)[0])
    n = 2 * N
    shapes = dict(iLQ=(n, n), OptB=(n, 6), OptC=(n, n), Pu=(N, N), iPu=(N, N), Px=(N, 3), Q=(n, n), OptBq=(n, 6), OptCq=(n, n),
                  PuT=(N, N), iPuPx=(n, 6))
    out = {k: np.zeros(shapes[k] if N > 0 else (0, 0)) for k in DIMITROV_BLOCK_ARRAYS}
    m = DimitrovModel()
    _check(lib().wg_dimitrov_constants_unpack(_hp(blk), C.addressof(m), *[_hp(out[k]) for k in DIMITROV_BLOCK_ARRAYS]))
    out["model"] = m
    return out


def dimitrov_constants_batch(base, M, com_height=None, alpha=None, beta=None, ctx=None):
    """(blocks [M][bytes] uint8, status [M]) of M models through the device, host arrays in and out"""
    arr = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (com_height, alpha, beta)]
    blocks = np.zeros((M, dimitrov_constants_bytes()), dtype=np.uint8)
    status = np.zeros(M, dtype=np.int32)
    _call("wg_dimitrov_constants_batch", ctx, int(M), C.byref(base), _hp(arr[0]), _hp(arr[1]), _hp(arr[2]), _hp(blocks), _hp(status))
    return blocks, status


def dimitrov_constants_batch_dev(M, base, com_height_ptr, alpha_ptr, beta_ptr, blocks_ptr, status_ptr, stream=None, ctx=None):
    """M blocks and M status ints on the device; a per-model array that is None takes its value from base"""
    _call("wg_dimitrov_constants_batch_dev", ctx, int(M), C.byref(base), com_height_ptr, alpha_ptr, beta_ptr, blocks_ptr,
          status_ptr, stream)


def dimitrov_fleet(base, M, blocks_ptr, model_of_ptr):
    """the descriptor of the fleet launches: N, solver, T, Tctrl of `base`, M blocks and an int per gait on the device"""
    return DimitrovFleet(int(base.N), int(base.solver), int(M), 0, float(base.T), float(base.Tctrl), blocks_ptr, model_of_ptr)


def dimitrov_tick_fleet_dev(B, fleet, polys_ptr, states_ptr, outs_ptr=None, max_iter=0, stream=None, ctx=None):
    """dimitrov_tick_batch_dev with blocks[model_of[g]] as gait g's model; no configured model is read"""
    _call("wg_dimitrov_tick_fleet_dev", ctx, int(B), C.byref(fleet), polys_ptr, states_ptr, outs_ptr, int(max_iter), stream)


def dimitrov_walk_fleet_dev(B, fleet, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr, t0, n_ticks, states_ptr,
                            outs_ptr=None, ran_out_ptr=None, max_iter=0, stream=None, ctx=None):
    """dimitrov_walk_dev with a model per gait"""
    _call("wg_dimitrov_walk_fleet_dev", ctx, int(B), C.byref(fleet), int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr,
          float(t0), int(n_ticks), states_ptr, outs_ptr, ran_out_ptr, int(max_iter), stream)


def dimitrov_follow_fleet_dev(B, fleet, qcap, queues_ptr, t_start_ptr, t_end_ptr, count_ptr, lcap, time_ptr, have_ptr, walk_ptr,
                              flags, clock_ptr, ticks_ptr, tick_cap, max_ticks, states_ptr, outs_ptr=None, ran_out_ptr=None,
                              max_iter=0, stream=None, ctx=None):
    """dimitrov_follow_dev with a model per gait"""
    _call("wg_dimitrov_follow_fleet_dev", ctx, int(B), C.byref(fleet), int(qcap), queues_ptr, t_start_ptr, t_end_ptr, count_ptr,
          int(lcap), time_ptr, have_ptr, walk_ptr, int(flags), clock_ptr, ticks_ptr, int(tick_cap), int(max_ticks), states_ptr,
          outs_ptr, ran_out_ptr, int(max_iter), stream)


def dimitrov_walk_time(t0, n_ticks, ctx=None):
    """the t at which tick n_ticks of a walk started at t0 selects (the walk's own repeated addition of the configured T)"""
    t = float(_raw("wg_dimitrov_walk_time", ctx, float(t0), int(n_ticks)))
    if t != t:
        raise WgError("dimitrov_walk_time: " + lib().wg_last_error().decode())
    return t


def dimitrov_walk_safe_ticks(t0, t_have, ctx=None):
    """ticks from t0 on whose N previewed instants all lie at or before t_have"""
    n = int(_raw("wg_dimitrov_walk_safe_ticks", ctx, float(t0), float(t_have)))
    _check(min(n, 0))
    return n


# ---- Herdt fleets with a model per gait: blocks (the model and its tick tables), the fleet launches (wg_mpc.h) ----
class MpcFleet(C.Structure):            # wg_mpc_fleet_t
    _fields_ = [("base", Model), ("M", C.c_int), ("pad_", C.c_int), ("blocks", C.c_void_p), ("model_of", C.c_void_p)]


IFAIL_NO_MODEL = -1                     # WG_IFAIL_NO_MODEL
MPC_BLOCK_ARRAYS = ("Sv", "Sz", "Uv", "Uz", "Qb", "R2", "Z2")
_NMAXH = 32                             # wg::kNMaxH: the tables are laid out for it
MPC_BLOCK_TABLES = 256                  # where the tables start in a block
MPC_BLOCK_TABLES_BYTES = 8 * (2 * 3 * _NMAXH + 3 * _NMAXH * _NMAXH + _NMAXH * (2 * _NMAXH + 1) + 4 * _NMAXH * _NMAXH) + 16 + \
    8 * (_NMAXH * _NMAXH // 64)


def mpc_block_bytes():
    return int(lib().wg_mpc_block_bytes())


def mpc_block(model):
    """(rc, block): the model's block as a uint8 array, made on the host; all zeros when rc != 0"""
    blk = np.zeros(mpc_block_bytes(), dtype=np.uint8)
    return int(lib().wg_mpc_block(C.byref(model), _hp(blk))), blk


def mpc_block_unpack(block):
    """the arrays of a host copy of a block at the block's own N, by the names of MPC_BLOCK_ARRAYS (R2 packed, Z2 column-major
    with leading dimension 2N), `sign` (the sign words of Z2's cross block, read from the block's bytes), `diag_b`, `blocks_ok`
    and `model`"""
    blk = np.ascontiguousarray(block, dtype=np.uint8)
    N = int(blk[:4].view(np.int32)[0])
    n = 2 * N
    shapes = dict(Sv=(N, 3), Sz=(N, 3), Uv=(N, N), Uz=(N, N), Qb=(N, N), R2=(n * (n + 1) // 2,), Z2=(n * n,))
    out = {k: np.zeros(shapes[k]) for k in MPC_BLOCK_ARRAYS}
    m = Model()
    diag_b, ok = C.c_double(0.0), C.c_int(0)
    _check(lib().wg_mpc_block_unpack(_hp(blk), C.addressof(m), *[_hp(out[k]) for k in MPC_BLOCK_ARRAYS], C.addressof(diag_b),
                                     C.addressof(ok)))
    end = MPC_BLOCK_TABLES + MPC_BLOCK_TABLES_BYTES
    out["sign"] = blk[end - 8 * (_NMAXH * _NMAXH // 64):end].view(np.uint64).copy()
    out["diag_b"], out["blocks_ok"], out["model"] = diag_b.value, ok.value, m
    return out


def mpc_blocks_batch(models, ctx=None):
    """(blocks [M][bytes] uint8, status [M]) of the models through the device, host arrays in and out"""
    M = len(models)
    arr = (Model * M)(*models)
    blocks = np.zeros((M, mpc_block_bytes()), dtype=np.uint8)
    status = np.zeros(M, dtype=np.int32)
    _call("wg_mpc_blocks_batch", ctx, M, C.addressof(arr), _hp(blocks), _hp(status))
    return blocks, status


def mpc_blocks_batch_dev(M, models_ptr, blocks_ptr, status_ptr, stream=None, ctx=None):
    """M blocks and M status ints on the device from M wg_model_t on the device"""
    _call("wg_mpc_blocks_batch_dev", ctx, int(M), models_ptr, blocks_ptr, status_ptr, stream)


def mpc_fleet(base, M, blocks_ptr, model_of_ptr):
    """the descriptor of the fleet launches: `base` decides the launch plan, M blocks and an int per gait on the device"""
    return MpcFleet(Model.from_buffer_copy(bytes(base)), int(M), 0, blocks_ptr, model_of_ptr)


def _fleet_ref(fleet):
    return None if fleet is None else C.byref(fleet)


def mpc_tick_fleet_dev(B, fleet, states_ptr, outs_ptr=None, diag_ptr=None, advance_calls=0, hist_ptr=None, hist_cap=0,
                       hist_len_ptr=None, stream=None, ctx=None):
    """mpc_tick_batch_dev with blocks[model_of[g]] as gait g's model; no configured model is read.  Returns the raw code."""
    return int(_raw("wg_mpc_tick_fleet_dev", ctx, int(B), _fleet_ref(fleet), states_ptr, outs_ptr, diag_ptr, int(advance_calls), hist_ptr,
                    int(hist_cap), hist_len_ptr, stream))


def mpc_run_fleet_dev(B, fleet, states_ptr, n_ticks, advance_calls=20, vref_sched_ptr=None, period=1, outs_ptr=None,
                      diag_ptr=None, stream=None, ctx=None):
    """mpc_run_sched_dev with a model per gait (vref_sched_ptr None: the unstaged run).  Returns the raw code."""
    return int(_raw("wg_mpc_run_fleet_dev", ctx, int(B), _fleet_ref(fleet), states_ptr, int(n_ticks), int(advance_calls), vref_sched_ptr,
                    int(period), outs_ptr, diag_ptr, stream))


# ---- invariant Hessian block on the matrix cores ----
GRAMIAN_F64 = 0
GRAMIAN_F32 = 1


def gramian_batch(N, T, h, alpha, beta, gamma, precision=GRAMIAN_F64, ctx=None):
    """Q_b[B, N, N] for models with sampling periods T[B] and CoM heights h[B] (wg_gramian_batch)."""
    T = np.ascontiguousarray(T, dtype=np.float64); h = np.ascontiguousarray(h, dtype=np.float64)
    B = T.shape[0]
    Qb = np.zeros((B, N, N))
    _call("wg_gramian_batch", ctx, B, int(N), _hp(T), _hp(h), alpha, beta, gamma, int(precision), _hp(Qb))
    return Qb


# ---- Morisawa-2007 analytic walks: CoM, ZMP and feet of a step sequence in closed form (include/wg_mpc.h) ----
MORISAWA_MAX_STEPS = 14
MORISAWA_BAD_INPUT, MORISAWA_CAPACITY, MORISAWA_SINGULAR = -1, -2, -3
MORISAWA_OUTPUTS = ("zmp_x", "zmp_y", "com", "left", "left_type", "right", "right_type")


class MorisawaModel(C.Structure):       # wg_morisawa_model_t
    _fields_ = [(k, C.c_double) for k in ("T", "t_single", "t_double", "step_height", "omega")]


class MorisawaView(C.Structure):        # wg_morisawa_view_t
    _fields_ = [(k, C.c_int) for k in ("n_steps", "n_int", "n", "smax")] + [("com_height", C.c_double), ("t_total", C.c_double)] + \
               [(k, _dp) for k in ("dT", "omega", "tref", "zmp_x", "cog_x", "zmp_y", "cog_y", "Vx", "Wx", "Vy", "Wy", "left", "right")] + \
               [("left_type", _ip), ("right_type", _ip)] + \
               [(k, _dp) for k in ("profile_x", "profile_y", "support", "wx", "wy", "yx", "yy")] + \
               [("piv", _ip), ("lu", _dp), ("lu_pitch", C.c_int), ("pad_", C.c_int)]


def morisawa_defaults():
    m = MorisawaModel()
    lib().wg_morisawa_defaults(C.byref(m))
    return m


_MO, _MOL = "wg_morisawa_", "wg_morisawa_long_"       # the two families: one set of wrappers, the prefix chooses


def _mo_block_bytes(fam, smax):
    return int(getattr(lib(), fam + "block_bytes")(int(smax)))


def _mo_length(fam, model, n_steps, t_start):
    return int(getattr(lib(), fam + "length")(C.byref(model), int(n_steps), float(t_start)))


def morisawa_block_bytes(smax):
    return _mo_block_bytes(_MO, smax)


def morisawa_length(model, n_steps, t_start):
    return _mo_length(_MO, model, n_steps, t_start)


def morisawa_coshsinh(x):
    c, s = C.c_double(), C.c_double()
    _check(lib().wg_morisawa_coshsinh(float(x), C.byref(c), C.byref(s)))
    return c.value, s.value


def morisawa_system(model, steps, init_feet, com0):
    """Z [n, n], w of x, w of y of one gait before the elimination (host arithmetic); steps: (RelStep * S)"""
    S = len(steps)
    n = 4 * S + 8
    Z, wx, wy = np.zeros((n, n)), np.zeros(n), np.zeros(n)
    feet, com = np.ascontiguousarray(init_feet, dtype=np.float64), np.ascontiguousarray(com0, dtype=np.float64)
    rc = lib().wg_morisawa_system(C.byref(model), S, C.addressof(steps), _hp(feet), _hp(com), _hp(Z), _hp(wx), _hp(wy))
    if rc != n:
        raise WgError(f"wg_morisawa_system: {rc}")
    return Z, wx, wy


def _mo_solve(fam, model, steps, n_steps, init_feet, com0, smax, blocks):
    n_steps = np.ascontiguousarray(n_steps, dtype=np.int32); B = n_steps.shape[0]
    init_feet = np.ascontiguousarray(init_feet, dtype=np.float64); com0 = np.ascontiguousarray(com0, dtype=np.float64)
    assert init_feet.shape == (B, 6) and com0.shape == (B, 3) and len(steps) == B * smax
    if blocks is None:
        blocks = np.zeros((B, _mo_block_bytes(fam, smax) // 8))
    status = np.zeros(B, np.int32)
    fleet = not isinstance(model, MorisawaModel)
    fn = getattr(lib(), fam + ("solve_fleet" if fleet else "solve"))
    _check(fn(C.addressof(model), B, int(smax), C.addressof(steps), _hp(n_steps), _hp(init_feet), _hp(com0), _hp(blocks), _hp(status)))
    return blocks, status


def morisawa_solve(model, steps, n_steps, init_feet, com0, smax, blocks=None):
    """Host twin.  model: one MorisawaModel, or (MorisawaModel * B) for a model per gait; steps: (RelStep * (B*smax)); n_steps [B];
    init_feet [B, 6]; com0 [B, 3].  Returns (blocks [B, words] float64 -- `blocks` itself if given -- , status [B])."""
    return _mo_solve(_MO, model, steps, n_steps, init_feet, com0, smax, blocks)


def _mo_view(fam, block, smax):
    block = np.ascontiguousarray(block, dtype=np.float64)
    v = MorisawaView()
    rc = getattr(lib(), fam + "block_unpack")(_hp(block), int(smax), C.byref(v))
    if rc != 0:
        raise WgError(f"{fam}block_unpack: {rc}")
    I, n, S = v.n_int, v.n, v.n_steps
    arr = lambda p, *shape: np.ctypeslib.as_array(p, shape=shape).copy()  # noqa: E731
    r = dict(n_steps=S, n_int=I, n=n, smax=v.smax, com_height=v.com_height, t_total=v.t_total)
    for k in ("dT", "omega", "tref", "Vx", "Wx", "Vy", "Wy", "profile_x", "profile_y", "left_type", "right_type"):
        r[k] = arr(getattr(v, k), I)
    for k in ("zmp_x", "cog_x", "zmp_y", "cog_y"):
        r[k] = arr(getattr(v, k), I, 5)
    for k in ("left", "right"):
        r[k] = arr(getattr(v, k), I, 6, 6)
    r["support"] = arr(v.support, S, 3)
    for k in ("wx", "wy", "yx", "yy", "piv"):
        r[k] = arr(getattr(v, k), n)
    if fam == _MOL:
        r["band"] = arr(v.lu, n, v.lu_pitch)        # row i: columns i - 5 .. i + 9 in words 0 .. 14, multipliers where they were made
    else:
        r["lu"] = arr(v.lu, v.lu_pitch, v.lu_pitch)[:n, :n]
    return r


def morisawa_view(block, smax):
    """dict of numpy arrays (copies) from one block: what wg_morisawa_block_unpack points at, cut to the gait's own sizes"""
    return _mo_view(_MO, block, smax)


def _mo_sample(fam, blocks, status, smax, t_start, T, lcap, want, into):
    blocks = np.ascontiguousarray(blocks, dtype=np.float64); B = blocks.shape[0]
    shapes = dict(zmp_x=(lcap, B), zmp_y=(lcap, B), com=(lcap, 4, B), left=(lcap, 6, B), right=(lcap, 6, B), left_type=(lcap, B),
                  right_type=(lcap, B))
    r = {}
    for k in want:
        r[k] = into[k] if into is not None and k in into else np.zeros(shapes[k], np.int32 if k.endswith("type") else np.float64)
        assert r[k].shape == shapes[k] and r[k].flags.c_contiguous
    r["length"] = into["length"] if into is not None and "length" in into else np.zeros(B, np.int32)
    st = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    _check(getattr(lib(), fam + "sample")(B, int(smax), _hp(blocks), _hp(st), float(t_start), float(T), int(lcap),
                                          *[_hp(r.get(k)) for k in MORISAWA_OUTPUTS], _hp(r["length"])))
    return r


def morisawa_sample(blocks, status, smax, t_start, T, lcap, want=MORISAWA_OUTPUTS, into=None):
    """Host twin of the sampler.  Returns dict(zmp_x, zmp_y [lcap, B], com [lcap, 4, B], left, right [lcap, 6, B], left_type,
    right_type [lcap, B] int32, length [B]) with the outputs named in `want`; `into`: arrays to write into instead of zeros."""
    return _mo_sample(_MO, blocks, status, smax, t_start, T, lcap, want, into)


def _mo_outs(outs):
    assert set(outs) <= set(MORISAWA_OUTPUTS), outs
    return [outs.get(k) for k in MORISAWA_OUTPUTS]


def _mo_solve_dev(fam, model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, stream, ctx):
    if isinstance(model, MorisawaModel):
        _call(fam + "solve_dev", ctx, C.addressof(model), int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr,
              com0_ptr, blocks_ptr, status_ptr, stream)
    else:
        _call(fam + "solve_fleet_dev", ctx, model, int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr,
              blocks_ptr, status_ptr, stream)


def _mo_sample_dev(fam, B, smax, blocks_ptr, status_ptr, t_start, T, lcap, outs, length_ptr, stream, ctx):
    _call(fam + "sample_dev", ctx, int(B), int(smax), blocks_ptr, status_ptr, float(t_start), float(T), int(lcap),
          *_mo_outs(outs), length_ptr, stream)


def _mo_walk_dev(fam, model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, t_start, lcap, outs,
                 length_ptr, stream, T, ctx):
    if isinstance(model, MorisawaModel):
        _call(fam + "walk_dev", ctx, C.addressof(model), int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr,
              com0_ptr, blocks_ptr, status_ptr, float(t_start), int(lcap), *_mo_outs(outs), length_ptr, stream)
    else:
        _call(fam + "walk_fleet_dev", ctx, model, float(T), int(B), int(smax), steps_ptr, n_steps_ptr, init_feet_ptr,
              com0_ptr, blocks_ptr, status_ptr, float(t_start), int(lcap), *_mo_outs(outs), length_ptr, stream)


def morisawa_solve_dev(model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, stream=None,
                       ctx=None):
    """every pointer a device pointer; `model`: a MorisawaModel (host), or a device pointer to B of them (the fleet form)"""
    _mo_solve_dev(_MO, model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, stream, ctx)


def morisawa_sample_dev(B, smax, blocks_ptr, status_ptr, t_start, T, lcap, outs, length_ptr=None, stream=None, ctx=None):
    """`outs`: device pointers by name (MORISAWA_OUTPUTS, time-major), absent = not wanted"""
    _mo_sample_dev(_MO, B, smax, blocks_ptr, status_ptr, t_start, T, lcap, outs, length_ptr, stream, ctx)


def morisawa_walk_dev(model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, t_start, lcap,
                      outs, length_ptr=None, stream=None, T=None, ctx=None):
    """solve and sample on one stream; `model` as in morisawa_solve_dev, the fleet form needs the common sampling period T"""
    _mo_walk_dev(_MO, model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, t_start, lcap, outs,
                 length_ptr, stream, T, ctx)


# ---- the long family (wg_morisawa_long_*): walks of up to MORISAWA_LONG_MAX_STEPS steps, Z eliminated as a band.  The same
# arguments and results as the wrappers above; blocks of the two families are not interchangeable ----
MORISAWA_LONG_MAX_STEPS = 64
MORISAWA_BAND_PITCH, MORISAWA_BAND_KL, MORISAWA_BAND_KU = 16, 5, 9     # row i of the band: columns i - 5 .. i + 9


def morisawa_long_block_bytes(smax):
    return _mo_block_bytes(_MOL, smax)


def morisawa_long_length(model, n_steps, t_start):
    return _mo_length(_MOL, model, n_steps, t_start)


def morisawa_long_system(model, steps, init_feet, com0):
    """Z before the elimination in row-band form [n, 16] (entry (i, c) at [i, c - i + 5]), w of x, w of y; steps: (RelStep * S)"""
    S = len(steps)
    n = 4 * S + 8
    Zb, wx, wy = np.zeros((n, MORISAWA_BAND_PITCH)), np.zeros(n), np.zeros(n)
    feet, com = np.ascontiguousarray(init_feet, dtype=np.float64), np.ascontiguousarray(com0, dtype=np.float64)
    rc = lib().wg_morisawa_long_system(C.byref(model), S, C.addressof(steps), _hp(feet), _hp(com), _hp(Zb), _hp(wx), _hp(wy))
    if rc != n:
        raise WgError(f"wg_morisawa_long_system: {rc}")
    return Zb, wx, wy


def morisawa_band_to_dense(band):
    """[n, 16] row band -> [n, n]"""
    n = band.shape[0]
    Z = np.zeros((n, n))
    for i in range(n):
        lo, hi = max(0, i - MORISAWA_BAND_KL), min(n - 1, i + MORISAWA_BAND_KU)
        Z[i, lo:hi + 1] = band[i, lo - i + MORISAWA_BAND_KL:hi - i + MORISAWA_BAND_KL + 1]
    return Z


def morisawa_long_solve(model, steps, n_steps, init_feet, com0, smax, blocks=None):
    """Host twin of the long solve: morisawa_solve's arguments and results"""
    return _mo_solve(_MOL, model, steps, n_steps, init_feet, com0, smax, blocks)


def morisawa_long_view(block, smax):
    """morisawa_view of a long block; in place of "lu" it has "band" [n, 16] (see include/wg_mpc.h for the convention)"""
    return _mo_view(_MOL, block, smax)


def morisawa_long_sample(blocks, status, smax, t_start, T, lcap, want=MORISAWA_OUTPUTS, into=None):
    return _mo_sample(_MOL, blocks, status, smax, t_start, T, lcap, want, into)


def morisawa_long_solve_dev(model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, stream=None,
                            ctx=None):
    _mo_solve_dev(_MOL, model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, stream, ctx)


def morisawa_long_sample_dev(B, smax, blocks_ptr, status_ptr, t_start, T, lcap, outs, length_ptr=None, stream=None, ctx=None):
    _mo_sample_dev(_MOL, B, smax, blocks_ptr, status_ptr, t_start, T, lcap, outs, length_ptr, stream, ctx)


def morisawa_long_walk_dev(model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, t_start, lcap,
                           outs, length_ptr=None, stream=None, T=None, ctx=None):
    _mo_walk_dev(_MOL, model, B, smax, steps_ptr, n_steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, t_start, lcap, outs,
                 length_ptr, stream, T, ctx)


# ---- the re-plan from a block's kept factor (wg_morisawa_resolve*, wg_morisawa_long_resolve*): new steps, feet and start CoM x, y
# on the timing of a solved block; the bytes of the full solve without building or eliminating Z.  A gait's step count is its
# factor block's; `factor_of` [B] names each gait's factor block (None: block 0) ----
def _mo_resolve(fam, model, factors, factor_of, steps, init_feet, com0, smax, blocks):
    init_feet = np.ascontiguousarray(init_feet, dtype=np.float64); com0 = np.ascontiguousarray(com0, dtype=np.float64)
    B = init_feet.shape[0]
    words = _mo_block_bytes(fam, smax) // 8
    factors = np.ascontiguousarray(factors, dtype=np.float64).reshape(-1, words)
    fo = None if factor_of is None else np.ascontiguousarray(factor_of, dtype=np.int32)
    assert init_feet.shape == (B, 6) and com0.shape == (B, 3) and len(steps) == B * smax and (fo is None or fo.shape == (B,))
    if blocks is None:
        blocks = np.zeros((B, words))
    status = np.zeros(B, np.int32)
    fleet = not isinstance(model, MorisawaModel)
    fn = getattr(lib(), fam + ("resolve_fleet" if fleet else "resolve"))
    _check(fn(C.addressof(model), B, int(smax), _hp(factors), factors.shape[0], _hp(fo), C.addressof(steps), _hp(init_feet), _hp(com0),
              _hp(blocks), _hp(status)))
    return blocks, status


def morisawa_resolve(model, factors, factor_of, steps, init_feet, com0, smax, blocks=None):
    """Host twin.  model as in morisawa_solve; factors [F, words] solved blocks of this smax; factor_of [B] or None; steps
    (RelStep * (B*smax)); init_feet [B, 6]; com0 [B, 3] with the factor block's height.  Returns (blocks, status) as morisawa_solve."""
    return _mo_resolve(_MO, model, factors, factor_of, steps, init_feet, com0, smax, blocks)


def morisawa_long_resolve(model, factors, factor_of, steps, init_feet, com0, smax, blocks=None):
    return _mo_resolve(_MOL, model, factors, factor_of, steps, init_feet, com0, smax, blocks)


def _mo_resolve_dev(fam, model, B, smax, factors_ptr, n_factors, factor_of_ptr, steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr,
                    stream, ctx):
    fleet = not isinstance(model, MorisawaModel)
    _call(fam + ("resolve_fleet_dev" if fleet else "resolve_dev"), ctx, model if fleet else C.addressof(model), int(B), int(smax),
          factors_ptr, int(n_factors), factor_of_ptr, steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr, stream)


def morisawa_resolve_dev(model, B, smax, factors_ptr, n_factors, factor_of_ptr, steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr,
                         status_ptr, stream=None, ctx=None):
    """every pointer a device pointer (factor_of_ptr may be None); `model` as in morisawa_solve_dev.  `blocks` must not overlap
    `factors`; morisawa_sample_dev on the same stream samples the new walks"""
    _mo_resolve_dev(_MO, model, B, smax, factors_ptr, n_factors, factor_of_ptr, steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr,
                    stream, ctx)


def morisawa_long_resolve_dev(model, B, smax, factors_ptr, n_factors, factor_of_ptr, steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr,
                              status_ptr, stream=None, ctx=None):
    _mo_resolve_dev(_MOL, model, B, smax, factors_ptr, n_factors, factor_of_ptr, steps_ptr, init_feet_ptr, com0_ptr, blocks_ptr, status_ptr,
                    stream, ctx)
