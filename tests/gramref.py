"""Test infrastructure (no tests): a reference of the SAME operation as wg_gramian_kernel (csrc/wg_gramian_device.hpp), an
entrywise error bound that is derived and not fitted, and a numpy model of the kernel's arithmetic that can be broken on purpose.

    Q_b = beta I + alpha Uv'Uv + gamma Uz'Uz          (generator-vel-ref.cpp:587-614 on the maps of rigid-body-system.cpp:377-452)

operands   Uv, Uz as the float64 values of the reference's left-to-right expressions (rigid-body-system.cpp:404-441), the same
           operations in the same order; in f32 mode rounded to float32 as the kernel rounds them.  Everything below takes these
           as given: rounding the operands is part of the operation, not of its error.
exact      the two products of those operands in np.longdouble (64-bit significand on x86-64), combined as
           beta I + alpha Pv + gamma Pz in np.longdouble; exact_fraction does the same in fractions.Fraction.
bound      (2 N + 2) u_p (alpha |Uv|'|Uv| + gamma |Uz|'|Uz|) + 4 * 2^-53 (beta delta + alpha |Pv| + gamma |Pz|), entrywise.
           An entry of a product is a sum of at most N products.  However they are ordered, fused or not, every partial result
           passes through at most N product roundings and N additions on its way out; 2 N + 2 relative errors of u_p on terms
           whose magnitudes sum to (|U|'|U|)_ij bound the error to first order by (2 N + 2) u_p (|U|'|U|)_ij (Higham, Accuracy
           and Stability of Numerical Algorithms, 3.1; the two spare roundings absorb the second-order term for N <= 32).
           u_p = 2^-53 for v_mfma_f64; u_p = 2^-23, not 2^-24, for the f32 form, which allows an accumulator that truncates.
           The epilogue is three float64 multiply-adds, q = 0 + delta beta, q += Pv alpha, q += Pz gamma: at most 4 roundings of
           2^-53 each on partial sums no larger than beta delta + alpha |Pv| + gamma |Pz|.
emulate    the kernel's arithmetic in numpy: operands of the operand type, one accumulator per entry in the operand type, k in
           ascending blocks of 4 (one rounding per product, one per addition), tiles of 16 x 16, the float64 epilogue in the
           kernel's order.  `fault` breaks it in one of four ways (see FAULTS).

T and h may be scalars or arrays [B]; results are [N][N] or [B][N][N]."""
import fractions
import functools

import numpy as np

F64, F32 = 0, 1                                # WG_GRAMIAN_F64 / WG_GRAMIAN_F32
U_P = {F64: 2.0 ** -53, F32: 2.0 ** -23}
FAULTS = ("no_uz",                             # the CoP accumulator is dropped
          "f64_rows_in_f32",                   # f32 mode stores result register r of lane l at row (l >> 4) + 4 r, the f64 map
          "short_k",                           # the k-loop ends at 4 floor(N / 4)
          "transposed_tile")                   # tile (ti, tj) is stored at (tj, ti)
WEIGHTS = ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 1e-5, 1e-6))       # (alpha, beta, gamma); the last: the reference's
REF_MODEL = (0.1, 0.814)                       # T, CoM height of the reference


def _key(a):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def _operands(N, Tb, hb, prec):
    T, h = np.frombuffer(Tb)[:, None, None], np.frombuffer(hb)[:, None, None]
    k, i = np.arange(N)[None, :, None], np.arange(N)[None, None, :]
    d = np.maximum(k - i, 0).astype(np.float64)
    low = i <= k
    uv = np.where(low, (2 * d + 1) * T * T * 0.5, 0.0)
    uz = np.where(low, (1 + 3 * d + 3 * d * d) * T * T * T / 6.0 - T * h / 9.81, 0.0)
    if prec == F32:
        uv, uz = uv.astype(np.float32).astype(np.float64), uz.astype(np.float32).astype(np.float64)
    return uv, uz


def _shape(x, T):
    return x if np.ndim(T) else x[0]


def operands(N, T, h, prec):
    """(Uv, Uz), [k][i], float64 values (in f32 mode: of float32 numbers)"""
    uv, uz = _operands(int(N), _key(T), _key(h), int(prec))
    return _shape(uv, T), _shape(uz, T)


@functools.lru_cache(maxsize=None)
def _products(N, Tb, hb, prec):
    """(Pv, Pz, |Uv|'|Uv|, |Uz|'|Uz|) in np.longdouble, [B][N][N]"""
    uv, uz = (u.astype(np.longdouble) for u in _operands(N, Tb, hb, prec))
    g = lambda u: np.einsum("bki,bkj->bij", u, u)  # noqa: E731
    return g(uv), g(uz), g(np.abs(uv)), g(np.abs(uz))


def exact(N, T, h, alpha, beta, gamma, prec):
    """beta I + alpha Uv'Uv + gamma Uz'Uz of operands(...), np.longdouble"""
    pv, pz, _, _ = _products(int(N), _key(T), _key(h), int(prec))
    ld = np.longdouble
    return _shape(ld(beta) * np.eye(N, dtype=ld)[None] + ld(alpha) * pv + ld(gamma) * pz, T)


def exact_fraction(N, T, h, alpha, beta, gamma, prec):
    """the same in exact rational arithmetic, one model: [N][N] of Fractions"""
    uv, uz = operands(N, float(T), float(h), prec)
    Fr = fractions.Fraction
    fv, fz = [[Fr(float(x)) for x in row] for row in uv], [[Fr(float(x)) for x in row] for row in uz]
    a, b, c = Fr(float(alpha)), Fr(float(beta)), Fr(float(gamma))
    return [[b * (i == j) + a * sum(fv[k][i] * fv[k][j] for k in range(N)) + c * sum(fz[k][i] * fz[k][j] for k in range(N))
             for j in range(N)] for i in range(N)]


def bound(N, T, h, alpha, beta, gamma, prec):
    """the entrywise bound of the module docstring, np.longdouble"""
    pv, pz, av, az = _products(int(N), _key(T), _key(h), int(prec))
    ld = np.longdouble
    a, b, c = ld(abs(alpha)), ld(abs(beta)), ld(abs(gamma))
    first = ld(2 * N + 2) * ld(U_P[prec]) * (a * av + c * az)
    second = ld(4) * ld(2.0 ** -53) * (b * np.eye(N, dtype=ld)[None] + a * np.abs(pv) + c * np.abs(pz))
    return _shape(first + second, T)


@functools.lru_cache(maxsize=None)
def _accumulate(N, Tb, hb, prec, short_k):
    """the kernel's two accumulators for one model, padded to whole tiles: (Pv, Pz) [P][P] float64 values of the operand type"""
    dt = np.float32 if prec == F32 else np.float64
    uv, uz = (u[0] for u in _operands(N, Tb, hb, prec))
    P = 16 * ((N + 15) // 16)
    out = []
    for u in (uv, uz):
        pad = np.zeros((4 * ((N + 3) // 4), P), dt)                # rows k >= N and columns >= N are the kernel's zeros
        pad[:N, :N] = u.astype(dt)
        acc = np.zeros((P, P), dt)
        for k0 in range(0, 4 * (N // 4) if short_k else N, 4):     # one MFMA: four k, ascending
            for k in range(k0, k0 + 4):
                acc = acc + pad[k][:, None] * pad[k][None, :]       # numpy rounds the product and the sum to dt
        out.append(acc.astype(np.float64))
    return out


def emulate(N, T, h, alpha, beta, gamma, prec, fault=None):
    """the kernel's result for ONE model by the numpy model of its arithmetic, float64 [N][N]"""
    assert fault is None or fault in FAULTS
    pv, pz = _accumulate(int(N), _key(float(T)), _key(float(h)), int(prec), fault == "short_k")
    if fault == "no_uz":
        pz = np.zeros_like(pz)
    P = pv.shape[0]
    q = np.zeros((P, P))
    q += np.eye(P) * beta                                           # generator-vel-ref.cpp:592-613: += in call order
    q += pv * alpha
    q += pz * gamma
    out = np.full((N, N), np.nan)
    for ti in range(P // 16):
        for tj in range(P // 16):
            tile = q[16 * ti:16 * ti + 16, 16 * tj:16 * tj + 16]
            if fault == "f64_rows_in_f32" and prec == F32:          # lane l, register r holds row 4 (l >> 4) + r; stored at (l >> 4) + 4 r
                moved = np.empty_like(tile)
                for kq in range(4):
                    for r in range(4):
                        moved[kq + 4 * r] = tile[4 * kq + r]
                tile = moved
            r0, c0 = (16 * tj, 16 * ti) if fault == "transposed_tile" else (16 * ti, 16 * tj)
            rows, cols = min(16, N - r0), min(16, N - c0)
            if rows > 0 and cols > 0:
                out[r0:r0 + rows, c0:c0 + cols] = tile[:rows, :cols]
    return out
