// wg_riccati_math.hpp -- the arithmetic of the Kajita preview-control gains, once, for the host calls (wg_riccati.cpp:
// wg_riccati_solve / wg_riccati_gains) and the kernel (wg_riccati_kernels.hpp: wg_riccati_gains_batch_dev).
//
//   OptimalControllerSolver::ComputeWeights     src/PreviewControl/OptimalControllerSolver.cpp:200-352
//   PreviewControl::ComputeOptimalWeights       src/PreviewControl/PreviewControl.cpp:198-322   (the cart-table set-up)
//
// The reference obtains the stabilising solution P of
//     P = A'PA - A'Pb (R + b'Pb)^-1 b'PA + c'Qc
// from an ordered generalised Schur form of the symplectic pencil (LAPACK dgges, OptimalControllerSolver.cpp:133-198).  The
// system is 3x3 / 4x4, so P is computed here with the structure-preserving doubling algorithm (quadratically convergent, same
// fixed point: the unique stabilising solution) followed by two fixed-point polishing steps of the Riccati map.  Everything
// downstream of P (K, the F recursion) follows the reference's operation order.
//
// Plain C++ that a HIP translation unit compiles for both sides: WG_RC_HD is `__host__ __device__` there and nothing elsewhere,
// and nothing here names a kernel, a lane or a block index.  The library is built with -ffp-contract=off and / is IEEE on both
// sides, so host and kernel give the same bytes.  The order n is a template argument and every loop has constant bounds: in the
// kernel a matrix is a set of registers, never dynamically indexed scratch (the pivot row of `solve` is found by comparison and
// swapped under a predicate, not addressed).
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/wg_mpc.h"
#ifdef __HIP__
#define WG_RC_HD __host__ __device__
#else
#define WG_RC_HD
#endif
#define WG_RC_INLINE WG_RC_HD inline __attribute__((always_inline))

namespace wg {

constexpr int kRcMaxN = 8;                          // wg_riccati_solve's largest order
// a double is finite iff x - x == 0 (inf - inf and nan - nan are nan); <cmath>'s isfinite is not spelt alike on both sides
WG_RC_INLINE bool rc_finite(double x) { return x - x == 0.0; }

template <int R, int C>
struct RcMat {
  double v[R * C];
  WG_RC_INLINE double &operator()(int i, int j) { return v[i * C + j]; }
  WG_RC_INLINE double operator()(int i, int j) const { return v[i * C + j]; }
};

template <int R, int C>
WG_RC_INLINE RcMat<R, C> rc_zeros() {
  RcMat<R, C> m;
#pragma unroll
  for (int i = 0; i < R * C; i++) m.v[i] = 0.0;
  return m;
}
template <int N>
WG_RC_INLINE RcMat<N, N> rc_eye() {
  RcMat<N, N> m = rc_zeros<N, N>();
#pragma unroll
  for (int i = 0; i < N; i++) m(i, i) = 1.0;
  return m;
}
// plain triple loop, k ascending (the order of ublas prod on dense matrices)
template <int R, int K, int C>
WG_RC_INLINE RcMat<R, C> rc_mul(const RcMat<R, K> &a, const RcMat<K, C> &b) {
  RcMat<R, C> o;
#pragma unroll
  for (int i = 0; i < R; i++)
#pragma unroll
    for (int j = 0; j < C; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < K; k++) s += a(i, k) * b(k, j);
      o(i, j) = s;
    }
  return o;
}
template <int R, int C>
WG_RC_INLINE RcMat<C, R> rc_tr(const RcMat<R, C> &a) {
  RcMat<C, R> o;
#pragma unroll
  for (int i = 0; i < R; i++)
#pragma unroll
    for (int j = 0; j < C; j++) o(j, i) = a(i, j);
  return o;
}
template <int R, int C>
WG_RC_INLINE RcMat<R, C> rc_add(const RcMat<R, C> &a, const RcMat<R, C> &b) {
  RcMat<R, C> o = a;
#pragma unroll
  for (int i = 0; i < R * C; i++) o.v[i] += b.v[i];
  return o;
}
template <int R, int C>
WG_RC_INLINE RcMat<R, C> rc_sub(const RcMat<R, C> &a, const RcMat<R, C> &b) {
  RcMat<R, C> o = a;
#pragma unroll
  for (int i = 0; i < R * C; i++) o.v[i] -= b.v[i];
  return o;
}
template <int R, int C>
WG_RC_INLINE RcMat<R, C> rc_scale(const RcMat<R, C> &a, double s) {
  RcMat<R, C> o = a;
#pragma unroll
  for (int i = 0; i < R * C; i++) o.v[i] *= s;
  return o;
}
// the largest magnitude; an entry that is not a number is passed over, as fmax does
template <int R, int C>
WG_RC_INLINE double rc_maxabs(const RcMat<R, C> &a) {
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < R * C; i++) {
    const double x = fabs(a.v[i]);
    if (x > m) m = x;
  }
  return m;
}

// X = W^-1 * B by Gaussian elimination with partial pivoting; false when W is numerically singular
template <int N, int C>
WG_RC_INLINE bool rc_solve(RcMat<N, N> W, RcMat<N, C> B, RcMat<N, C> &X) {
#pragma unroll
  for (int k = 0; k < N; k++) {
    int p = k;
    double best = fabs(W(k, k));
#pragma unroll
    for (int i = k + 1; i < N; i++)
      if (fabs(W(i, k)) > best) { best = fabs(W(i, k)); p = i; }
    if (!(best > 0.0)) return false;
#pragma unroll
    for (int i = k + 1; i < N; i++)
      if (i == p) {                                  // rows k and p change places
#pragma unroll
        for (int j = 0; j < N; j++) { const double t = W(k, j); W(k, j) = W(i, j); W(i, j) = t; }
#pragma unroll
        for (int j = 0; j < C; j++) { const double t = B(k, j); B(k, j) = B(i, j); B(i, j) = t; }
      }
#pragma unroll
    for (int i = k + 1; i < N; i++) {
      const double f = W(i, k) / W(k, k);
      if (f == 0.0) continue;
#pragma unroll
      for (int j = k; j < N; j++) W(i, j) -= f * W(k, j);
#pragma unroll
      for (int j = 0; j < C; j++) B(i, j) -= f * B(k, j);
    }
  }
#pragma unroll
  for (int j = 0; j < C; j++)
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
      double s = B(i, j);
#pragma unroll
      for (int k = i + 1; k < N; k++) s -= W(i, k) * X(k, j);
      X(i, j) = s / W(i, i);
    }
  return true;
}

// one application of the Riccati map  P -> A'PA - A'Pb (R + b'Pb)^-1 b'PA + H
template <int N>
WG_RC_INLINE RcMat<N, N> rc_riccati_map(const RcMat<N, N> &A, const RcMat<N, 1> &b, const RcMat<N, N> &H, double R,
                                        const RcMat<N, N> &P) {
  const RcMat<N, N> At = rc_tr(A);
  const RcMat<1, N> bt = rc_tr(b);
  const RcMat<N, N> PA = rc_mul(P, A);
  const RcMat<1, N> btPA = rc_mul(bt, PA);
  const double den = R + rc_mul(rc_mul(bt, P), b)(0, 0);
  const RcMat<N, N> out = rc_add(rc_mul(At, PA), H);
  const RcMat<N, N> corr = rc_scale(rc_mul(rc_tr(btPA), btPA), 1.0 / den);
  return rc_sub(out, corr);
}

// structure-preserving doubling:  A_{k+1} = A_k W^-1 A_k,  G_{k+1} = G_k + A_k W^-1 G_k A_k',
//                                 H_{k+1} = H_k + A_k' H_k W^-1 A_k,   W = I + G_k H_k;   H_k -> P
template <int N>
WG_RC_HD inline bool rc_dare(const RcMat<N, N> &A0, const RcMat<N, 1> &b, const RcMat<1, N> &c, double Q, double R,
                             RcMat<N, N> &P) {
  RcMat<N, N> A = A0;
  RcMat<N, N> G = rc_scale(rc_mul(b, rc_tr(b)), 1.0 / R);
  const RcMat<N, N> H0 = rc_mul(rc_scale(rc_tr(c), Q), c);
  RcMat<N, N> H = H0;
  bool converged = false;
  for (int it = 0; it < 60; it++) {
    const RcMat<N, N> W = rc_add(rc_eye<N>(), rc_mul(G, H));
    RcMat<N, N> WiA, WiG;
    if (!rc_solve(W, A, WiA) || !rc_solve(W, G, WiG)) return false;
    const RcMat<N, N> An = rc_mul(A, WiA);
    const RcMat<N, N> Gn = rc_add(G, rc_mul(rc_mul(A, WiG), rc_tr(A)));
    const RcMat<N, N> Hn = rc_add(H, rc_mul(rc_mul(rc_tr(A), H), WiA));
    const double dh = rc_maxabs(rc_sub(Hn, H)), hs = rc_maxabs(Hn);
    A = An; G = Gn; H = Hn;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < N * N; i++) finite = finite && rc_finite(H.v[i]);
    if (!finite) return false;
    if (dh <= 1e-15 * hs) { converged = true; break; }
  }
  if (!converged) return false;
  // symmetrise, then polish on the original equation
  P = rc_scale(rc_add(H, rc_tr(H)), 0.5);
  for (int k = 0; k < 2; k++) {
    const RcMat<N, N> Pn = rc_riccati_map(A0, b, H0, R, P);
    P = rc_scale(rc_add(Pn, rc_tr(Pn)), 0.5);
  }
  return true;
}

// wg_riccati_solve for order N.  K[i] goes to K[i * sK], F[k] to F[k * sF] (strides of 1 on the host, of the fleet in the
// kernel); nothing is stored unless the result is WG_OK.
template <int N>
WG_RC_HD inline int rc_solve_order(const double *A_rm, const double *b, const double *c, double Q, double R, int Nl, int mode,
                                   double *K, size_t sK, double *F, size_t sF) {
  if (!A_rm || !b || !c || !K || (Nl > 0 && !F) || Nl < 0 || !(R > 0.0)) return WG_ERR_BAD_ARG;
  RcMat<N, N> A;
  RcMat<N, 1> B;
  RcMat<1, N> C;
#pragma unroll
  for (int i = 0; i < N; i++) {
#pragma unroll
    for (int j = 0; j < N; j++) A(i, j) = A_rm[i * N + j];
    B(i, 0) = b[i];
    C(0, i) = c[i];
  }
  RcMat<N, N> P;
  if (!rc_dare(A, B, C, Q, R, P)) return WG_ERR_BAD_ARG;

  // OptimalControllerSolver.cpp:300-352
  const RcMat<1, N> tb = rc_tr(B);
  double la = R + rc_mul(rc_mul(tb, P), B)(0, 0);
  la = 1 / la;
  const RcMat<1, N> Km = rc_scale(rc_mul(tb, rc_mul(P, A)), la);     // K = la * b' (P A)
#pragma unroll
  for (int i = 0; i < N; i++) K[(size_t)i * sK] = Km(0, i);

  const RcMat<1, N> Pre = rc_scale(tb, la);
  const RcMat<N, N> Base = rc_tr(rc_sub(A, rc_mul(B, Km)));
  RcMat<N, 1> Post = rc_scale(rc_tr(C), Q);
  if (mode == WG_RICCATI_WITHOUT_INITIALPOS) Post = rc_mul(P, Post);
  RcMat<N, 1> Rec = Post;
  for (int k = 0; k < Nl; k++) {
    F[(size_t)k * sF] = rc_mul(Pre, Rec)(0, 0);
    Rec = rc_mul(Base, Rec);
  }
  return WG_OK;
}

// wg_riccati_gains: the cart table of sampling period T and CoM height zc, as the 3-state system (WITH_INITIALPOS) or the
// 4-state error system (WITHOUT_INITIALPOS); K[0..3] and F[0..Nl) with the strides of rc_solve_order
WG_RC_HD inline int rc_gains(double T, double zc, double Q, double R, int Nl, int mode, double *K, size_t sK, double *F,
                             size_t sF) {
  if (!(T > 0.0) || !K) return WG_ERR_BAD_ARG;
  // PreviewControl.cpp:203-214
  const double A3[9] = {1.0, T, T * T / 2.0, 0.0, 1.0, T, 0.0, 0.0, 1.0};
  const double B3[3] = {T * T * T / 6.0, T * T / 2.0, T};
  const double C3[3] = {1.0, 0.0, -zc / 9.81};
  if (mode == WG_RICCATI_WITH_INITIALPOS) {               // :297-315  (K[0] doubles as Ks there; K[3] unused)
    double K3[3];
    const int rc = rc_solve_order<3>(A3, B3, C3, Q, R, Nl, mode, K3, 1, F, sF);
    if (rc != WG_OK) return rc;
    K[0] = K3[0]; K[sK] = K3[1]; K[2 * sK] = K3[2]; K[3 * sK] = 0.0;
    return WG_OK;
  }
  if (mode != WG_RICCATI_WITHOUT_INITIALPOS) return WG_ERR_BAD_ARG;
  // :232-273  augmented ("derivated") system: state (accumulated ZMP error, dx)
  double Ax[16] = {0}, bx[4], cx[4] = {1.0, 0.0, 0.0, 0.0};
  double tmpA[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) s += C3[k] * A3[k * 3 + j];
    tmpA[j] = s;
  }
  Ax[0] = 1.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    Ax[0 * 4 + i + 1] = tmpA[i];
#pragma unroll
    for (int j = 0; j < 3; j++) Ax[(i + 1) * 4 + j + 1] = A3[i * 3 + j];
  }
  double tb = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) tb += C3[k] * B3[k];
  bx[0] = tb;
#pragma unroll
  for (int i = 0; i < 3; i++) bx[i + 1] = B3[i];
  return rc_solve_order<4>(Ax, bx, cx, Q, R, Nl, mode, K, sK, F, sF);   // K = [Ks, Kx0, Kx1, Kx2]
}

}  // namespace wg
