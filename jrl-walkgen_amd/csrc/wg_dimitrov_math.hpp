// wg_dimitrov_math.hpp -- the arithmetic of the Dimitrov-2008 constants, once, for the host calls (wg_dimitrov_configure,
// wg_dimitrov_constants: DimitrovHost::build in wg_dimitrov_device.hpp) and the kernel (wg_dimitrov_kernels.hpp:
// wg_dimitrov_constants_batch_dev).
//
//   InitConstants / InitializeMatrixPbConstants   src/ZMPRefTrajectoryGeneration/ZMPConstrainedQPFastFormulation.cpp:158-246
//   BuildingConstantPartOfTheObjectiveFunction*   :382-389, 384-467, 524-556   (OptA with its alpha VPu' quirk, OptB, OptC, LQ)
//   BuildingConstantPartOfConstraintMatrices      :597-690                     (Pu', m_Pu = iLQ Pu', its inverse)
//   OptCholesky::ComputeNormalCholeskyOnANormal / ComputeInverseCholeskyNormal   OptCholesky.cpp:225-302
//   PLDPSolver::PrecomputeiPuPx
//
// Plain C++ that a HIP translation unit compiles for both sides: WG_DM_HD is `__host__ __device__` there and nothing elsewhere,
// and nothing here names a kernel, a lane or a block index.  dm_build is a list of phases; a phase is a loop over independent
// outputs, `for (e = x.lane(); e < count; e += x.lanes())`, and x.sync() stands between a phase and the next one that reads
// what it wrote.  The host runs it with one lane and no fence (DmHostExec), the kernel with the 64 lanes of a wavefront and
// WG_WSYNC.  Every output element keeps the operation order of the reference whichever lane computes it -- sums with k ascending
// from 0.0 over the whole inner range (zero terms included: they decide the sign of a zero), the f == 0.0 skip of the
// elimination, 1 / L and then -d * r in the inverse -- and the library is built with -ffp-contract=off, / and sqrt are IEEE on
// both sides: host and kernel give the same bytes.  What every lane needs (a pivot, a diagonal entry of the factor) every lane
// computes from the work area, so every exit is uniform.
//
// The work matrices (DmWork: OptA 2N x 2N, the factor, its inverse, Pu', m_Pu and the two halves of the Gauss-Jordan tableau,
// N x N each) are LDS in the kernel, 22 KB at N = 16.  PPu, VPu, PPx, VPx are Toeplitz / closed forms: generated from two tables
// of N values, never stored.  Nothing is written to the model's block before the model is known to be good: a block has one
// writer per byte and a failed model none but the caller's zeros.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/wg_mpc.h"
#ifdef __HIP__
#define WG_DM_HD __host__ __device__
#else
#define WG_DM_HD
#endif
#define WG_DM_INLINE WG_DM_HD inline __attribute__((always_inline))

namespace wg {

constexpr int kDmN = WG_PLDP_N, kDm2N = 2 * WG_PLDP_N;

struct DmWork {
  double OptA[kDm2N * kDm2N];                       // leading dimension n = 2N
  double LQ[kDmN * kDmN], iLQ1[kDmN * kDmN];        // leading dimension N, like the four below
  double PuT[kDmN * kDmN], Pu[kDmN * kDmN], a[kDmN * kDmN], inv[kDmN * kDmN];
  double OptB[kDm2N * 6];                           // before the LQ step
  double Px[kDmN * 3];
  double p[kDmN], v[kDmN];                          // PPu(i, j) = p[i - j], VPu(i, j) = v[i - j] inside a diagonal block, j <= i
  double fcol[kDmN];                                // the pivot column of an elimination step
};

struct DmHostExec {
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() const {}
};

// a double is finite iff x - x == 0 (inf - inf and nan - nan are nan)
WG_DM_INLINE bool dm_finite(double x) { return x - x == 0.0; }

// entries of the 2N x 2N block-diagonal Toeplitz matrices and of the 2N x 6 state maps (:165-211)
WG_DM_INLINE double dm_toep(const double *tab, int r, int c, int N) {
  const bool lo = r < N;
  if (lo != (c < N)) return 0.0;
  const int d = (lo ? r : r - N) - (lo ? c : c - N);
  return d >= 0 ? tab[d] : 0.0;
}
WG_DM_INLINE double dm_ppx(int r, int j, int N, double T) {
  const bool lo = r < N;
  const unsigned i = (unsigned)(lo ? r : r - N);
  const int jj = lo ? j : j - 3;
  if (jj == 0) return 1.0;
  if (jj == 1) return (i + 1) * T;
  if (jj == 2) return (i + 1) * (i + 1) * T * T * 0.5;
  return 0.0;
}
WG_DM_INLINE double dm_vpx(int r, int j, int N, double T) {
  const bool lo = r < N;
  const unsigned i = (unsigned)(lo ? r : r - N);
  const int jj = lo ? j : j - 3;
  if (jj == 1) return 1.0;
  if (jj == 2) return (i + 1) * T;
  return 0.0;
}
// iLQ (2N x 2N): the inverse factor in both diagonal blocks (:448-461)
WG_DM_INLINE double dm_ilq(const DmWork &W, int i, int k, int N) {
  const bool lo = i < N;
  if (lo != (k < N)) return 0.0;
  return W.iLQ1[(lo ? i : i - N) * N + (lo ? k : k - N)];
}

// The constants of model m into K (a DimitrovConst).  false, with nothing of K written, when a height or weight is not finite or
// the LQ factor or the inverse of Pu does not exist.  Bytes of K behind the arrays' used parts are zeroed; the caller owns what
// lies behind K.
template <class X, class KT>
WG_DM_HD inline bool dm_build(const X x, const wg_dimitrov_model_t &m, DmWork &W, KT &K) {
  const int N = m.N, n = 2 * N;
  const double T = m.T, alpha = m.alpha, beta = m.beta, h = m.com_height;
  const int l0 = x.lane(), S = x.lanes();
  if (!dm_finite(T) || !dm_finite(h) || !dm_finite(alpha) || !dm_finite(beta)) return false;

  // ---- the generators of PPu / VPu, Px (:165-220), a clean inverse factor ----
  for (int d = l0; d < N; d += S) {
    const unsigned u = (unsigned)d;
    W.v[d] = (2 * u + 1) * T * T * 0.5;
    W.p[d] = (1 + 3 * u + 3 * u * u) * T * T * T / 6.0;
    W.Px[d * 3 + 0] = 1.0;
    W.Px[d * 3 + 1] = (double)(1.0 + u) * T;
    W.Px[d * 3 + 2] = (u + 1.0) * (u + 1.0) * T * T * 0.5 - h / 9.81;
  }
  for (int e = l0; e < N * N; e += S) W.iLQ1[e] = 0.0;
  x.sync();

  // ---- OptA = Id + beta PPu'PPu + alpha VPu'   (the reference scales VPu', not VPu'VPu: :524-527) ----
  for (int e = l0; e < n * n; e += S) {
    const int i = e / n, j = e - i * n;
    double s = 0.0;
    for (int k = 0; k < n; k++) s += dm_toep(W.p, k, i, N) * dm_toep(W.p, k, j, N);
    W.OptA[e] = ((i == j ? 1.0 : 0.0) + beta * s) + alpha * dm_toep(W.v, j, i, N);
  }
  // ---- linear part: OptB = alpha VPu'VPx + beta PPu'PPx   (:545-556) ----
  for (int e = l0; e < n * 6; e += S) {
    const int i = e / 6, j = e - i * 6;
    double l1 = 0.0, ob = 0.0;
    for (int k = 0; k < n; k++) l1 += dm_toep(W.p, k, i, N) * dm_ppx(k, j, N, T);
    for (int k = 0; k < n; k++) ob += dm_toep(W.v, k, i, N) * dm_vpx(k, j, N, T);
    W.OptB[e] = alpha * ob + beta * l1;
  }
  x.sync();

  // ---- LQ factor of the leading N x N block: only the lower triangle of OptA is read (:384-420).  Column by column: the
  // diagonal entry by every lane, the entries below it one per lane ----
  for (int lj = 0; lj < N; lj++) {
    double r = W.OptA[lj * n + lj];
    for (int lk = 0; lk < lj; lk++) r = r - W.LQ[lj * N + lk] * W.LQ[lj * N + lk];
    if (!(r > 0.0)) return false;
    const double dd = sqrt(r);
    if (l0 == 0) W.LQ[lj * N + lj] = dd;
    for (int li = lj + 1 + l0; li < N; li += S) {
      double q = W.OptA[li * n + lj];
      for (int lk = 0; lk < lj; lk++) q = q - W.LQ[li * N + lk] * W.LQ[lj * N + lk];
      W.LQ[li * N + lj] = q / dd;
    }
    x.sync();
  }
  // ---- its inverse: a row reads the factor and its own entries to the right, so a row per lane ----
  for (int li = l0; li < N; li += S)
    for (int lj = li; lj >= 0; lj--) {
      const double d = 1 / W.LQ[lj * N + lj];
      if (lj == li) W.iLQ1[li * N + lj] = d;
      else {
        double r = 0.0;
        for (int lk = lj + 1; lk < N; lk++) r = r + W.iLQ1[li * N + lk] * W.LQ[lk * N + lj];
        W.iLQ1[li * N + lj] = -d * r;
      }
    }
  // ---- constraint side: Pu' (transposed storage, :629-637) ----
  for (int e = l0; e < N * N; e += S) {
    const int k = e / N, i = e - k * N;
    W.PuT[e] = k <= i ? (W.p[i - k] - T * h / 9.81) : 0.0;
  }
  x.sync();
  // ---- m_Pu = iLQ Pu', the tableau [m_Pu | I] ----
  for (int e = l0; e < N * N; e += S) {
    const int i = e / N, j = e - i * N;
    double s = 0;
    for (int k = 0; k < N; k++) s += W.iLQ1[i * N + k] * W.PuT[k * N + j];
    W.Pu[e] = s;
    W.a[e] = s;
    W.inv[e] = i == j ? 1.0 : 0.0;
  }
  x.sync();
  // ---- MAL_INVERSE (jrl-mal -> LAPACK, unpinned): Gauss-Jordan with partial pivoting, the first of equal maxima ----
  for (int c = 0; c < N; c++) {
    int p = c;
    double best = fabs(W.a[c * N + c]);
    for (int r = c + 1; r < N; r++)
      if (fabs(W.a[r * N + c]) > best) { best = fabs(W.a[r * N + c]); p = r; }
    if (!(best > 0.0)) return false;
    if (p != c) {
      for (int j = l0; j < N; j += S) {
        const double ta = W.a[c * N + j], ti = W.inv[c * N + j];
        W.a[c * N + j] = W.a[p * N + j]; W.a[p * N + j] = ta;
        W.inv[c * N + j] = W.inv[p * N + j]; W.inv[p * N + j] = ti;
      }
      x.sync();
    }
    const double d = W.a[c * N + c];
    x.sync();
    for (int j = l0; j < N; j += S) { W.a[c * N + j] /= d; W.inv[c * N + j] /= d; }
    for (int r = l0; r < N; r += S)
      if (r != c) W.fcol[r] = W.a[r * N + c];
    x.sync();
    for (int e = l0; e < N * N; e += S) {
      const int r = e / N, j = e - r * N;
      if (r == c) continue;
      const double f = W.fcol[r];
      if (f == 0.0) continue;
      W.a[e] -= f * W.a[c * N + j];
      W.inv[e] -= f * W.inv[c * N + j];
    }
    x.sync();
  }

  // ---- the block: every element of every array once, zero behind the used part ----
  if (l0 == 0) {
    K.N = N; K.solver = m.solver; K.T = T; K.Tctrl = m.Tctrl; K.h = h;
    K.pldp.N = N; K.pldp.pad_ = 0;
  }
  for (int e = l0; e < kDm2N * kDm2N; e += S) {
    double ilq = 0.0, oc = 0.0, qq = 0.0, ocq = 0.0;
    if (e < n * n) {
      const int i = e / n, j = e - i * n;
      ilq = dm_ilq(W, i, j, N);
      for (int k = 0; k < n; k++) oc += dm_ilq(W, i, k, N) * (beta * dm_toep(W.p, j, k, N));   // iLQ OptC, OptC = beta PPu'  (:464-467)
      qq = W.OptA[j * n + i];                       // m_Q[i 2N + j] = OptA(j, i): ql0001_'s column-major layout (:382-389)
      ocq = beta * dm_toep(W.p, j, i, N);
    }
    K.iLQ[e] = ilq; K.OptC[e] = oc; K.Qq[e] = qq; K.OptCq[e] = ocq;
  }
  for (int e = l0; e < kDm2N * 6; e += S) {
    double ob = 0.0, obq = 0.0, ip = 0.0;
    if (e < n * 6) {
      const int i = e / 6, j = e - i * 6;
      for (int k = 0; k < n; k++) ob += dm_ilq(W, i, k, N) * W.OptB[k * 6 + j];                  // iLQ OptB
      obq = W.OptB[e];
      if ((i < N) == (j < 3)) {                     // PLDPSolver::PrecomputeiPuPx: the same N x 3 block for x and for y
        const int ii = i < N ? i : i - N, jj = j < 3 ? j : j - 3;
        double s = 0.0;
        for (int k = 0; k < N; k++) s += W.inv[k * N + ii] * W.Px[k * 3 + jj];
        ip = s;
      }
    }
    K.OptB[e] = ob; K.OptBq[e] = obq; K.pldp.iPuPx[e] = ip;
  }
  for (int e = l0; e < kDmN * kDmN; e += S) {
    const bool in = e < N * N;
    K.pldp.iPu[e] = in ? W.inv[e] : 0.0;
    K.pldp.Pu[e] = in ? W.Pu[e] : 0.0;
    K.PuTq[e] = in ? W.PuT[e] : 0.0;
  }
  for (int e = l0; e < kDmN * 3; e += S) K.pldp.Px[e] = e < N * 3 ? W.Px[e] : 0.0;
  return true;
}

}  // namespace wg
