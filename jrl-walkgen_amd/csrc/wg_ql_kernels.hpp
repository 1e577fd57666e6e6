// wg_ql_kernels.hpp -- the __global__ kernel of the dense ql0001_ boundary (wg_qp_solve_batch*).  Included by wg_capi.hip,
// which launches it; the solver itself is wg_ql_device.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/wg_mpc.h"
#include "wg_ql_device.hpp"

// ---------------------------------------------------------------------------
// Dense batched QP kernel: one wavefront (= one workgroup) per QP.
// Replaces ql0001_ (qld.hh:27-31) for B problems at once.
// ---------------------------------------------------------------------------
// kFixN / kFixM > 0: the Herdt-sized boundary (nmax == kFixN, mmax == kFixM, A, G and wa | b out of the LDS) with the strides, the
// LDS layout and the solver's loop bounds as compile-time constants (QlView::carve_fixed_dense, DenseProbT<false, kFixN>)
template <bool kALds, bool kGLds, bool kWLds = true, int kFixN = 0, int kFixM = 0>   // where A / G / wa | b live is known at compile time: ds_ or global_ accesses,
// Left to itself the compiler takes 256 VGPRs plus 3 AGPRs -- 259 registers, one wave per SIMD, four QPs per CU where the LDS
// would admit five at n = 36, m = 75.  Forced to two waves per SIMD (-DWG_QLD_WPE=2: 256 registers, 2-3 spilled, 12-16 B of
// scratch) it measured 5 % SLOWER on the Herdt workload's real QPs (1.73 against 1.82 M QPs/s, B = 4096): the fifth QP per CU
// does not pay for the tighter allocation.  The default stays.
// With G read in place as well (21.7 KB of LDS at n = 36, m = 75: seven QPs per CU) the residency is worth the 256-register
// build: that instantiation is compiled for two waves per SIMD.
#ifdef WG_QLD_WPE
#define WG_QLD_ATTR __attribute__((amdgpu_waves_per_eu(WG_QLD_WPE, WG_QLD_WPE)))
#else
#define WG_QLD_ATTR __attribute__((amdgpu_waves_per_eu(kGLds ? 1 : 2, kGLds ? 8 : 2)))
#endif
__global__ __launch_bounds__(64) WG_QLD_ATTR void wg_ql_dense_kernel(   // never flat_ (those also count on lgkmcnt and stall the LDS waits)
    int B, int nmax_arg, int mmax_arg, const int *__restrict__ n_arr, const int *__restrict__ m_arr,
    const int *__restrict__ me_arr, const double *__restrict__ C, const double *__restrict__ dvec,
    const double *__restrict__ A, const double *__restrict__ bvec, const double *__restrict__ xl,
    const double *__restrict__ xu, double eps, double *__restrict__ x, double *__restrict__ u,
    int *__restrict__ ifail, int *__restrict__ n_iter, int *__restrict__ iact, int *__restrict__ nact,
    int *__restrict__ hist, int hist_cap, int *__restrict__ hist_len, double *__restrict__ wab_slots,
    const int *__restrict__ order, int *__restrict__ iters_out) {
  extern __shared__ __attribute__((aligned(16))) double wg_lds[];
  const int lane = threadIdx.x & 63;
  // one QP per block (grid == B): nothing lane-dependent lives across QPs.  Blocks start in index order: `order`
  // (wg_lpt_order_kernel) makes that the order of decreasing solve length, as far as the previous batch predicts it
  const int qp = order ? wg::uni(order[blockIdx.x]) : (int)blockIdx.x;
  const int nmax = kFixN > 0 ? kFixN : nmax_arg, mmax = kFixM > 0 ? kFixM : mmax_arg;   // the host checks the match
  if (qp < B) {
    const int n = n_arr ? n_arr[qp] : nmax;
    const int m = m_arr ? m_arr[qp] : mmax - 1;
    const int me = me_arr ? me_arr[qp] : 0;
    wg::QlDims D(n, m, m, true, kALds, 0, true, true, kWLds, true, 0, kGLds);
    wg::QlView q;
    // kWLds = false: the constraint weights wa (m + n) and b (m) -- read lane-parallel once per iteration -- live in this
    // block's slot of global memory [wa (mmax + nmax) | b (mmax)]: 1.5 KB less LDS, the eighth QP on the CU at n = 36, m = 75
    if constexpr (kFixN > 0) q.template carve_fixed_dense<kFixN, kFixM>(wg_lds, n, m, me, wab_slots + (size_t)qp * (2 * kFixM + kFixN));
    else if constexpr (kWLds) q.carve(wg_lds, D, me);
    else q.template carve<true, false, true>(wg_lds, D, me, wab_slots + (size_t)qp * (2 * (size_t)mmax + nmax), mmax + nmax);

    // ---- stage the problem into LDS (coalesced 8-byte lanes) ----
    const double *Cg = C + (size_t)qp * nmax * nmax;
    const double *Ag = A + (size_t)qp * mmax * nmax;
    if constexpr (kGLds) {
      for (int j = 0; j < n; ++j)
        for (int i = lane; i < n; i += 64) q.G[i + j * q.ldg] = Cg[i + (size_t)j * nmax];
    } else {                                   // G is cold after the factorisation: in place (L2), its diagonal in LDS
      q.G = const_cast<double *>(Cg);
      q.ldg = nmax;
      for (int i = lane; i < n; i += 64) q.Gdiag[i] = Cg[i + (size_t)i * nmax];
    }
    if constexpr (kALds) {
      for (int i = 0; i < n; ++i)
        for (int k = lane; k < m; k += 64) q.A[k + i * q.lda] = Ag[k + (size_t)i * mmax];
    } else {                                   // too large for LDS next to G, Z, R: the solver only reads A -> in place (L2)
      q.A = const_cast<double *>(Ag);
      q.lda = mmax;
    }
    for (int i = lane; i < n; i += 64) {
      q.d[i] = dvec[(size_t)qp * nmax + i];
      q.xl[i] = xl[(size_t)qp * nmax + i];
      q.xu[i] = xu[(size_t)qp * nmax + i];
    }
    for (int k = lane; k < m; k += 64) q.b[k] = -bvec[(size_t)qp * mmax + k];   // qld.cpp:469-475
    WG_WSYNC();
    // qld.cpp:442-444: c(nmax,nmax) == 0 -> eps (inside the n x n block only if nmax == n)
    typename std::conditional<(kFixN > 0), wg::DenseRegProb<(kFixN > 0 ? kFixN : 1), (kFixM > 0 ? kFixM : 1)>, wg::DenseProbT<kGLds, kFixN>>::type prob;
    // (kFixN > 0: A's rows go into registers inside ql_solve, once R and Z exist -- m <= kFixM <= 128: two rows per lane)
    if (nmax == n && lane == 0 && fabs(prob.Gd(q, n - 1)) == 0.0) prob.setGd(q, n - 1, eps);
    WG_WSYNC();

    int *hq = hist ? hist + (size_t)qp * hist_cap : nullptr;
    wg::QlResult r = wg::ql_solve(q, prob, eps, hq, hist_cap);

    // ---- results ----
    for (int i = lane; i < n; i += 64) x[(size_t)qp * nmax + i] = q.x[i];
    if (u) {
      double *uq = u + (size_t)qp * (mmax + 2 * nmax);
      if (r.ifail == 0) {                                   // qld.cpp:520-536
        for (int j = lane; j < m + 2 * n; j += 64) uq[j] = 0.0;
        WG_WSYNC();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        for (int i = lane; i < r.nact; i += 64) uq[q.iact[i] - 1] = q.lam[i];
      }
    }
    if (iact)
      for (int i = lane; i < nmax; i += 64) iact[(size_t)qp * nmax + i] = (i < r.nact) ? q.iact[i] : 0;
    if (lane == 0) {
      ifail[qp] = r.ifail;
      if (n_iter) n_iter[qp] = r.n_iter;
      if (nact) nact[qp] = r.nact;
      if (hist_len) hist_len[qp] = r.hist_len;
      if (iters_out) iters_out[qp] = r.n_iter;
    }
    WG_WSYNC();
  }
}
