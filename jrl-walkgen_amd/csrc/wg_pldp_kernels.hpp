// wg_pldp_kernels.hpp -- the __global__ kernel of the PLDP / OptCholesky back-end (wg_pldp_solve_batch*).  Included by
// wg_capi.hip, which launches it; the solver itself is wg_pldp_device.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wg_mpc.h"
#include "wg_pldp_device.hpp"

// ---- PLDP / OptCholesky back-end -----------------------------------------------------------------------------------

template <bool kALds>                                      // A's place known at compile time (see wg_ql_dense_kernel)
__global__ void __launch_bounds__(64)
wg_pldp_kernel(int B, int mcap, const wg::PldpModel *__restrict__ model, const int *__restrict__ m,
               const double *__restrict__ D, const double *__restrict__ A, const double *__restrict__ b,
               const double *__restrict__ zmpref, const double *__restrict__ xkyk, const int *__restrict__ similar,
               const int *__restrict__ n_removed, const int *__restrict__ starting, int max_iter,
               wg_pldp_state_t *states, double *X, int *ret, int *n_iter, int *active, int *n_active) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pldp_lds[];
  const wg::PldpModel &M = *model;
  const int n = 2 * M.N;
  const size_t aslot = (size_t)(mcap + 1) * n;
  const int p = blockIdx.x;                        // one problem per block (grid == B)
  if (p < B) {
    int mp = m[p];
    if (mp < 0 || mp > mcap) {                      // refuse rather than index out of the slot
      if (threadIdx.x == 0) { ret[p] = WG_PLDP_BAD_INPUT; if (n_iter) n_iter[p] = 0; if (n_active) n_active[p] = 0; }
      return;
    }
    wg::pldp_problem<kALds>(M, pldp_lds, mcap, mp, D + (size_t)p * n, A + p * aslot, b + (size_t)p * mcap,
                     zmpref + (size_t)p * n, xkyk + (size_t)p * 6, similar + (size_t)p * mcap, n_removed[p], starting[p],
                     max_iter, states + p, X + (size_t)p * n, ret + p, n_iter ? n_iter + p : nullptr,
                     active ? active + (size_t)p * mcap : nullptr, n_active ? n_active + p : nullptr);
  }
}
