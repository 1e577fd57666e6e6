// wg_dimitrov_kernels.hpp -- the __global__ kernels of the Dimitrov-2008 tick (wg_dimitrov_tick_batch*): around PLDP, and around
// the in-wave ql0002.  Included by wg_capi.hip, which launches them; the ticks themselves are wg_dimitrov_device.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wg_mpc.h"
#include "wg_dimitrov_device.hpp"

// ---- Dimitrov-2008 tick around PLDP ------------------------------------------------------------------------------------

__global__ void __launch_bounds__(64)
wg_dimitrov_tick_kernel(int B, const wg::DimitrovConst *__restrict__ K, const wg_zmp_polytope_t *__restrict__ polys,
                        wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dim_lds[];
  const int N = K->N;
  const int g = blockIdx.x;                       // one gait per block (grid == B), like the Herdt tick
  // (a longest-solve-first start order as in the QL back-ends below was measured here and gave nothing: 5.19 against 5.20 M
  // ticks/s -- PLDP's four iterations per tick leave nothing to order)
  if (g < B) (void)wg::dimitrov_tick(*K, dim_lds, polys + (size_t)g * N, states + g, outs ? outs + g : nullptr, max_iter);
}

// modes QLD / QLDANDLQ: the same tick with the in-wave ql0002 as its back-end (wg_dimitrov_device.hpp, dimitrov_qld_tick)
template <bool kLQ>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
wg_dimitrov_qld_tick_kernel(int B, const wg::DimitrovConst *__restrict__ K, const wg_zmp_polytope_t *__restrict__ polys,
                            wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, const int *__restrict__ order,
                            int *__restrict__ iters_out) {
  extern __shared__ __attribute__((aligned(16))) double dimq_lds[];
  const int N = K->N;
  const int g = order ? wg::uni(order[blockIdx.x]) : (int)blockIdx.x;     // longest-solve-first by the previous tick (scheduling only)
  if (g < B) {
    const int it = wg::dimitrov_qld_tick<kLQ>(*K, dimq_lds, polys + (size_t)g * N, states + g, outs ? outs + g : nullptr);
    if (iters_out && (threadIdx.x & 63) == 0) iters_out[g] = it;
  }
}

// ---- the ticks of wg_dimitrov_follow_dev: the same ticks, for the gaits wg_dimitrov_follow_select_kernel let go ---------------
// row[g] is the row of outs ([tick_cap][B], absolute) gait g's tick writes, or -1: the gait sits this round out and its block
// returns at once -- its state, its outs and, in the QL modes, its iteration count of the previous tick stay as they are.

__global__ void __launch_bounds__(64)
wg_dimitrov_follow_tick_kernel(int B, const wg::DimitrovConst *__restrict__ K, const wg_zmp_polytope_t *__restrict__ polys,
                               wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, const int *__restrict__ row, int max_iter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dim_lds[];
  const int N = K->N;
  const int g = blockIdx.x;
  if (g >= B) return;
  const int r = wg::uni(row[g]);
  if (r < 0) return;
  (void)wg::dimitrov_tick(*K, dim_lds, polys + (size_t)g * N, states + g, outs ? outs + (size_t)r * (size_t)B + g : nullptr, max_iter);
}

template <bool kLQ>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
wg_dimitrov_qld_follow_tick_kernel(int B, const wg::DimitrovConst *__restrict__ K, const wg_zmp_polytope_t *__restrict__ polys,
                                   wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, const int *__restrict__ row,
                                   const int *__restrict__ order, int *__restrict__ iters_out) {
  extern __shared__ __attribute__((aligned(16))) double dimq_lds[];
  const int N = K->N;
  const int g = order ? wg::uni(order[blockIdx.x]) : (int)blockIdx.x;     // longest-solve-first by the gait's last tick (scheduling only)
  if (g >= B) return;
  const int r = wg::uni(row[g]);
  if (r < 0) return;
  const int it = wg::dimitrov_qld_tick<kLQ>(*K, dimq_lds, polys + (size_t)g * N, states + g, outs ? outs + (size_t)r * (size_t)B + g : nullptr);
  if (iters_out && (threadIdx.x & 63) == 0) iters_out[g] = it;
}
