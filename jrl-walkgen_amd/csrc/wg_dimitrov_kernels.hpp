// wg_dimitrov_kernels.hpp -- the __global__ kernels of the Dimitrov-2008 tick (wg_dimitrov_tick_batch*): around PLDP, and around
// the in-wave ql0002.  Included by wg_capi.hip, which launches them; the ticks themselves are wg_dimitrov_device.hpp.
// Behind them the kernels of fleets with a model per gait: wg_dimitrov_constants_kernel (the constants of M models, the text of
// wg_dimitrov_math.hpp run by a wavefront per model) and the fleet twins of the four ticks.
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

// ---- a model per gait: the constants on the device, and the fleet twins of the four ticks ---------------------------------------

// the text of wg_dimitrov_math.hpp run by the 64 lanes of one wavefront
struct DmWaveExec {
  __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
  __device__ __forceinline__ int lanes() const { return 64; }
  __device__ __forceinline__ void sync() const { WG_WSYNC(); }
};

// wg_dimitrov_constants_batch_dev: one wave per model, kDimConstWaves models per block, each with its own work area in LDS.
// `base` gives N, solver, T, Tctrl and the value of every per-model array that is NULL.  Block m is written by wave m alone,
// every byte once: the constants and zeros behind them, or zeros throughout when the model fails; status[m] says which.
constexpr int kDimConstWaves = 2;
__global__ void __launch_bounds__(64 * kDimConstWaves)
wg_dimitrov_constants_kernel(int M, wg_dimitrov_model_t base, const double *__restrict__ com_height, const double *__restrict__ alpha,
                             const double *__restrict__ beta, unsigned char *__restrict__ blocks, int *__restrict__ status) {
  __shared__ wg::DmWork dm_work[kDimConstWaves];
  const int w = wg::uni((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int m = blockIdx.x * kDimConstWaves + w;
  if (m >= M) return;
  wg_dimitrov_model_t model = base;
  if (com_height) model.com_height = com_height[m];
  if (alpha) model.alpha = alpha[m];
  if (beta) model.beta = beta[m];
  unsigned char *blk = blocks + (size_t)m * wg::kDimitrovBlockBytes;
  const bool ok = wg::dm_build(DmWaveExec{}, model, dm_work[w], *reinterpret_cast<wg::DimitrovConst *>(blk));
  static_assert(sizeof(wg::DimitrovConst) % 8 == 0 && wg::kDimitrovBlockBytes % 8 == 0, "blocks are zeroed in 8-byte words");
  unsigned long long *words = reinterpret_cast<unsigned long long *>(blk);
  for (size_t e = (ok ? sizeof(wg::DimitrovConst) / 8 : 0) + lane; e < wg::kDimitrovBlockBytes / 8; e += 64) words[e] = 0ull;
  if (lane == 0) status[m] = ok ? WG_OK : WG_ERR_BAD_ARG;
}

// Gait g of a fleet launch runs with blocks[model_of[g]].  nullptr: the gait is refused -- model_of[g] outside [0, M), or a failed
// (all-zero) block, which a good one is told from by its N >= 1.
__device__ __forceinline__ const wg::DimitrovConst *wg_dimitrov_fleet_block(const unsigned char *__restrict__ blocks,
                                                                            const int *__restrict__ model_of, int M, int g) {
  const int mi = wg::uni(model_of[g]);
  if (mi < 0 || mi >= M) return nullptr;
  const wg::DimitrovConst *K = reinterpret_cast<const wg::DimitrovConst *>(blocks + (size_t)mi * wg::kDimitrovBlockBytes);
  return wg::uni(K->N) >= 1 ? K : nullptr;
}
// what a refused gait leaves: its return code and no iteration, in its out struct; of its state no byte is touched
__device__ __forceinline__ void wg_dimitrov_fleet_refuse(wg_dimitrov_out_t *out) {
  if (out && (threadIdx.x & 63) == 0) { out->ret = WG_PLDP_BAD_INPUT; out->n_iter = 0; }
}

__global__ void __launch_bounds__(64)
wg_dimitrov_fleet_tick_kernel(int B, int N, int M, const unsigned char *__restrict__ blocks, const int *__restrict__ model_of,
                              const wg_zmp_polytope_t *__restrict__ polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs,
                              int max_iter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dim_lds[];
  const int g = blockIdx.x;
  if (g >= B) return;
  wg_dimitrov_out_t *out = outs ? outs + g : nullptr;
  const wg::DimitrovConst *K = wg_dimitrov_fleet_block(blocks, model_of, M, g);
  if (!K || K->N != N) { wg_dimitrov_fleet_refuse(out); return; }
  (void)wg::dimitrov_tick(*K, dim_lds, polys + (size_t)g * N, states + g, out, max_iter);
}

template <bool kLQ>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
wg_dimitrov_qld_fleet_tick_kernel(int B, int N, int M, const unsigned char *__restrict__ blocks, const int *__restrict__ model_of,
                                  const wg_zmp_polytope_t *__restrict__ polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs,
                                  const int *__restrict__ order, int *__restrict__ iters_out) {
  extern __shared__ __attribute__((aligned(16))) double dimq_lds[];
  const int g = order ? wg::uni(order[blockIdx.x]) : (int)blockIdx.x;
  if (g >= B) return;
  wg_dimitrov_out_t *out = outs ? outs + g : nullptr;
  const wg::DimitrovConst *K = wg_dimitrov_fleet_block(blocks, model_of, M, g);
  int it = 0;
  if (!K || K->N != N) wg_dimitrov_fleet_refuse(out);
  else it = wg::dimitrov_qld_tick<kLQ>(*K, dimq_lds, polys + (size_t)g * N, states + g, out);
  if (iters_out && (threadIdx.x & 63) == 0) iters_out[g] = it;
}

__global__ void __launch_bounds__(64)
wg_dimitrov_fleet_follow_tick_kernel(int B, int N, int M, const unsigned char *__restrict__ blocks, const int *__restrict__ model_of,
                                     const wg_zmp_polytope_t *__restrict__ polys, wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs,
                                     const int *__restrict__ row, int max_iter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dim_lds[];
  const int g = blockIdx.x;
  if (g >= B) return;
  const int r = wg::uni(row[g]);
  if (r < 0) return;
  wg_dimitrov_out_t *out = outs ? outs + (size_t)r * (size_t)B + g : nullptr;
  const wg::DimitrovConst *K = wg_dimitrov_fleet_block(blocks, model_of, M, g);
  if (!K || K->N != N) { wg_dimitrov_fleet_refuse(out); return; }
  (void)wg::dimitrov_tick(*K, dim_lds, polys + (size_t)g * N, states + g, out, max_iter);
}

template <bool kLQ>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
wg_dimitrov_qld_fleet_follow_tick_kernel(int B, int N, int M, const unsigned char *__restrict__ blocks, const int *__restrict__ model_of,
                                         const wg_zmp_polytope_t *__restrict__ polys, wg_dimitrov_state_t *states,
                                         wg_dimitrov_out_t *outs, const int *__restrict__ row, const int *__restrict__ order,
                                         int *__restrict__ iters_out) {
  extern __shared__ __attribute__((aligned(16))) double dimq_lds[];
  const int g = order ? wg::uni(order[blockIdx.x]) : (int)blockIdx.x;
  if (g >= B) return;
  const int r = wg::uni(row[g]);
  if (r < 0) return;
  wg_dimitrov_out_t *out = outs ? outs + (size_t)r * (size_t)B + g : nullptr;
  const wg::DimitrovConst *K = wg_dimitrov_fleet_block(blocks, model_of, M, g);
  int it = 0;
  if (!K || K->N != N) wg_dimitrov_fleet_refuse(out);
  else it = wg::dimitrov_qld_tick<kLQ>(*K, dimq_lds, polys + (size_t)g * N, states + g, out);
  if (iters_out && (threadIdx.x & 63) == 0) iters_out[g] = it;
}
