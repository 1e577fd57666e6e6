// wg_dimitrov_kernels.hpp -- the __global__ kernels of the Dimitrov-2008 tick (wg_dimitrov_tick_batch*): around PLDP, and around
// the in-wave ql0002.  Included by wg_capi.hip, which launches them; the ticks themselves are wg_dimitrov_device.hpp.
// Each tick is one kernel template over two bindings -- which model a gait runs with, which row of outs it writes -- whose
// instantiations are the follow, fleet and fleet-follow forms; the plain form, the one that is timed, stands beside it.  Ahead of them wg_dimitrov_constants_kernel: the constants of the M models
// of a fleet (the text of wg_dimitrov_math.hpp run by a wavefront per model), the blocks the fleet binding reads.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/wg_mpc.h"
#include "wg_dimitrov_device.hpp"

// ---- a model per gait: the constants on the device -----------------------------------------------------------------------------

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

// ---- the two bindings of a tick launch -----------------------------------------------------------------------------------------

// Model binding, the launch's one model (wg_dimitrov_tick_batch_dev, _walk_dev, _follow_dev): every gait runs with *K, none is refused.
struct DimOneModel {
  const wg::DimitrovConst *K;
  static constexpr bool kRefuses = false;
  __device__ __forceinline__ int N() const { return K->N; }
  __device__ __forceinline__ const wg::DimitrovConst *bind(int) const { return K; }
};
// Model binding, a model per gait (the wg_dimitrov_*_fleet_dev calls): gait g runs with blocks[model_of[g]].  nullptr: the gait is
// refused -- model_of[g] outside [0, M), a failed (all-zero) block, which a good one is told from by its N >= 1, or a block of
// another horizon than the launch's N.
struct DimFleetModels {
  int n, M;
  const unsigned char *__restrict__ blocks;
  const int *__restrict__ model_of;
  static constexpr bool kRefuses = true;
  __device__ __forceinline__ int N() const { return n; }
  __device__ __forceinline__ const wg::DimitrovConst *bind(int g) const {
    const int mi = wg::uni(model_of[g]);
    if (mi < 0 || mi >= M) return nullptr;
    const wg::DimitrovConst *K = reinterpret_cast<const wg::DimitrovConst *>(blocks + (size_t)mi * wg::kDimitrovBlockBytes);
    return wg::uni(K->N) >= 1 && K->N == n ? K : nullptr;
  }
};
// what a refused gait leaves: its return code and no iteration, in its out struct; of its state no byte is touched
__device__ __forceinline__ void wg_dimitrov_refuse(wg_dimitrov_out_t *out) {
  if (out && (threadIdx.x & 63) == 0) { out->ret = WG_PLDP_BAD_INPUT; out->n_iter = 0; }
}

// Row binding.  out(): false when the gait sits the launch out, else *out is the struct its tick writes (nullptr without outs).
// Row g of outs [B]:
struct DimOwnRow {
  __device__ __forceinline__ bool out(wg_dimitrov_out_t *outs, int, int g, wg_dimitrov_out_t **out) const {
    *out = outs ? outs + g : nullptr;
    return true;
  }
};
// The ticks of wg_dimitrov_follow_dev, for the gaits wg_dimitrov_follow_select_kernel let go: row[g] is the row of outs
// ([tick_cap][B], absolute) gait g's tick writes, or -1: the gait sits this round out and its block returns at once -- its state,
// its outs and, in the QL modes, its iteration count of the previous tick stay as they are.
struct DimFollowRow {
  const int *__restrict__ row;
  __device__ __forceinline__ bool out(wg_dimitrov_out_t *outs, int B, int g, wg_dimitrov_out_t **out) const {
    const int r = wg::uni(row[g]);
    if (r < 0) return false;
    *out = outs ? outs + (size_t)r * (size_t)B + g : nullptr;
    return true;
  }
};

// ---- Dimitrov-2008 tick around PLDP ------------------------------------------------------------------------------------

// The follow, fleet and fleet-follow forms: one gait per block (grid == B), like the Herdt tick.
// (a longest-solve-first start order as in the QL back-ends below was measured here and gave nothing: 5.19 against 5.20 M
// ticks/s -- PLDP's four iterations per tick leave nothing to order)
template <class Model, class Row>
__global__ void __launch_bounds__(64)
wg_dimitrov_tick_form_kernel(int B, Model Mo, const wg_zmp_polytope_t *__restrict__ polys, wg_dimitrov_state_t *states,
                             wg_dimitrov_out_t *outs, Row Ro, int max_iter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dim_lds[];
  const int N = Mo.N();
  const int g = blockIdx.x;
  if (g >= B) return;
  wg_dimitrov_out_t *out = nullptr;
  if (!Ro.out(outs, B, g, &out)) return;
  const wg::DimitrovConst *K = Mo.bind(g);
  if (Model::kRefuses && !K) { wg_dimitrov_refuse(out); return; }
  (void)wg::dimitrov_tick(*K, dim_lds, polys + (size_t)g * N, states + g, out, max_iter);
}
// The plain form -- <DimOneModel, DimOwnRow>, which binds nothing and refuses nobody -- is timed by this name and these arguments,
// and keeps its text: ANY function between the kernel and wg::dimitrov_tick, a shared body included, makes the compiler order its
// first passes differently and changes a handful of the kernel's 2 541 instructions.
__global__ void __launch_bounds__(64)
wg_dimitrov_tick_kernel(int B, const wg::DimitrovConst *__restrict__ K, const wg_zmp_polytope_t *__restrict__ polys,
                        wg_dimitrov_state_t *states, wg_dimitrov_out_t *outs, int max_iter) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dim_lds[];
  const int N = K->N;
  const int g = blockIdx.x;
  if (g < B) (void)wg::dimitrov_tick(*K, dim_lds, polys + (size_t)g * N, states + g, outs ? outs + g : nullptr, max_iter);
}

// ---- modes QLD / QLDANDLQ: the same tick with the in-wave ql0002 as its back-end (wg_dimitrov_device.hpp, dimitrov_qld_tick) --

// `order`: longest-solve-first by the gait's last tick (scheduling only); iters_out[g] from lane 0, 0 for a refused gait.
template <bool kLQ, class Model, class Row>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
wg_dimitrov_qld_tick_form_kernel(int B, Model Mo, const wg_zmp_polytope_t *__restrict__ polys, wg_dimitrov_state_t *states,
                                 wg_dimitrov_out_t *outs, Row Ro, const int *__restrict__ order, int *__restrict__ iters_out) {
  extern __shared__ __attribute__((aligned(16))) double dimq_lds[];
  const int N = Mo.N();
  const int g = order ? wg::uni(order[blockIdx.x]) : (int)blockIdx.x;
  if (g >= B) return;
  wg_dimitrov_out_t *out = nullptr;
  if (!Ro.out(outs, B, g, &out)) return;
  const wg::DimitrovConst *K = Mo.bind(g);
  int it = 0;
  if (Model::kRefuses && !K) wg_dimitrov_refuse(out);
  else it = wg::dimitrov_qld_tick<kLQ>(*K, dimq_lds, polys + (size_t)g * N, states + g, out);
  if (iters_out && (threadIdx.x & 63) == 0) iters_out[g] = it;
}
// the plain form, as above
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
