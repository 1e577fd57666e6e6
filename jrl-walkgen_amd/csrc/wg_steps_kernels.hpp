// wg_steps_kernels.hpp -- wg_steps_plan_dev: the step stack of B gaits on the device, one wave per gait.
//
// Lane j of a gait's wave makes step j of THIS call (smax <= 64 = one wave).  Every lane runs the same pass over the gait's
// commands (wg_steps_plan.hpp's sp_scan: wave-uniform loads and arithmetic), which gives the verdict on the whole list -- a
// refusal is decided before the gait's first write -- the keep behind it, and tells the lane which command its step belongs to
// and the keep that command met.  The lanes then make their steps all at once: an arc's step i repeats the reference's i + 1
// additions of OmegaStep itself and takes its four wg_sin / wg_cos beside those of every other step of the call, whichever
// command they come from.  Each lane stores its whole 48-byte record; lane 0 stores the count and the stack.  No LDS, no
// barrier: B gaits are B independent waves (one lane per gait would walk 64 steps' trigonometry one after the other in B / 64).
#pragma once
#include <hip/hip_runtime.h>

#include "wg_steps_plan.hpp"

namespace wg {

constexpr int kSpWaves = 4;              // gaits (waves) per block

// The support times of a launch.  FLEET = false: the call's ss, ds (checked on the host).  FLEET = true (wg_steps_plan_fleet_dev):
// the gait's own, ss[b], ds[b]; a gait that runs with a non-finite one is refused like a gait with a bad list.
template <bool FLEET>
struct SpTimes {
  double ss, ds;
};
template <>
struct SpTimes<true> {
  const double *__restrict__ ss, *__restrict__ ds;
};

template <bool FLEET>
__device__ __forceinline__ void sp_plan_gait(int B, int ccap, const wg_step_cmd_t *__restrict__ cmds, const int *__restrict__ n_cmds,
                                             const SpTimes<FLEET> &t, wg_step_stack_t *stack, int smax,
                                             wg_rel_step_t *__restrict__ steps, int *__restrict__ n_steps) {
  const int b = blockIdx.x * kSpWaves + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  if (b >= B) return;
  const wg_step_stack_t S = stack[b];
  const int nc = n_cmds[b];
  const wg_step_cmd_t *C = cmds + (size_t)b * ccap;
  const bool runs = S.error == 0 && nc != 0;              // else: a refused gait stays refused, an idle one sits out
  int keep = S.keep, w_cmd = 0, w_keep = 0, w_i = 0, total = 0;
  double ss = 0.0, ds = 0.0;
  bool times_ok = true;
  if constexpr (FLEET) {
    if (runs) {
      ss = t.ss[b]; ds = t.ds[b];
      times_ok = sp_finite(ss) && sp_finite(ds);
    }
  } else {
    ss = t.ss; ds = t.ds;
  }
  if (runs) total = nc < 0 || nc > ccap || !sp_foot_ok(keep) || !times_ok ? WG_STEPS_BAD_INPUT : sp_scan(C, nc, smax, &keep, lane, &w_cmd, &w_keep, &w_i);
  if (lane < total) steps[(size_t)b * smax + lane] = sp_cmd_step(C[w_cmd], w_keep, w_i, ss, ds);
  if (lane != 0) return;
  n_steps[b] = total > 0 ? total : 0;
  if (total < 0) {
    stack[b].error = total;
  } else if (runs) {
    wg_step_stack_t T = S;
    T.keep = keep;
    T.n_given = S.n_given + total;
    stack[b] = T;
  }
}

template <bool FLEET>
__global__ __launch_bounds__(64 * kSpWaves) void wg_steps_plan_form_kernel(int B, int ccap, const wg_step_cmd_t *__restrict__ cmds,
                                                                            const int *__restrict__ n_cmds, SpTimes<FLEET> t,
                                                                            wg_step_stack_t *stack, int smax,
                                                                            wg_rel_step_t *__restrict__ steps, int *__restrict__ n_steps) {
  sp_plan_gait<FLEET>(B, ccap, cmds, n_cmds, t, stack, smax, steps, n_steps);
}
// the form with the call's times, under its own name and arguments
__global__ __launch_bounds__(64 * kSpWaves) void wg_steps_plan_kernel(int B, int ccap, const wg_step_cmd_t *__restrict__ cmds,
                                                                       const int *__restrict__ n_cmds, double ss, double ds,
                                                                       wg_step_stack_t *stack, int smax,
                                                                       wg_rel_step_t *__restrict__ steps, int *__restrict__ n_steps) {
  sp_plan_gait<false>(B, ccap, cmds, n_cmds, {ss, ds}, stack, smax, steps, n_steps);
}

}  // namespace wg
