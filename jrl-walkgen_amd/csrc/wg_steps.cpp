// wg_steps.cpp -- the step stack on the host (host part of libwg_mpc.so): wg_steps_count and wg_steps_plan, the one-gait twins of
// wg_steps_plan_dev.  The arithmetic is wg_steps_plan.hpp, shared with the kernel; this file is the argument check and the
// sequential walk over a command list.  Plain host C++: no kernels, nothing here touches the GPU.
#include "wg_steps_plan.hpp"

extern "C" int wg_steps_count(const wg_step_cmd_t *cmds, int n_cmds) {
  if (n_cmds < 0 || (n_cmds > 0 && !cmds)) return WG_STEPS_BAD_INPUT;
  int keep = 1, c = 0, k = 0, i = 0;
  return wg::sp_scan(cmds, n_cmds, WG_ZMPDISC_MAX_STEPS, &keep, -1, &c, &k, &i);
}

extern "C" int wg_steps_plan(const wg_step_cmd_t *cmds, int n_cmds, double ss, double ds, wg_step_stack_t *stack, int smax,
                             wg_rel_step_t *steps, int *n_steps) {
  if (!stack || !steps || !n_steps || (n_cmds > 0 && !cmds) || smax < 1 || smax > WG_ZMPDISC_MAX_STEPS || !wg::sp_finite(ss) ||
      !wg::sp_finite(ds))
    return WG_ERR_BAD_ARG;
  *n_steps = 0;
  if (stack->error) return WG_OK;                          // sticky
  if (n_cmds == 0) return WG_OK;                           // the gait sits out
  int keep = stack->keep, c = 0, k = 0, i = 0;
  int total = n_cmds < 0 || !wg::sp_foot_ok(keep) ? WG_STEPS_BAD_INPUT : wg::sp_scan(cmds, n_cmds, smax, &keep, -1, &c, &k, &i);
  if (total < 0) {
    stack->error = total;
    return WG_OK;
  }
  int at = 0;
  k = stack->keep;
  for (c = 0; c < n_cmds; c++) {
    const int n = wg::sp_cmd_count(cmds[c], smax - at);
    for (i = 0; i < n; i++) steps[at + i] = wg::sp_cmd_step(cmds[c], k, i, ss, ds);
    k = wg::sp_keep_after(cmds[c], k, n);
    at += n;
  }
  stack->keep = keep;
  stack->n_given += total;
  *n_steps = total;
  return WG_OK;
}
