// wg_footcons.cpp -- ZMP polytopes of a feet trajectory (host part of libwg_mpc.so): the argument check and the sequential
// walk of FootConstraintsAsLinearSystem::BuildLinearConstraintInequalities (src/Mathematics/FootConstraintsAsLinearSystem.cpp
// :258-539) over one gait's samples.  The geometry of a polytope is wg_footcons_geom.hpp, shared with the kernels of
// wg_foot_constraints_batch_dev / _append_dev.
//
// Runs once per step sequence (one polytope per support phase), far off the per-tick path: plain host C++.  Its output
// feeds wg_dimitrov_tick_batch (one wg_zmp_polytope_t per previewed instant, picked by time like
// ZMPConstrainedQPFastFormulation::BuildConstraintMatrices :783-795, 822-840 does).
#include "wg_footcons_geom.hpp"

extern "C" int wg_foot_constraints(int n, const double *time, const double *left, const int *left_type, const double *right,
                                   double sole_w, double sole_h, double constraint_x, double constraint_y, int cap,
                                   wg_zmp_polytope_t *polys, double *t_start, double *t_end) {
  if (n < 0 || cap < 0 || (n > 0 && (!time || !left || !left_type || !right)) || (cap > 0 && (!polys || !t_start || !t_end)))
    return WG_ERR_BAD_ARG;
  double hw = sole_w * 0.5, hh = sole_h * 0.5;
  hh -= constraint_y;
  hw -= constraint_x;
  double scratch[2 * wg::kFcSlots];
  const wg::FcPts<1> P{scratch};
  int state = wg::kFcDouble, count = 0;                   // sample 0 inherits DOUBLE_SUPPORT
  for (int i = 0; i < n; i++) {
    const double *L = left + 6 * (size_t)i, *R = right + 6 * (size_t)i;   // x, y, z, theta (degrees), ...
    const int s = wg::fc_classify(left_type[i], L[2], R[2]);
    const int next = s == wg::kFcInherit ? state : s;
    const bool fresh = i == 0 || next != state;
    state = next;
    if (fresh) {
      int nh = 4;
      if (state == wg::kFcDouble) {
        wg::fc_corners(P, 0, L[0], L[1], L[3], hw, hh);
        wg::fc_corners(P, 4, R[0], R[1], R[3], hw, hh);
        nh = wg::fc_hull8(P);
      } else {
        const double *F = L[2] < R[2] ? L : R;
        wg::fc_corners(P, 0, F[0], F[1], F[3], hw, hh);
      }
      wg_zmp_polytope_t poly;
      if (!wg::fc_polytope(P, nh, &poly)) return WG_ERR_BAD_ARG;
      if (count > 0 && count - 1 < cap) t_end[count - 1] = time[i];
      if (count < cap) {
        polys[count] = poly;
        t_start[count] = time[i];
        t_end[count] = time[i];
      }
      count++;
    }
    if (i == n - 1 && count > 0 && count - 1 < cap) t_end[count - 1] = time[i];
  }
  return count;
}
