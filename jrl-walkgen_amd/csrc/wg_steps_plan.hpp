// wg_steps_plan.hpp -- the step generators of the reference's StepStackHandler, once, for the host call (wg_steps.cpp) and the
// kernel (wg_steps_kernels.hpp): what a command gives (how many steps, or a refusal), what it leaves in
// m_KeepLastCorrectSupportFoot, and step i of it.
//
//   StepStackHandler::PrepareForSupportFoot              src/StepStackHandler.cpp:754-764
//   StepStackHandler::CreateArcInStepStack               :299-457
//   StepStackHandler::FinishOnTheLastCorrectSupportFoot  :872-882
//   StepStackHandler::AddStepInTheStack                  :850-863
//   StepStackHandler::AddStandardOnLineStep              :791-832
//
// Plain C++ that a HIP translation unit compiles for both sides: WG_SP_HD is `__host__ __device__` there and nothing elsewhere,
// and nothing here names a kernel, a lane or a block index.  The arc follows the oracle's restatement (wgo_steps_arc) operation
// for operation: the library is built with -ffp-contract=off, / and sqrt are IEEE on both sides and sin / cos are
// include/wg_trig.h, so host, kernel and the oracle's portable-trigonometry build give the same bytes.
//
// An arc's step i does not depend on its steps before i but for the running angle, and that is a sum of equal addends: step i
// repeats the reference's i + 1 additions from 0.0 itself (sp_arc_step), so the steps of an arc may be made in any order, or
// all at once.
#pragma once
#include <cmath>

#include "../../include/wg_mpc.h"
#ifdef __HIP__
#define WG_SP_HD __host__ __device__
#else
#define WG_SP_HD
#endif
#define WG_SP_INLINE WG_SP_HD inline __attribute__((always_inline))
#ifndef WG_TRIG_FN
#define WG_TRIG_FN WG_SP_HD static inline
#endif
#include "../../include/wg_trig.h"

namespace wg {

constexpr double kSpPi = 3.14159265358979323846;
constexpr double kSpStepMax = 0.15;                 // CreateArcInStepStack's StepMax
// a double is finite iff x - x == 0 (inf - inf and nan - nan are nan); <cmath>'s isfinite is not spelt alike on both sides
WG_SP_INLINE bool sp_finite(double x) { return x - x == 0.0; }
WG_SP_INLINE bool sp_foot_ok(int foot) { return foot == 1 || foot == -1; }

// what CreateArcInStepStack derives from (x, y, arc_deg) before its loop
struct SpArc {
  double R, OmegaStep, LastOmegaStep;               // degrees, signed by y
  int NumberOfStep, DirectionRay;
  bool last;                                        // LastStep != 0.0: one shorter step closes the arc
};

// the arc's derived quantities and its count (NumberOfStep, + 1 with a last step) or a refusal; `room` is how many steps may
// still be given (the float is tested before it becomes an int)
WG_SP_INLINE int sp_arc_setup(double x, double y, double arc_deg, int room, SpArc *A) {
  double StepMax = kSpStepMax, LastStep, NumberOfStepFloat, OmegaStep, OmegaTotal = arc_deg * kSpPi / 180.0, LastOmegaStep;
  int DirectionRay = -1;
  const double R = sqrt(x * x + y * y);
  NumberOfStepFloat = OmegaTotal * R / StepMax;
  if (!sp_finite(R) || !(NumberOfStepFloat >= 0.0)) return WG_STEPS_BAD_INPUT;        // x * x overflowed: no arc of a finite radius
  const double whole = floor(NumberOfStepFloat);
  if (whole > (double)room) return WG_STEPS_CAPACITY;
  const int NumberOfStep = (int)whole;
  LastStep = OmegaTotal * R - NumberOfStep * StepMax;
  OmegaStep = StepMax / R;
  LastOmegaStep = OmegaTotal - OmegaStep * NumberOfStep;
  OmegaStep = OmegaStep * 180.0 / kSpPi;
  LastOmegaStep = LastOmegaStep * 180.0 / kSpPi;
  if (x < 0) {
    LastStep = -LastStep;
    DirectionRay = 1;
  }
  if (y < 0) {
    OmegaStep = -OmegaStep;
    LastOmegaStep = -LastOmegaStep;
  }
  A->R = R;
  A->OmegaStep = OmegaStep;
  A->LastOmegaStep = LastOmegaStep;
  A->NumberOfStep = NumberOfStep;
  A->DirectionRay = DirectionRay;
  A->last = LastStep != 0.0;
  const int n = NumberOfStep + (A->last ? 1 : 0);
  return n > room ? WG_STEPS_CAPACITY : n;
}

// step i of the arc that starts on SupportFoot: (sx, sy, theta)
WG_SP_INLINE void sp_arc_step(const SpArc &A, int SupportFoot, int i, double *sx, double *sy, double *theta) {
  const double dOmega = i == A.NumberOfStep ? A.LastOmegaStep : A.OmegaStep;
  const int full = i < A.NumberOfStep ? i : A.NumberOfStep;     // whole steps behind step i
  double Omegakp = 0.0;
  for (int k = 0; k < full; k++) Omegakp = Omegakp + A.OmegaStep;
  const double Omegak = Omegakp + dOmega;
  if (i & 1) SupportFoot = -SupportFoot;
  const double c = wg_cos(Omegak * kSpPi / 180.0), s = wg_sin(Omegak * kSpPi / 180.0);
  const double cp = wg_cos(Omegakp * kSpPi / 180.0), sp = wg_sin(Omegakp * kSpPi / 180.0);
  const double R = A.R;
  const int side = A.DirectionRay * SupportFoot;
  const double lv0 = (R + side * 0.095) * s - (R - side * 0.095) * sp;
  const double lv1 = -((R + side * 0.095) * c - (R - side * 0.095) * cp);
  double a = 0.0, b = 0.0;                                      // lv2 = A lv, A = [c s; -s c]
  a += c * lv0;
  a += s * lv1;
  b += -s * lv0;
  b += c * lv1;
  *sx = a;
  *sy = b;
  *theta = dOmega;
}

// how many steps command C gives when `room` more may be given, or the refusal it earns
WG_SP_INLINE int sp_cmd_count(const wg_step_cmd_t &C, int room) {
  if (!sp_finite(C.a[0]) || !sp_finite(C.a[1]) || !sp_finite(C.a[2])) return WG_STEPS_BAD_INPUT;
  switch (C.op) {
    case WG_STEP_NONE: return 0;
    case WG_STEP_SUPPORT_FOOT:
      if (!sp_foot_ok(C.foot)) return WG_STEPS_BAD_INPUT;
      break;
    case WG_STEP_ARC: {
      if (!sp_foot_ok(C.foot) || C.a[2] < 0.0) return WG_STEPS_BAD_INPUT;
      SpArc A;
      return sp_arc_setup(C.a[0], C.a[1], C.a[2], room, &A);
    }
    case WG_STEP_LAST_SUPPORT:
    case WG_STEP_ADD:
    case WG_STEP_ONLINE:
    case WG_STEP_ONLINE_IDLE: break;
    default: return WG_STEPS_BAD_INPUT;
  }
  return room < 1 ? WG_STEPS_CAPACITY : 1;
}

// m_KeepLastCorrectSupportFoot behind a command that gave n steps
WG_SP_INLINE int sp_keep_after(const wg_step_cmd_t &C, int keep, int n) {
  if (C.op == WG_STEP_ARC) return (n & 1) ? -C.foot : C.foot;   // the foot the arc ends on
  if (C.op == WG_STEP_ONLINE || C.op == WG_STEP_ONLINE_IDLE) return -keep;
  return keep;
}

// step i of command C, met with m_KeepLastCorrectSupportFoot == keep: a whole record, every byte of it
WG_SP_INLINE wg_rel_step_t sp_cmd_step(const wg_step_cmd_t &C, int keep, int i, double ss, double ds) {
  double sx = 0.0, sy = 0.0, theta = 0.0;
  switch (C.op) {
    case WG_STEP_SUPPORT_FOOT: sy = C.foot * 0.095; break;
    case WG_STEP_ARC: {
      SpArc A;
      sp_arc_setup(C.a[0], C.a[1], C.a[2], WG_ZMPDISC_MAX_STEPS, &A);
      sp_arc_step(A, C.foot, i, &sx, &sy, &theta);
      break;
    }
    case WG_STEP_ADD: sx = C.a[0]; sy = C.a[1]; theta = C.a[2]; break;
    case WG_STEP_ONLINE: sx = C.a[0]; sy = C.a[1] + keep * 0.19; theta = C.a[2]; break;
    default: sy = keep * 0.19; break;                           // LAST_SUPPORT, ONLINE_IDLE
  }
  wg_rel_step_t s;
  s.sx = sx;
  s.sy = sy;
  s.theta = theta;
  s.ss_time = ss;
  s.ds_time = ds;
  s.step_type = 0;
  s.pad_ = 0;
  return s;
}

// One pass over a gait's commands: the verdict on the whole list, and -- for the caller that makes step `want` -- where that
// step comes from.  Returns the number of steps (<= cap) or the refusal of the first command, in order, that earns one.
//   *keep      in: m_KeepLastCorrectSupportFoot before the list; out: behind it (unchanged on a refusal)
//   want       index of a step of this call, or -1; *w_cmd, *w_keep, *w_i: its command, the keep that command met, its index in it
WG_SP_INLINE int sp_scan(const wg_step_cmd_t *cmds, int n_cmds, int cap, int *keep, int want, int *w_cmd, int *w_keep, int *w_i) {
  int total = 0, k = *keep;
  for (int c = 0; c < n_cmds; c++) {
    const int n = sp_cmd_count(cmds[c], cap - total);
    if (n < 0) return n;
    if (want >= total && want < total + n) {
      *w_cmd = c;
      *w_keep = k;
      *w_i = want - total;
    }
    k = sp_keep_after(cmds[c], k, n);
    total += n;
  }
  *keep = k;
  return total;
}

}  // namespace wg
