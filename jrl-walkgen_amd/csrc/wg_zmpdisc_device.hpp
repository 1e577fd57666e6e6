// wg_zmpdisc_device.hpp -- ZMP reference queue and feet trajectories of a step sequence, batched over independent gaits.
//
// Device-side replacement for
//   ZMPDiscretization::GetZMPDiscretization      src/ZMPRefTrajectoryGeneration/ZMPDiscretization.cpp:143-173
//     = InitOnLine :319-513, OnLineAddFoot :573-1020 (per step), EndPhaseOfTheWalking :1129-1300,
//       FilterOutValues :1045-1109 (window of InitializeFilter :240-262), UpdateCurrentSupportFootPosition :515-558
//   FootTrajectoryGenerationStandard::UpdateFootPosition  src/FootTrajectoryGeneration/FootTrajectoryGenerationStandard.cpp:411-566
//   Polynome::Compute / Polynome3,4,5::SetParameters      src/Mathematics/Polynome.cpp:44-53, PolynomeFoot.cpp:41-57, 100-120, 174-195
//
// The reference walks one gait sample by sample: every output of the 11-tap (0.05 s) sin^2 filter is an ordered sum, the
// first outputs of each phase read earlier *filtered* outputs (FilterOutValues' `o + r` indexing), the ZMP ramp of a phase
// starts at the last filtered value of the previous one, and step types 3/4 accumulate.  Nothing inside a gait can be
// reordered without changing bits, so the parallel axis is the batch: one lane = one gait, 64 gaits per wave, every
// output array TIME-MAJOR ([sample][gait]) so that a wave stores 512-byte rows -- the layout wg_preview_kernel reads.
// Per lane the last nwin unfiltered and 2 nwin filtered samples live in LDS rings laid out [slot][axis][lane]
// (lane-contiguous: conflict-free).  Operation order follows the oracle restatement (oracle/zmpdisc_oracle.c) line by
// line; sin / cos come from include/wg_trig.h like in the tick kernel.
//
// The walk is one function template, zd_walk<RES, FLEET>.  RES = false is the whole-sequence kernel (InitOnLine, every
// OnLineAddFoot, EndPhaseOfTheWalking in one launch; nothing kept).  RES = true is the on-line form of the reference's public
// API: one launch runs InitOnLine + some steps (ZD_OP_BEGIN), some more OnLineAddFoot (ZD_OP_APPEND) or
// EndPhaseOfTheWalking (ZD_OP_END) and carries what the walk keeps between phases in a wg_zmpdisc_state_t per gait.  The
// walk only ever pushes samples and FilterOutValues reads at most nwin filtered samples back, so a resumed launch refills
// the filtered ring from the gait's own rows of zmp_x_tm / zmp_y_tm (the reference's deque) -- or, when the caller does not
// ask for the queue, from the tail the previous launch left in the state.  Everything resumable sits under
// `if constexpr (RES)`: the whole-sequence instantiation carries none of it.  FLEET = true is the twin with a model per gait
// (ZdLaneModel below).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#include "../../include/wg_mpc.h"
#ifndef WG_TRIG_FN
#define WG_TRIG_FN __host__ __device__ static inline
#endif
#include "../../include/wg_trig.h"

namespace wg {

#define WG_ZD_WIN_MAX 52                 // (nwin + 2 nwin) x 2 axes x 64 lanes x 8 B = 3 KB x nwin <= 160 KB
#define WG_ZD_PI 3.14159265358979323846
static_assert(WG_ZD_WIN_MAX <= WG_ZMPDISC_TAIL_MAX, "wg_zmpdisc_state_t::tail holds one filter window");

constexpr int kZdWinStd = 11;            // floor(0.05 / T) + 1 taps at the reference's T = 5 ms (ZMPDiscretization.cpp:240-262)
struct ZdConst {
  wg_zmpdisc_model_t M;
  int nwin, pad_;
  double win[WG_ZD_WIN_MAX];
};

struct ZdOut {                           // all optional, all time-major
  double *zx, *zy, *ztheta;              // [lcap][B]
  int *ztype;                            // [lcap][B]
  double *left, *right;                  // [lcap][6][B]
  int *ltype, *rtype;                    // [lcap][B]
};

struct ZdFoot {
  double x, y, z, theta, omega, omega2;
  int type;
};

struct ZdPoly {
  double c[6];
};

__device__ __forceinline__ double zd_poly(const ZdPoly &p, int n, double t) {   // Polynome::Compute
  double r = 0.0, pt = 1.0;
#pragma unroll
  for (int i = 0; i < 6; i++)
    if (i < n) {
      r += p.c[i] * pt;
      pt *= t;
    }
  return r;
}
__device__ __forceinline__ void zd_poly3(ZdPoly &p, double FT, double FP) {
  p.c[0] = 0.0; p.c[1] = 0.0; p.c[4] = 0.0; p.c[5] = 0.0;
  double tmp = FT * FT;
  if (FP == 0.0 || FT == 0.0) {
    p.c[2] = 0.0; p.c[3] = 0.0;
  } else {
    p.c[2] = 3.0 * FP / tmp;
    p.c[3] = -2.0 * FP / (tmp * FT);
  }
}
__device__ __forceinline__ void zd_poly4(ZdPoly &p, double FT, double MP) {
  p.c[0] = 0.0; p.c[1] = 0.0; p.c[5] = 0.0;
  double tmp = FT * FT;
  if (MP == 0.0 || tmp == 0.0) {
    p.c[2] = p.c[3] = p.c[4] = 0.0;
  } else {
    p.c[2] = 16.0 * MP / tmp;
    tmp = tmp * FT;
    p.c[3] = -32.0 * MP / tmp;
    tmp = tmp * FT;
    p.c[4] = 16.0 * MP / tmp;
  }
}
__device__ __forceinline__ void zd_poly5(ZdPoly &p, double FT, double FP) {
  p.c[0] = p.c[1] = p.c[2] = 0.0;
  double tmp = FT * FT * FT;
  if (FP == 0.0 || tmp == 0.0) {
    p.c[3] = p.c[4] = p.c[5] = 0.0;
  } else {
    p.c[3] = 10 * FP / tmp;
    tmp *= FT;
    p.c[4] = -15 * FP / tmp;
    tmp *= FT;
    p.c[5] = 6 * FP / tmp;
  }
}

// host + device: number of samples of a sequence (the arithmetic of InitOnLine :390-391, OnLineAddFoot :636-641,
// EndPhaseOfTheWalking :1147-1148, 1248-1249), or a negative code
__host__ __device__ inline int zd_length(const wg_zmpdisc_model_t &M, const wg_rel_step_t *steps, int n_steps) {
  if (n_steps < 2 || n_steps > WG_ZMPDISC_MAX_STEPS || !(M.T > 0)) return WG_ZMPDISC_BAD_INPUT;
  long long n = (int)(2 * M.preview_time / M.T);
  if (n < 3) return WG_ZMPDISC_BAD_INPUT;
  for (int i = 1; i < n_steps; i++) {
    double d = M.t_double, s = M.t_single;
    if (steps[i].ds_time != 0.0) {
      d = steps[i].ds_time;
      s = steps[i].ss_time;
    }
    const double a = round((d + s) / M.T), a1 = round(d / M.T), a2 = round(s / M.T);
    if (!(a >= 1.0 && a < 1048576.0) || a1 < 1.0 || a1 + a2 > a) return WG_ZMPDISC_BAD_INPUT;
    n += (long long)a;
  }
  const double e = round(M.t_double / (2 * M.T)), r = 3.0 * M.preview_time / M.T;
  if (!(e >= 1.0 && e < 1048576.0) || !(r >= 0.0 && r < 16777216.0)) return WG_ZMPDISC_BAD_INPUT;
  n += (long long)e + (int)r;
  return n > (1 << 24) ? WG_ZMPDISC_BAD_INPUT : (int)n;
}

// host + device: samples of the phases, one by one (the terms of zd_length's sum), or a negative code
__host__ __device__ inline int zd_init_samples(const wg_zmpdisc_model_t &M) {
  if (!(M.T > 0)) return WG_ZMPDISC_BAD_INPUT;
  const int n = (int)(2 * M.preview_time / M.T);
  return n < 3 || n > (1 << 24) ? WG_ZMPDISC_BAD_INPUT : n;
}
__host__ __device__ inline int zd_step_samples(const wg_zmpdisc_model_t &M, const wg_rel_step_t &s) {
  double d = M.t_double, ss = M.t_single;
  if (s.ds_time != 0.0) {
    d = s.ds_time;
    ss = s.ss_time;
  }
  const double a = round((d + ss) / M.T), a1 = round(d / M.T), a2 = round(ss / M.T);
  if (!(a >= 1.0 && a < 1048576.0) || a1 < 1.0 || a1 + a2 > a) return WG_ZMPDISC_BAD_INPUT;
  return (int)a;
}
__host__ __device__ inline int zd_end_samples(const wg_zmpdisc_model_t &M) {
  const double e = round(M.t_double / (2 * M.T)), r = 3.0 * M.preview_time / M.T;
  if (!(e >= 1.0 && e < 1048576.0) || !(r >= 0.0 && r < 16777216.0)) return WG_ZMPDISC_BAD_INPUT;
  return (int)e + (int)r;
}
// samples `n` further steps add to a walk that holds `have`, or a negative code; the total stays within zd_length's 2^24
__host__ __device__ inline int zd_steps_samples(const wg_zmpdisc_model_t &M, const wg_rel_step_t *steps, int n, int have) {
  long long tot = have;
  for (int i = 0; i < n; i++) {
    const int a = zd_step_samples(M, steps[i]);
    if (a < 0) return a;
    tot += a;
    if (tot > (1 << 24)) return WG_ZMPDISC_BAD_INPUT;
  }
  return (int)(tot - have);
}
// samples after the first n_steps >= 2 steps of a sequence (InitOnLine on them), and after EndPhaseOfTheWalking if `ended`:
// the prefix sums of zd_length.  An on-line walk has no bound on its number of steps, only on its samples.
__host__ __device__ inline int zd_length_after(const wg_zmpdisc_model_t &M, const wg_rel_step_t *steps, int n_steps, int ended) {
  if (n_steps < 2) return WG_ZMPDISC_BAD_INPUT;
  const int n0 = zd_init_samples(M);
  if (n0 < 0) return n0;
  const int ns = zd_steps_samples(M, steps + 1, n_steps - 1, n0);
  if (ns < 0) return ns;
  long long n = (long long)n0 + ns;
  if (ended) {
    const int e = zd_end_samples(M);
    if (e < 0) return e;
    n += e;
  }
  return n > (1 << 24) ? WG_ZMPDISC_BAD_INPUT : (int)n;
}

// per-lane view of the two LDS rings
struct ZdRings {
  double *z, *f;      // base of this lane's column in the unfiltered / filtered ring
  int nwin, nf;       // slots
  __device__ __forceinline__ double &Z(int slot, int axis) { return z[(slot * 2 + axis) * 64]; }
  __device__ __forceinline__ double &F(int slot, int axis) { return f[(slot * 2 + axis) * 64]; }
};

// One phase (InitOnLine's rest, one OnLineAddFoot, or the end phase) is described by how its unfiltered samples are
// generated; the filter / output loop is common.
enum { ZD_INIT = 0, ZD_STEP = 1, ZD_END = 2 };

// what a resumable launch does (the reference's three on-line entry points)
enum { ZD_OP_BEGIN = 0, ZD_OP_APPEND = 1, ZD_OP_END = 2 };
#define WG_ZD_STATE_MAGIC 0x5a4d5044     // wg_zmpdisc_state_t::begun once InitOnLine has run on it

// A fleet launch (FLEET): a model per gait, models[model_of[g]], or models[g] where model_of is NULL (the host checks M == B).
struct ZdFleet {
  const wg_zmpdisc_model_t *models;      // [M]
  const int *model_of;                   // [B] or NULL
  int M, pad_;
};

constexpr int kZdModelWords = (int)(sizeof(wg_zmpdisc_model_t) / 8);
static_assert(kZdModelWords * 8 == (int)sizeof(wg_zmpdisc_model_t), "wg_zmpdisc_model_t: doubles only");
// LDS of a launch: the rings, and behind them the models of a fleet wave, [field][lane] like the rings (conflict-free)
__host__ __device__ inline size_t zd_lds_bytes(int nwin, bool fleet) {
  return ((size_t)nwin * 3 * 2 + (fleet ? kZdModelWords : 0)) * 64 * 8;
}

// The model as the walk reads it.  FLEET = false: the kernel argument itself, wave-uniform (SGPRs).  FLEET = true: the lane's
// own model.  It is not carried in registers across the walk (the kernel sits at one wave per SIMD as it is): the lane keeps it
// in its column of the LDS table above, and ZdLaneModel names the fields of that column like wg_zmpdisc_model_t names its own --
// a field is read from LDS where the walk uses it: most of them at the head of a phase, t_single, omega and foot_b / h / f per
// sample.  T is the launch's (a gait whose own T differs is refused), so the window, the taps and the filter stay wave-uniform.
struct ZdLdsField {
  const double *p;
  __device__ __forceinline__ operator double() const { return *p; }
};
struct ZdLaneModel {
  double T;
  ZdLdsField preview_time, t_single, t_double, step_height, omega, modulation, zmp_neutral[2], zmp_shift[4], foot_b, foot_h, foot_f;
#define WG_ZD_COL(field) {col + offsetof(wg_zmpdisc_model_t, field) / 8 * 64}
  __device__ __forceinline__ ZdLaneModel(double T_, const double *col)
      : T(T_), preview_time WG_ZD_COL(preview_time), t_single WG_ZD_COL(t_single), t_double WG_ZD_COL(t_double),
        step_height WG_ZD_COL(step_height), omega WG_ZD_COL(omega), modulation WG_ZD_COL(modulation),
        zmp_neutral{WG_ZD_COL(zmp_neutral[0]), WG_ZD_COL(zmp_neutral[1])},
        zmp_shift{WG_ZD_COL(zmp_shift[0]), WG_ZD_COL(zmp_shift[1]), WG_ZD_COL(zmp_shift[2]), WG_ZD_COL(zmp_shift[3])},
        foot_b WG_ZD_COL(foot_b), foot_h WG_ZD_COL(foot_h), foot_f WG_ZD_COL(foot_f) {}
#undef WG_ZD_COL
};
template <bool FLEET>
using ZdModelView = std::conditional_t<FLEET, const ZdLaneModel, const wg_zmpdisc_model_t &>;
template <bool FLEET>
__device__ __forceinline__ ZdModelView<FLEET> zd_model_view(const ZdConst &K, const double *col) {
  if constexpr (FLEET) return ZdLaneModel(K.M.T, col);
  else return K.M;
}

// RES = false: `op`, `select` and `state` are unused.  RES = true: `steps` holds only the steps of this launch (ZD_OP_BEGIN:
// the first n_steps[g] >= 2 of the walk; ZD_OP_APPEND: n_steps[g] >= 0 further ones), `select` (ZD_OP_END, may be NULL)
// names the gaits that end.  A gait that sits a launch out (0 steps, not selected) returns before it touches anything.
// FLEET = false: `FL` is unused and every gait walks with K.M.  FLEET = true: gait g walks with its own model out of FL; K.M is the
// base model, of which only T is read.  A gait whose model_of lies outside [0, FL.M), or whose T is not the base's bit for bit,
// is refused with WG_ZMPDISC_BAD_INPUT where the other refusals are decided.  Everything of the fleet sits under
// `if constexpr (FLEET)` or in ZdLaneModel: the instantiations without it carry none of it.
template <bool RES, bool FLEET>
__device__ __forceinline__ void zd_walk(const ZdConst &K, const ZdFleet &FL, int op, int B, int smax,
                                        const wg_rel_step_t *__restrict__ steps, const int *__restrict__ n_steps,
                                        const double *__restrict__ init_feet, const int *__restrict__ select, int lcap,
                                        const ZdOut &O, wg_zmpdisc_state_t *__restrict__ state, int *__restrict__ length) {
  extern __shared__ __attribute__((aligned(16))) double zd_lds[];
  const int lane = threadIdx.x;
  const int g = blockIdx.x * 64 + lane;
  if (g >= B) return;
  [[maybe_unused]] wg_zmpdisc_model_t Mg;           // FLEET: the gait's model, from here to the LDS table and no further
  [[maybe_unused]] bool model_ok = true;
  [[maybe_unused]] auto load_model = [&]() {        // called once, by a gait that does not sit the launch out
    const int mi = FL.model_of ? FL.model_of[g] : g;
    model_ok = mi >= 0 && mi < FL.M;
    Mg = FL.models[model_ok ? mi : 0];
    model_ok = model_ok && __double_as_longlong(Mg.T) == __double_as_longlong(K.M.T);
  };
  const wg_zmpdisc_model_t &Mh = [&]() -> const wg_zmpdisc_model_t & {   // what the sample counts are made from
    if constexpr (FLEET) return Mg;
    else return K.M;
  }();
  const size_t sB = (size_t)B;
  const wg_rel_step_t *st = steps + (size_t)g * smax;
  int S = 0;                                        // RES = false / ZD_OP_BEGIN: steps of the sequence, the first one included
  int nz0 = 0;                                      // RES: samples the walk holds when this launch starts
  wg_zmpdisc_state_t *sp = nullptr;
  if constexpr (!RES) {
    S = n_steps[g];
    if constexpr (FLEET) load_model();
    int Ltot = (S <= smax) ? zd_length(Mh, st, S) : WG_ZMPDISC_BAD_INPUT;
    if constexpr (FLEET)
      if (!model_ok) Ltot = WG_ZMPDISC_BAD_INPUT;
    if (Ltot > lcap) Ltot = WG_ZMPDISC_CAPACITY;
    if (length) length[g] = Ltot;
    if (Ltot < 0) return;
  } else {
    // every refusal is decided here, before the first sample: a refused launch writes the code and nothing else
    sp = state + g;
    int code;
    if (op == ZD_OP_BEGIN) {
      S = n_steps[g];
      if constexpr (FLEET) load_model();
      code = (S >= 2 && S <= smax) ? zd_length_after(Mh, st, S, 0) : WG_ZMPDISC_BAD_INPUT;
      if constexpr (FLEET)
        if (!model_ok) code = WG_ZMPDISC_BAD_INPUT;
      if (code > lcap) code = WG_ZMPDISC_CAPACITY;
      if (code < 0) {
        sp->begun = WG_ZD_STATE_MAGIC; sp->error = code; sp->ended = 0; sp->n_samples = 0; sp->n_steps = 0;
      }
    } else {
      S = op == ZD_OP_APPEND ? n_steps[g] : (select ? (select[g] != 0) : 1);
      if (S == 0) return;
      if constexpr (FLEET) load_model();
      const bool begun = sp->begun == WG_ZD_STATE_MAGIC;
      code = !begun ? WG_ZMPDISC_BAD_INPUT : sp->error;
      if (code == 0 && sp->ended) code = WG_ZMPDISC_BAD_INPUT;
      if constexpr (FLEET)
        if (code == 0 && !model_ok) code = WG_ZMPDISC_BAD_INPUT;
      if (code == 0) {
        nz0 = sp->n_samples;
        if (op == ZD_OP_END) {
          code = zd_end_samples(Mh);
          if (code >= 0 && (long long)nz0 + code > (1 << 24)) code = WG_ZMPDISC_BAD_INPUT;
        } else {
          code = (S > 0 && S <= smax) ? zd_steps_samples(Mh, st, S, nz0) : WG_ZMPDISC_BAD_INPUT;
        }
        if (code >= 0 && nz0 + code > lcap) code = WG_ZMPDISC_CAPACITY;
      }
      if (code < 0) sp->error = code;
    }
    if (code < 0) {
      if (length) length[g] = code;
      return;
    }
  }

  const bool want_feet = O.left || O.right || O.ltype || O.rtype;   // otherwise only each phase's last sample is evaluated
  ZdRings R;
  R.nwin = K.nwin;
  R.nf = 2 * K.nwin;
  R.z = zd_lds + lane;
  R.f = zd_lds + (size_t)K.nwin * 2 * 64 + lane;
  double *mcol = nullptr;
  if constexpr (FLEET) {                            // the lane's column of the model table: only this lane ever touches it
    mcol = zd_lds + (size_t)K.nwin * 3 * 2 * 64 + lane;
    const double *src = reinterpret_cast<const double *>(&Mg);
#pragma unroll
    for (int f = 0; f < kZdModelWords; f++) mcol[f * 64] = src[f];
  }
  ZdModelView<FLEET> M = zd_model_view<FLEET>(K, mcol);

  // ---- gait state -------------------------------------------------------------------------------------------------------
  double s00 = 1.0, s01 = 0.0, s02 = 0.0, s10 = 0.0, s11 = 1.0, s12 = 0.0;   // m_CurrentSupportFootPosition rows 0, 1
  double p02 = 0.0, p12 = 0.0;                                               // translation of m_PrevCurrentSupportFootPosition
  double vpre0, vpre1, ang_support, ang_zmp;
  ZdFoot cl, cr;                                                             // back() of the final feet deques
  wg_rel_step_t rel0;
  const bool fresh = !RES || op == ZD_OP_BEGIN;                              // otherwise all of this comes from the state below
  if (fresh) {
  cl.x = init_feet[(size_t)g * 6 + 0]; cl.y = init_feet[(size_t)g * 6 + 1]; cl.theta = init_feet[(size_t)g * 6 + 2];
  cr.x = init_feet[(size_t)g * 6 + 3]; cr.y = init_feet[(size_t)g * 6 + 4]; cr.theta = init_feet[(size_t)g * 6 + 5];
  cl.z = cl.omega = cl.omega2 = 0.0; cr.z = cr.omega = cr.omega2 = 0.0;
  cl.type = cr.type = 0;
  rel0 = st[0];
  }
  double bpx = 0.0, bpy = 0.0, btheta = 0.0;        // FinalZMPPositions.back()
  double f0x = 0.0, f0y = 0.0;                      // FinalZMPPositions[0]
  int nz = 0;                                       // FinalZMPPositions.size()
  int fslot = 0;                                    // nz mod nf: where the next filtered sample goes in its ring

  auto bookkeeping = [&](double zmp_theta, int &who) {   // :370-383, :619-634
    if (rel0.sy < 0) {
      who = -1;
      vpre0 = cr.x - cl.x; vpre1 = cr.y - cl.y;
      ang_support = cr.theta - cl.theta;
      ang_zmp = cr.theta - zmp_theta;
    } else {
      who = 1;
      vpre0 = -cr.x + cl.x; vpre1 = -cr.y + cl.y;
      ang_support = cl.theta - cr.theta;
      ang_zmp = cl.theta - zmp_theta;
    }
  };
  auto update_support = [&](const wg_rel_step_t &s) {     // :515-558
    p02 = s02; p12 = s12;
    const double c = wg_cos(s.theta * WG_ZD_PI / 180.0), sn = wg_sin(s.theta * WG_ZD_PI / 180.0);
    double o00 = 0.0, o01 = 0.0, o10 = 0.0, o11 = 0.0;
    o00 += c * s00; o00 += -sn * s10;
    o01 += c * s01; o01 += -sn * s11;
    o10 += sn * s00; o10 += c * s10;
    o11 += sn * s01; o11 += c * s11;
    double v0 = 0.0, v1 = 0.0;
    v0 += o00 * s.sx; v0 += o01 * s.sy;
    v1 += o10 * s.sx; v1 += o11 * s.sy;
    s00 = o00; s01 = o01; s10 = o10; s11 = o11;
    s02 += v0; s12 += v1;
  };
  auto zmp_world = [&](double &w0, double &w1) {
    double t = 0.0;
    t += s00 * M.zmp_neutral[0]; t += s01 * M.zmp_neutral[1]; t += s02 * 1.0;
    w0 = t;
    t = 0.0;
    t += s10 * M.zmp_neutral[0]; t += s11 * M.zmp_neutral[1]; t += s12 * 1.0;
    w1 = t;
  };
  auto put_foot = [&](double *base, int *tbase, size_t l, const ZdFoot &f) {
    if (base) {
      double *p = base + l * 6 * sB + g;
      p[0] = f.x; p[sB] = f.y; p[2 * sB] = f.z; p[3 * sB] = f.theta; p[4 * sB] = f.omega; p[5 * sB] = f.omega2;
    }
    if (tbase) tbase[l * sB + g] = f.type;
  };

  if (fresh) {
    int who;
    bookkeeping((cr.theta + cl.theta) / 2.0, who);
  }

  // ---- phases -----------------------------------------------------------------------------------------------------------
  // phase ph is the rest (ph == 0), the end (ph == ph_end) or OnLineAddFoot on st[ph - st_off]
  int ph_first = 0, ph_stop = S + 1, ph_end = S;    // rest, S - 1 steps, end
  int st_off = 0;
  if constexpr (RES) {
    if (op == ZD_OP_BEGIN) {
      ph_end = -1; ph_stop = S;                     // rest, S - 1 steps
    } else {
      // the walk so far: what the phases above leave behind, and the filter's look-back
      s00 = sp->support[0]; s01 = sp->support[1]; s02 = sp->support[2];
      s10 = sp->support[3]; s11 = sp->support[4]; s12 = sp->support[5];
      p02 = sp->prev_support[0]; p12 = sp->prev_support[1];
      vpre0 = sp->prev_rel[0]; vpre1 = sp->prev_rel[1];
      ang_support = sp->ang_support; ang_zmp = sp->ang_zmp;
      cl.x = sp->left[0]; cl.y = sp->left[1]; cl.z = sp->left[2]; cl.theta = sp->left[3]; cl.omega = sp->left[4]; cl.omega2 = sp->left[5];
      cr.x = sp->right[0]; cr.y = sp->right[1]; cr.z = sp->right[2]; cr.theta = sp->right[3]; cr.omega = sp->right[4]; cr.omega2 = sp->right[5];
      cl.type = sp->left_type; cr.type = sp->right_type;
      rel0 = sp->last_step;
      bpx = sp->zmp_last[0]; bpy = sp->zmp_last[1]; btheta = sp->zmp_last[2];
      f0x = sp->zmp_first[0]; f0y = sp->zmp_first[1];
      nz = nz0;
      fslot = nz % R.nf;
      const int back = nz < R.nwin ? nz : R.nwin;   // FilterOutValues reads no further back than its window
      int slot = fslot;
      for (int k = 0; k < back; k++) {              // k-th sample before the next one
        slot = slot == 0 ? R.nf - 1 : slot - 1;
        const size_t l = (size_t)(nz - 1 - k);
        R.F(slot, 0) = O.zx ? O.zx[l * sB + g] : sp->tail[k][0];
        R.F(slot, 1) = O.zx ? O.zy[l * sB + g] : sp->tail[k][1];
      }
      if (op == ZD_OP_APPEND) {
        st_off = 1; ph_first = 1; ph_stop = S + 1; ph_end = -1;   // OnLineAddFoot on steps[0 .. S)
      } else {
        ph_first = 1; ph_stop = 2; ph_end = 1;
      }
    }
  }
  for (int ph = ph_first; ph < ph_stop; ph++) {
    const int kind = ph == 0 ? ZD_INIT : (ph == ph_end ? ZD_END : ZD_STEP);
    int nZ, n1 = 0, n2 = 0, t1 = 0, who = 1, n_end = 0;
    double px0 = 0, py0 = 0, theta0 = 0, dx = 0, dy = 0, w0 = 0, w1 = 0, mod_sst = 0, fin0 = 0, fin1 = 0;
    int type_ss = 0;
    ZdPoly qx, qy, qz, qth, qom, qom2, qzt;
    ZdFoot dsl = cl, dsr = cr;                      // the feet while nothing moves in this phase
    if (kind == ZD_INIT) {
      nZ = (int)(2 * M.preview_time / M.T);
      fin0 = M.zmp_neutral[0]; fin1 = M.zmp_neutral[1];
      dsl.type = dsr.type = 10;
    } else if (kind == ZD_STEP) {
      const wg_rel_step_t rel1 = st[ph - st_off];
      double lTdble = M.t_double, lTsingle = M.t_single;
      if (rel1.ds_time != 0.0) {
        lTdble = rel1.ds_time;
        lTsingle = rel1.ss_time;
      }
      bookkeeping(btheta, who);
      nZ = (int)(unsigned)round((lTdble + lTsingle) / M.T);
      update_support(rel0);
      n1 = (int)(unsigned)round(lTdble / M.T);
      n2 = (int)(unsigned)round(lTsingle / M.T);
      px0 = bpx; py0 = bpy; theta0 = btheta;
      zmp_world(w0, w1);
      dx = (w0 - px0) / (unsigned)n1; dy = (w1 - py0) / (unsigned)n1;
      t1 = rel1.step_type;
      if (t1 == 3) { dx = (s02 + M.zmp_shift[0] - px0) / (unsigned)n1; dy = (s12 - py0) / (unsigned)n1; }
      if (t1 == 4) { dx = (s02 + M.zmp_shift[2] - px0) / (unsigned)n1; dy = (s12 - py0) / (unsigned)n1; }
      if (t1 == 5) {
        dx = (s02 - (M.zmp_shift[0] + M.zmp_shift[2] + M.zmp_shift[1] + M.zmp_shift[3]) - px0) / (unsigned)n1;
        dy = (s12 - py0) / (unsigned)n1;
      }
      dsl.z = 0.0; dsr.z = 0.0;
      dsl.type = dsr.type = t1 + 10;
      // second phase set-up, :770-861
      const double next_theta = rel1.theta;
      const double rel_theta = next_theta + ang_support, rel_zmp_theta = next_theta + ang_zmp;
      const double c = wg_cos(next_theta * WG_ZD_PI / 180.0), s = wg_sin(next_theta * WG_ZD_PI / 180.0);
      double o00 = 0.0, o01 = 0.0, o10 = 0.0, o11 = 0.0;
      o00 += c * s00; o00 += -s * s10;
      o01 += c * s01; o01 += -s * s11;
      o10 += s * s00; o10 += c * s10;
      o11 += s * s01; o11 += c * s11;
      double vd0 = 0.0, vd1 = 0.0;
      vd0 += o00 * rel1.sx; vd0 += o01 * rel1.sy;
      vd1 += o10 * rel1.sx; vd1 += o11 * rel1.sy;
      const double vrel0 = vd0 + vpre0, vrel1 = vd1 + vpre1;
      vpre0 = vd0; vpre1 = vd1;
      mod_sst = lTsingle * M.modulation;
      const double end_lift = (lTsingle - mod_sst) * 0.5;
      zd_poly5(qx, mod_sst, vrel0);
      zd_poly5(qy, mod_sst, vrel1);
      zd_poly4(qz, M.t_single, M.step_height);
      zd_poly3(qth, mod_sst, rel_theta);
      zd_poly3(qom, end_lift, M.omega);
      zd_poly3(qom2, mod_sst, 2 * M.omega);
      zd_poly3(qzt, lTsingle, rel_zmp_theta);
      type_ss = who * rel0.step_type;
      rel0 = rel1;                                  // pop_front
    } else {
      update_support(rel0);                         // m_RelativeFootPositions.size() > 0
      n_end = (int)(unsigned)round(M.t_double / (2 * M.T));
      nZ = n_end + (int)(3.0 * M.preview_time / M.T);
      px0 = bpx; py0 = bpy; theta0 = btheta;
      const double pxf = 0.5 * (s02 + p02), pyf = 0.5 * (s12 + p12);
      dx = (pxf - px0) / (double)(unsigned)n_end; dy = (pyf - py0) / (double)(unsigned)n_end;
      dsl.type = dsr.type = 0;
    }

    // unfiltered sample r of this phase (called with r = 0, 1, 2, ... in order: the chains need the previous value)
    double gx = 0.0, gy = 0.0;                      // last generated
    int slot_top = -1;                              // ring slot of the last generated sample
    auto generate = [&](int r) {
      double x, y;
      if (kind == ZD_INIT) {
        const double coef = (double)r / (double)(unsigned)nZ;
        x = 0.0 + (fin0 - 0.0) * coef;
        y = 0.0 + (fin1 - 0.0) * coef;
      } else if (kind == ZD_STEP) {
        if (r < n1) {
          x = px0 + (unsigned)r * dx;
          y = py0 + (unsigned)r * dy;
        } else if (r < n1 + n2) {
          x = w0; y = w1;
          if (t1 == 3 || t1 == 4) {
            const double px02 = px0 + (unsigned)(n1 - 1) * dx, py02 = py0 + (unsigned)(n1 - 1) * dy;
            const double sh = t1 == 3 ? M.zmp_shift[1] : M.zmp_shift[3];
            const double ddx = (s02 + sh - px02) / (unsigned)n2, ddy = (s12 - py02) / (unsigned)n2;
            x = gx + ddx; y = gy + ddy;
          }
        } else {
          x = 0.0; y = 0.0;                         // value-initialised tail of the reference's deque (rounding mismatch)
        }
      } else {
        if (r == 0) { x = px0 + dx; y = py0 + dy; }
        else if (r < n_end) { x = gx + dx; y = gy + dy; }
        else { x = gx; y = gy; }
      }
      gx = x; gy = y;
      slot_top = slot_top + 1 == R.nwin ? 0 : slot_top + 1;
      R.Z(slot_top, 0) = x; R.Z(slot_top, 1) = y;
    };

    double z2x = 0.0, z2y = 0.0;                    // ZMPPositions[lshift] of the rest phase
    int gen = 0;                                    // samples generated so far
    for (; gen < 2 && gen < nZ; gen++) generate(gen);
    for (int i = 0; i < nZ; i++) {
      if (gen < nZ) {
        generate(gen);
        if (gen == 2) { z2x = gx; z2y = gy; }
        gen++;
      }
      // FilterOutValues, :1051-1105.  slot of unfiltered sample q (q <= gen - 1): slot_top - (gen - 1 - q), wrapped
      double l0 = 0.0, l1 = 0.0;
      const int o = nz - 1 - 2;
      if (i + 3 >= K.nwin && i + 2 < nZ) {          // every tap inside the phase: r = i + 2 - j is sample gen - 1 - j
        if (K.nwin == kZdWinStd) {
          // the standard window (T = 5 ms: 11 taps): all 22 ring reads requested before the first add -- the loop below waits for
          // an LDS round trip per tap, which was most of a sample's 2 800 cycles; the same products added in the same order
          double zx[kZdWinStd], zy[kZdWinStd];
          int slot = slot_top;
#pragma unroll
          for (int j = 0; j < kZdWinStd; j++) {
            zx[j] = R.Z(slot, 0); zy[j] = R.Z(slot, 1);
            slot = slot == 0 ? kZdWinStd - 1 : slot - 1;
          }
#pragma unroll
          for (int j = 0; j < kZdWinStd; j++) { const double wj = K.win[j]; l0 += wj * zx[j]; l1 += wj * zy[j]; }
        } else {
        int slot = slot_top;
        for (int j = 0; j < K.nwin; j++) {
          const double wj = K.win[j];
          l0 += wj * R.Z(slot, 0); l1 += wj * R.Z(slot, 1);
          slot = slot == 0 ? R.nwin - 1 : slot - 1;
        }
        }
      } else {
        for (int j = 0; j < K.nwin; j++) {
          int r = i - j + 2;
          const double wj = K.win[j];
          if (r < 0) {
            if (kind == ZD_INIT) {
              l0 += wj * z2x; l1 += wj * z2y;
            } else if (-r < o) {
              const int q = (o + r) % R.nf;
              l0 += wj * R.F(q, 0); l1 += wj * R.F(q, 1);
            } else {
              l0 += wj * f0x; l1 += wj * f0y;
            }
          } else {
            if (r >= nZ) r = nZ - 1;
            int slot = slot_top - (gen - 1 - r);
            if (slot < 0) slot += R.nwin;
            l0 += wj * R.Z(slot, 0); l1 += wj * R.Z(slot, 1);
          }
        }
      }
      // theta, stepType and the feet of sample i
      double th;
      int ty;
      ZdFoot fl = dsl, fr = dsr;
      if (kind == ZD_INIT) {
        th = 0.0; ty = 0;
      } else if (kind == ZD_END) {
        th = theta0; ty = 0;
      } else if (i < n1) {
        th = theta0; ty = t1 + 10;
      } else if (i < n1 + n2) {
        const int k = i - n1;
        th = zd_poly(qzt, 4, (unsigned)k * M.T) + theta0;
        ty = type_ss;
        if (want_feet || i == nZ - 1) {
        // UpdateFootPosition: local index k + 1 (the last double-support sample is the initial one)
        ZdFoot &sup = who == 1 ? fl : fr;
        ZdFoot &non = who == 1 ? fr : fl;
        sup.type = (-1) * t1;
        const ZdFoot i0 = non;
        const double local = (unsigned)(k + 1) * M.T;
        const double end_lift = (M.t_single - mod_sst) * 0.5, start_land = end_lift + mod_sst;
        non.omega2 = 0.0;
        non.type = t1;
        if (local < end_lift) {
          non.x = i0.x; non.y = i0.y; non.theta = i0.theta;
        } else if (local < start_land) {
          non.x = i0.x + zd_poly(qx, 6, local - end_lift);
          non.y = i0.y + zd_poly(qy, 6, local - end_lift);
          non.theta = i0.theta + zd_poly(qth, 4, local - end_lift);
        } else {
          non.x = i0.x + zd_poly(qx, 6, mod_sst);
          non.y = i0.y + zd_poly(qy, 6, mod_sst);
          non.theta = i0.theta + zd_poly(qth, 4, mod_sst);
        }
        non.z = i0.z + zd_poly(qz, 5, local);
        if (local < end_lift)
          non.omega = zd_poly(qom, 4, local);
        else if (local < start_land)
          non.omega = M.omega - zd_poly(qom2, 4, local - end_lift);
        else
          non.omega = zd_poly(qom, 4, local - start_land) - M.omega;
        const double lo = non.omega * WG_ZD_PI / 180.0, lt = non.theta * WG_ZD_PI / 180.0;
        const double ct = wg_cos(lt), stt = wg_sin(lt);
        double dX, dFZ;
        const double Bq = M.foot_b, H = M.foot_h, F = M.foot_f;
        if (lo < 0) {
          const double X1 = Bq * wg_cos(-lo), X2 = H * wg_sin(-lo), Z1 = H * wg_cos(-lo), Z2 = Bq * wg_sin(-lo);
          dX = -(Bq - X1 + X2);
          dFZ = Z1 + Z2 - H;
        } else {
          const double X1 = F * wg_cos(lo), X2 = H * wg_sin(lo), Z1 = H * wg_cos(lo), Z2 = F * wg_sin(lo);
          dX = (F - X1 + X2);
          dFZ = Z1 + Z2 - H;
        }
        non.x += ct * dX;
        non.y += stt * dX;
        non.z += dFZ;
        }
      } else {                                      // value-initialised tail
        th = 0.0; ty = 0;
        fl.x = fl.y = fl.z = fl.theta = fl.omega = fl.omega2 = 0.0; fl.type = 0;
        fr = fl;
      }
      // push
      const size_t l = (size_t)nz;
      if (O.zx) O.zx[l * sB + g] = l0;
      if (O.zy) O.zy[l * sB + g] = l1;
      if (O.ztheta) O.ztheta[l * sB + g] = th;
      if (O.ztype) O.ztype[l * sB + g] = ty;
      put_foot(O.left, O.ltype, l, fl);
      put_foot(O.right, O.rtype, l, fr);
      R.F(fslot, 0) = l0; R.F(fslot, 1) = l1;        // fslot == nz mod nf, kept by increment (no division per sample)
      fslot = fslot + 1 == R.nf ? 0 : fslot + 1;
      if (nz == 0) { f0x = l0; f0y = l1; }
      bpx = l0; bpy = l1; btheta = th;
      cl = fl; cr = fr;
      nz++;
    }
  }
  if constexpr (RES) {
    sp->support[0] = s00; sp->support[1] = s01; sp->support[2] = s02;
    sp->support[3] = s10; sp->support[4] = s11; sp->support[5] = s12;
    sp->prev_support[0] = p02; sp->prev_support[1] = p12;
    sp->prev_rel[0] = vpre0; sp->prev_rel[1] = vpre1;
    sp->ang_support = ang_support; sp->ang_zmp = ang_zmp;
    sp->left[0] = cl.x; sp->left[1] = cl.y; sp->left[2] = cl.z; sp->left[3] = cl.theta; sp->left[4] = cl.omega; sp->left[5] = cl.omega2;
    sp->right[0] = cr.x; sp->right[1] = cr.y; sp->right[2] = cr.z; sp->right[3] = cr.theta; sp->right[4] = cr.omega; sp->right[5] = cr.omega2;
    sp->left_type = cl.type; sp->right_type = cr.type;
    sp->last_step = rel0;
    sp->zmp_last[0] = bpx; sp->zmp_last[1] = bpy; sp->zmp_last[2] = btheta;
    sp->zmp_first[0] = f0x; sp->zmp_first[1] = f0y;
    if (!O.zx) {                                    // no queue to read the look-back from next time
      const int back = nz < R.nwin ? nz : R.nwin;
      int slot = fslot;
      for (int k = 0; k < back; k++) {
        slot = slot == 0 ? R.nf - 1 : slot - 1;
        sp->tail[k][0] = R.F(slot, 0); sp->tail[k][1] = R.F(slot, 1);
      }
    }
    sp->n_samples = nz;
    sp->n_steps = op == ZD_OP_BEGIN ? S : sp->n_steps + (op == ZD_OP_APPEND ? S : 0);
    sp->ended = op == ZD_OP_END;
    sp->error = 0;
    sp->begun = WG_ZD_STATE_MAGIC;
    if (length) length[g] = nz;
    if (op != ZD_OP_END) return;
  }
  // a gait at rest after its last sample: lets one preview launch cover a ragged batch
  for (size_t l = (size_t)nz; l < (size_t)lcap; l++) {
    if (O.zx) O.zx[l * sB + g] = bpx;
    if (O.zy) O.zy[l * sB + g] = bpy;
  }
}

__global__ void __launch_bounds__(64)
wg_zmpdisc_kernel(ZdConst K, int B, int smax, const wg_rel_step_t *__restrict__ steps, const int *__restrict__ n_steps,
                  const double *__restrict__ init_feet, int lcap, ZdOut O, int *__restrict__ length) {
  zd_walk<false, false>(K, ZdFleet{}, 0, B, smax, steps, n_steps, init_feet, nullptr, lcap, O, nullptr, length);
}

// BEGIN / APPEND / END of an on-line walk; `state` [B], one blob per gait
__global__ void __launch_bounds__(64)
wg_zmpdisc_online_kernel(ZdConst K, int op, int B, int smax, const wg_rel_step_t *__restrict__ steps,
                         const int *__restrict__ n_steps, const double *__restrict__ init_feet,
                         const int *__restrict__ select, int lcap, ZdOut O, wg_zmpdisc_state_t *__restrict__ state,
                         int *__restrict__ length) {
  zd_walk<true, false>(K, ZdFleet{}, op, B, smax, steps, n_steps, init_feet, select, lcap, O, state, length);
}

// Every form of the walk, zd_walk's own argument list; the two above are <false, false> and <true, false> under the names and with
// the arguments they are timed and audited by.  Launched for a model per gait: <false, true> wg_zmpdisc_full_fleet_dev, <true, true>
// _begin_ / _append_ / _end_fleet_dev.
template <bool RES, bool FLEET>
__global__ void __launch_bounds__(64)
wg_zmpdisc_form_kernel(ZdConst K, ZdFleet FL, int op, int B, int smax, const wg_rel_step_t *__restrict__ steps,
                       const int *__restrict__ n_steps, const double *__restrict__ init_feet, const int *__restrict__ select,
                       int lcap, ZdOut O, wg_zmpdisc_state_t *__restrict__ state, int *__restrict__ length) {
  zd_walk<RES, FLEET>(K, FL, op, B, smax, steps, n_steps, init_feet, select, lcap, O, state, length);
}

}  // namespace wg
