// wg_prof.hpp -- the in-kernel phase timers of the diagnostic build (-DWG_PROFILE, lib/libwg_mpc_prof.so; never the measured or
// shipped library): the 48 slots of g_prof named once and the marks that fill them -- PT_* in the solver, TK_* in the tick,
// PT_LOCAL_* in a phase that times itself.  Without WG_PROFILE every mark is an empty statement and PT_PARAM / PT_ARG are nothing.
// ISA-sensitive: compare every kernel before changing a mark's empty form (`do {} while (0)` and `((void)0)` are not alike here).
#pragma once
#include <hip/hip_runtime.h>

namespace wg {

enum ProfSlot : int {   // the numbers are the interface: tools/probe_phases.py and tools/probe_tick_phases.py read them (wg_prof_read)
  // ql_solve, cycles (PT): set-up; refresh (24 - 27 are parts of 4); scan .. add; tail
  PS_NORMS = 0, PS_DIAGCHK = 1, PS_CHOL = 2 /* compact view: constant blocks into LDS */, PS_INVERSE = 3,
  PS_RESID = 4, PS_ZTWW_RESID = 5, PS_XSHIFT = 6, PS_BACKSUB_RESID = 7, PS_XMAG_RESID = 8,
  PS_SCAN = 9, PS_FDIFF = 10, PS_NEWNORMAL = 11, PS_SWEEP = 12, PS_ROUTE = 13, PS_STEP_PRE = 14, PS_BACKSUB_STEP = 15,
  PS_PICKDROP = 16, PS_STEP = 17, PS_ADD = 18, PS_XMAG_ADD = 19, PS_TAIL = 20,
  PS_RESET_BODY = 24, PS_RESID_GRAD = 25, PS_RESID_FWD = 26, PS_RESID_GX = 27,
  // event counts (PT_COUNT): route decisions, of which coordinate checks, dependent routes; 31: cycles, border rows of R
  PS_N_ROUTE = 28, PS_N_COORD = 29, PS_N_DEPENDENT = 30, PS_BORDER_ROWS = 31,
  PS_SW_NORMS = 32, PS_SW_COEFF = 33, PS_SW_ROWS = 34,   // sweep_flat's three phases (PT_SW)
  // mpc_tick, cycles (TK): 21 = 35 + 36 + 37 + 38 (state in, lane 0: FSM, lane 0: orientations, one instant per lane),
  // 22 the assembly, 23 = 39 + 40 + 41 + 42 (CoM, trunk, feet, samples into the queue) + the state store
  PS_TICK_PRE = 21, PS_TICK_ASSEMBLY = 22, PS_TICK_POST = 23,
  PS_TICK_LOAD = 35, PS_TICK_FSM = 36, PS_TICK_ORIENT = 37, PS_TICK_INSTANTS = 38,
  PS_TICK_COM = 39, PS_TICK_TRUNK = 40, PS_TICK_FEET = 41, PS_TICK_QUEUE = 42,
  // guarded sums (PT_COUNT2): local fallbacks at the dependence test, solves run again in the reference's order
  PS_N_FALLBACK = 43, PS_N_RERUN = 44,
  // the seeded norm chain (PT_SW_COUNT): sweeps of sweep_flat, those that took the seeded chain, those of them that fell back
  PS_N_SWEEPS = 45, PS_N_SEEDED = 46, PS_N_SEED_FALLBACK = 47,
  PS_COUNT = 48
};

#ifdef WG_PROFILE
__device__ unsigned long long g_prof[PS_COUNT];

// ---- the solver's timers: what PT_DECL declares is what a phase function receives ----
struct PtState {
  unsigned long long acc[28] = {0}, cnt[4] = {0}, sw[6] = {0}, cnt2[2] = {0};   // sw: three timers, then PS_N_SWEEPS ..
  unsigned long long last = clock64();
};
#define PT_DECL PtState pt;
#define PT_PARAM , PtState &pt
#define PT_ARG , pt
#define PT(k) do { unsigned long long t_ = clock64(); pt.acc[k] += t_ - pt.last; pt.last = t_; } while (0)
// a mark between two uses of a register value: the value goes through memory, so that the mark splits the chain it sits in
#define PT_VIA(k, mem, reg) do { mem = reg; PT(k); reg = mem; } while (0)
#define PT_FLUSH do { if ((threadIdx.x & 63) == 0) { for (int k_ = 0; k_ < 28; ++k_) if (k_ < PS_TICK_PRE || k_ > PS_TICK_POST) atomicAdd(&g_prof[k_], pt.acc[k_]); \
                                                      for (int k_ = 0; k_ < 4; ++k_) atomicAdd(&g_prof[PS_N_ROUTE + k_], pt.cnt[k_]); \
                                                      for (int k_ = 0; k_ < 3; ++k_) atomicAdd(&g_prof[PS_SW_NORMS + k_], pt.sw[k_]); \
                                                      for (int k_ = 0; k_ < 2; ++k_) atomicAdd(&g_prof[PS_N_FALLBACK + k_], pt.cnt2[k_]); \
                                                      for (int k_ = 0; k_ < 3; ++k_) atomicAdd(&g_prof[PS_N_SWEEPS + k_], pt.sw[3 + k_]); } } while (0)
#define PT_SW_PARAM , unsigned long long *ptsw = nullptr
#define PT_SW_ARG , pt.sw
#define PT_SW(k) do { if (ptsw) { unsigned long long t_ = clock64(); ptsw[(k) - PS_SW_NORMS] += t_ - ptsw_last; ptsw_last = t_; } } while (0)
#define PT_SW_BEGIN unsigned long long ptsw_last = clock64();
#define PT_SW_COUNT(k) do { if (ptsw) ptsw[3 + (k) - PS_N_SWEEPS]++; } while (0)
// event counters 28..31: kept in registers and flushed once (a global atomic per event would show up in the phase it sits in)
#define PT_COUNT(k) do { pt.cnt[(k) - PS_N_ROUTE]++; } while (0)
#define PT_COUNT2(k) do { pt.cnt2[(k) - PS_N_FALLBACK]++; } while (0)
// a phase that times itself: lane 0 adds the cycles since the previous mark to g_prof[k] at once
#define PT_LOCAL_BEGIN unsigned long long ptl_last = clock64();
#define PT_LOCAL(k) do { unsigned long long t_ = clock64(); if ((threadIdx.x & 63) == 0) atomicAdd(&g_prof[k], t_ - ptl_last); ptl_last = t_; } while (0)

// ---- the tick's timers ----
struct TkState {
  unsigned long long acc[PS_COUNT] = {0};                  // indexed by slot (constant indices: only the marked ones exist)
  unsigned long long last = clock64();
};
#define TK_DECL TkState tk;
#define TK(k) do { unsigned long long t_ = clock64(); tk.acc[k] += t_ - tk.last; tk.last = t_; } while (0)
#define TK_RESTART do { tk.last = clock64(); } while (0)      // what ran since the previous mark is charged elsewhere (the solve)
// the last mark (the state store) and the sums: lane 0 alone; constant indices only, so that acc stays in registers
#define TK_ADD_(k) atomicAdd(&g_prof[k], tk.acc[k])
#define TK_FLUSH do { if ((threadIdx.x & 63) == 0) { const unsigned long long store_ = clock64() - tk.last; \
    TK_ADD_(PS_TICK_LOAD); TK_ADD_(PS_TICK_FSM); TK_ADD_(PS_TICK_ORIENT); TK_ADD_(PS_TICK_INSTANTS); TK_ADD_(PS_TICK_ASSEMBLY); \
    TK_ADD_(PS_TICK_COM); TK_ADD_(PS_TICK_TRUNK); TK_ADD_(PS_TICK_FEET); TK_ADD_(PS_TICK_QUEUE); \
    atomicAdd(&g_prof[PS_TICK_PRE], tk.acc[PS_TICK_LOAD] + tk.acc[PS_TICK_FSM] + tk.acc[PS_TICK_ORIENT] + tk.acc[PS_TICK_INSTANTS]); \
    atomicAdd(&g_prof[PS_TICK_POST], tk.acc[PS_TICK_COM] + tk.acc[PS_TICK_TRUNK] + tk.acc[PS_TICK_FEET] + tk.acc[PS_TICK_QUEUE] + store_); } } while (0)
#else
#define PT_DECL
#define PT_PARAM
#define PT_ARG
#define PT(k) do {} while (0)
#define PT_VIA(k, mem, reg) ((void)0)
#define PT_FLUSH do {} while (0)
#define PT_SW_PARAM
#define PT_SW_ARG
#define PT_SW(k) do {} while (0)
#define PT_SW_BEGIN
#define PT_SW_COUNT(k) do {} while (0)
#define PT_COUNT(k) do {} while (0)
#define PT_COUNT2(k) do {} while (0)
#define PT_LOCAL_BEGIN
#define PT_LOCAL(k) ((void)0)
#define TK_DECL
#define TK(k) ((void)0)
#define TK_RESTART ((void)0)
#define TK_FLUSH ((void)0)
#endif

}  // namespace wg
