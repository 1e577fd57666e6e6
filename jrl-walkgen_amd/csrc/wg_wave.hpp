// wg_wave.hpp -- one wavefront per problem: the rules every device header of the project follows, and the small tools they
// share.  Used by the QL solver (wg_ql_view.hpp, wg_ql_phases.hpp, wg_ql_device.hpp) and -- without being solvers -- by the PLDP,
// Dimitrov and tick headers.
//
// Rules (gfx950 / CDNA4):
//   * one 64-lane wavefront owns one problem; a workgroup is exactly one wave, so
//     no s_barrier is ever needed -- LDS traffic of one wave is processed in
//     order, only the compiler has to be fenced (WG_WSYNC);
//   * lanes parallelise over *independent outputs* only (rows of Z, columns of
//     R, constraint rows of A); every inner sum runs sequentially inside one
//     lane in the reference's order, so every double is bit-identical to the
//     CPU solver and the active-set add/drop sequence is reproduced exactly
//     (one stated exception: sums that only decide a branch, under the
//     certificates of wg_ql_guard.hpp -- wave_sum_tree below);
//   * order-insensitive reductions (max, arg-max with first-index tie-break,
//     "any") use wave shuffles;
//   * the long scalar chains (Givens sweep norms, triangular solves) are
//     executed redundantly by all lanes on LDS-broadcast operands.
// Tools: the unroll pragmas, WG_WSYNC, the opaque lane index (wg_lane), wave-uniform values (uni, WG_UBOOL), lane broadcasts and
// ordered lane sums (rl, lane_sum_ordered), constants kept where they are used (wg_kconst), f2c's max / min, and the reductions
// on the DPP data path (wave_max, wave_min_int, wave_max_int, wave_argmax_first).
#pragma once
#include <hip/hip_runtime.h>

namespace wg {

#ifndef WG_UNROLL_N
#define WG_UNROLL_N 4
#endif
#define WG_PRAGMA(x) _Pragma(#x)
#define WG_UNROLL_(n) WG_PRAGMA(unroll n)
#define WG_UNROLL WG_UNROLL_(WG_UNROLL_N)

#define WG_WSYNC()                                          \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  \
    __builtin_amdgcn_wave_barrier();                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  \
  } while (0)

// lane index, opaque to the optimiser: inside a persistent loop (wg_mpc_run_kernel) nothing derived from it can be hoisted
// out of the loop and kept alive across a whole tick (that hoisting costs ~180 spilled registers)
__device__ __forceinline__ int wg_lane() { int l = threadIdx.x & 63; asm volatile("" : "+v"(l)); return l; }
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  return __hiloint2double(hi, lo);
}
// A wave-uniform predicate as a scalar: every lane computes the same value redundantly, so taking lane 0's copy is the
// identity -- but it tells the compiler the branch is uniform (s_cbranch on SCC instead of exec-mask juggling), which
// also keeps everything assigned under it (nact, knext, loop counters, LDS addresses) in scalar registers.
#define WG_UBOOL(c) (uni((int)(c)) != 0)
// value of `v` in lane `src` (src must be wave-uniform): two v_readlane_b32, no LDS round trip
__device__ __forceinline__ double rl(double v, int src) {
  int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
// sum_{j=lo}^{hi-1} v[lane j] in index order, starting from 0.0.  `v` must be 0.0 in every lane that is not in
// [lo, hi): adding +0.0 never changes a running sum, so the loop can run in chunks of four without a remainder
// loop (v_readlane is convergent and the compiler will not unroll it itself).  Needs hi <= 61.
__device__ __forceinline__ double lane_sum_ordered(double v, int lo, int hi) {
  double sum = 0.0;
  for (int j = lo; j < hi; j += 4) {
    sum += rl(v, j);
    sum += rl(v, j + 1);
    sum += rl(v, j + 2);
    sum += rl(v, j + 3);
  }
  return sum;
}
// A double constant materialised where it is used (two s_mov_b32), opaque to the optimiser: left to itself the compiler hoists
// 64-bit literals (0.1, 0.2, 1e-8, 0.01, 1.5 ...) out of the persistent loop into VGPR pairs at kernel entry, runs out of
// registers, SPILLS them and reloads them from scratch memory inside the active-set loop -- seen in the 256-register tick kernel:
// every scratch_ instruction at loop depth 2 was the reload of such a constant.
__device__ __forceinline__ double wg_kconst(double c) {
  int lo = __double2loint(c), hi = __double2hiint(c);
  asm volatile("" : "+s"(lo), "+s"(hi));
  return __hiloint2double(hi, lo);
}
// f2c.h max/min (qld.cpp:269-270)
__device__ __forceinline__ double maxd(double a, double b) { return a >= b ? a : b; }
__device__ __forceinline__ double mind(double a, double b) { return a <= b ? a : b; }

// ---- wave reductions on the DPP data path (gfx9 row shifts / row broadcasts: one VALU move per 32-bit half and step, no
// LDS crossbar, no exec-mask branching).  max / min are idempotent, so lanes without a partner just keep their own value
// (update_dpp's `old` operand): after row_shr 1,2,4,8 lane 15 of every row holds the row's result, row_bcast:15 and
// row_bcast:31 fold the rows into lane 63.  The __shfl_xor butterflies these replace cost ~1400 cycles per arg-max
// (three ds_bpermute per round plus divergent selects); this is ~250.
template <int CTRL>
__device__ __forceinline__ int dpp_keep(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ double dpp_keep(double v) {
  const int lo = dpp_keep<CTRL>(__double2loint(v)), hi = dpp_keep<CTRL>(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_max(double v) {
  v = __builtin_fmax(v, dpp_keep<0x111>(v));   // row_shr:1
  v = __builtin_fmax(v, dpp_keep<0x112>(v));   // row_shr:2
  v = __builtin_fmax(v, dpp_keep<0x114>(v));   // row_shr:4
  v = __builtin_fmax(v, dpp_keep<0x118>(v));   // row_shr:8
  v = __builtin_fmax(v, dpp_keep<0x142>(v));   // row_bcast:15
  v = __builtin_fmax(v, dpp_keep<0x143>(v));   // row_bcast:31
  return rl(v, 63);
}
__device__ __forceinline__ int wave_min_int(int v) {
  { const int o = dpp_keep<0x111>(v); v = o < v ? o : v; }
  { const int o = dpp_keep<0x112>(v); v = o < v ? o : v; }
  { const int o = dpp_keep<0x114>(v); v = o < v ? o : v; }
  { const int o = dpp_keep<0x118>(v); v = o < v ? o : v; }
  { const int o = dpp_keep<0x142>(v); v = o < v ? o : v; }
  { const int o = dpp_keep<0x143>(v); v = o < v ? o : v; }
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_max_int(int v) {
  { const int o = dpp_keep<0x111>(v); v = o > v ? o : v; }
  { const int o = dpp_keep<0x112>(v); v = o > v ? o : v; }
  { const int o = dpp_keep<0x114>(v); v = o > v ? o : v; }
  { const int o = dpp_keep<0x118>(v); v = o > v ? o : v; }
  { const int o = dpp_keep<0x142>(v); v = o > v ? o : v; }
  { const int o = dpp_keep<0x143>(v); v = o > v ? o : v; }
  return __builtin_amdgcn_readlane(v, 63);
}
// Sum of v over the 64 lanes as a balanced binary tree on the same data path (neighbours, pairs of pairs ... inside each row of
// 16, then rows 0 + 1 and 2 + 3, then the halves): lanes without a partner add +0.0 (bound_ctrl / a masked row keeps `old` = 0).
// NOT the reference's order of addition: only for the sums whose value decides a branch under a certificate (wg_ql_guard.hpp,
// whose guard_tree_sum is this order on the host).  Six dependent adds instead of a chain of n; result wave-uniform.
template <int CTRL, int ROWS>
__device__ __forceinline__ double dpp_zero(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWS, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWS, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_tree(double v) {
  v += dpp_zero<0x111, 0xf>(v);   // row_shr:1
  v += dpp_zero<0x112, 0xf>(v);   // row_shr:2
  v += dpp_zero<0x114, 0xf>(v);   // row_shr:4
  v += dpp_zero<0x118, 0xf>(v);   // row_shr:8: lane 15 of every row holds the row's sum
  v += dpp_zero<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v += dpp_zero<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return rl(v, 63);
}
// Inclusive prefix sums over the lanes on the same data path: lane i ends with v[0] + .. + v[i], added inside each row of 16 by
// doubling distances, then row 0's total into row 1 and row 2's into row 3, then the lower half's total into the upper half
// (wave_sum_tree's steps without the read-out).  NOT an order of the reference's: for values that only seed a computation checked
// afterwards (wg_ql_norms.hpp, whose norms_prefix_scan is this order on the host).
__device__ __forceinline__ double wave_prefix_sum(double v) {
  v += dpp_zero<0x111, 0xf>(v);   // row_shr:1
  v += dpp_zero<0x112, 0xf>(v);   // row_shr:2
  v += dpp_zero<0x114, 0xf>(v);   // row_shr:4
  v += dpp_zero<0x118, 0xf>(v);   // row_shr:8: every lane holds the prefix sum inside its row
  v += dpp_zero<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v += dpp_zero<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
  return v;
}
// arg-max over the wave: larger v wins, equal v -> smaller idx.  idx < 0 = no candidate (then idx stays < 0).
// Candidates must be finite.  Result is wave-uniform.
__device__ __forceinline__ void wave_argmax_first(double &v, int &idx) {
  const double vv = idx >= 0 ? v : -__builtin_huge_val();
  const double vmax = wave_max(vv);
  const int key = (idx >= 0 && v == vmax) ? idx : 0x7fffffff;
  const int kmin = wave_min_int(key);
  v = vmax;
  idx = kmin == 0x7fffffff ? -1 : kmin;
}

}  // namespace wg
