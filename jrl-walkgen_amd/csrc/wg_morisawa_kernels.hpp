// wg_morisawa_kernels.hpp -- Morisawa-2007 analytic walks for fleets (include/wg_mpc.h: wg_morisawa_solve_dev, _sample_dev,
// _walk_dev and their fleet forms).  The arithmetic is wg_morisawa_math.hpp, the text the host twins compile too.
//
// wg_morisawa_solve_kernel<FLEET>: one wavefront per gait, a workgroup is that one wave (no s_barrier: wg_wave.hpp).  The whole
// trajectory block is made in LDS -- mo_solve's work area, sized by the launch's smax: 11 336 B at smax = 3, 27 368 B at 7,
// 65 280 B at 14, so a CU of 160 KiB keeps 14, 5 and 2 gaits -- and only a gait that came through is copied out, lane after lane
// over consecutive words: whole 128-byte lines, and a refused gait's block keeps the caller's bytes.  Lane 0 walks the support
// feet (a serial product of rotations); lanes take intervals, rows of Z, entries of w, polynomials; in the elimination lane i
// owns row i of Z (n <= 64), rows nmax + 1 doubles apart: an odd pitch, so the lanes of a column access fall on different banks.
// The pivot is the wave's arg-max "largest, then first" on the DPP path.  FLEET: the gait's own model from a device array; the
// one-model form takes it by value.  One text, two bindings.
//
// wg_morisawa_solve_long_kernel<FLEET> (wg_morisawa_long_*, smax up to 64): the same wave per gait around mo_solve_long.  LDS holds
// the image without the feet's polynomials and Z as a row band, rows 16 doubles apart as in the block -- 19 080 B at smax = 15,
// 38 800 B at 32, 75 920 B at 64: 8, 4 and 2 gaits per CU -- and the block is written only behind the factor.  In the elimination
// a lane owns an ELEMENT of the live window, 5 rows x (9 columns + 2 right-hand sides) = 55 lanes per step, behind the step's
// five multipliers; the pivot is a compare chain over the six words of the column that every lane reads (a broadcast), not a
// reduction.  Pitch 16: in the window's read the rows k + 1 and k + 3 of the first half-wave meet on 7 of the 32 eight-byte bank pairs (two passes
// for one ds_read_b64 per step); the next conflict-free pitch, 22, costs 12 672 B at smax = 64 and with them the second gait of a
// CU, so the block's pitch is the work area's too.
//
// wg_morisawa_resolve_kernel<FLEET>, wg_morisawa_resolve_long_kernel<FLEET> (wg_morisawa[_long]_resolve_*): a new plan on a solved
// block's timing, both right-hand sides through the block's kept factor (mo_resolve, mo_resolve_long) in the work areas of the two
// solves: no Z, no pivot search, no elimination of Z.
//
// wg_morisawa_sample_kernel<LONG>: lanes = gaits; LONG reads blocks of the long layout and asks for their header tag.  The outputs are time-major with the gait index fastest, so consecutive lanes store
// consecutive words (a lane per sample would scatter every store over B x 8 bytes); the price is that each lane gathers its own
// gait's coefficients, which stay in cache across the kMoSampleChunk consecutive samples a lane makes.  The kernel is bound by its
// stores: 152 B per gait and sample with every output wanted (2 + 4 + 12 doubles, 2 ints).  The clock -- t_start, then one
// addition of T per sample -- is made once per launch by wg_morisawa_clock_kernel (a serial chain: one lane) into a buffer of the
// context, lcap + 1 entries: entry lcap tells a walk that does not fit.
#pragma once
#include <hip/hip_runtime.h>

#include "wg_morisawa_math.hpp"
#include "wg_wave.hpp"

namespace wg {

struct MoWaveExec {
  __device__ int lane() const { return threadIdx.x; }
  __device__ int lanes() const { return 64; }
  __device__ void sync() const { WG_WSYNC(); }
  __device__ void argmax_first(double &v, int &idx) const { wave_argmax_first(v, idx); }
};

template <bool FLEET>
__global__ __launch_bounds__(64) void wg_morisawa_solve_kernel(const wg_morisawa_model_t model, const wg_morisawa_model_t *models, int B,
                                                               int smax, const wg_rel_step_t *steps, const int *n_steps,
                                                               const double *init_feet, const double *com0, double *blocks, int *status) {
  extern __shared__ double wg_mo_lds[];
  const int b = blockIdx.x;
  if (b >= B) return;
  const MoLayout L = mo_layout(smax);
  const wg_morisawa_model_t m = FLEET ? models[b] : model;
  const int rc = mo_solve(MoWaveExec(), m, smax, steps + (size_t)b * smax, n_steps[b], init_feet + 6 * (size_t)b, com0 + 3 * (size_t)b,
                          wg_mo_lds, L, nullptr);
  if (threadIdx.x == 0) status[b] = rc;
  if (rc != WG_OK) return;
  double *blk = blocks + (size_t)b * L.words;
  for (int e = threadIdx.x; e < L.words; e += 64) blk[e] = mo_image_word(wg_mo_lds, L, e);
}

// The long walk (smax up to WG_MORISAWA_LONG_MAX_STEPS): the same wave per gait around mo_solve_long.  LDS holds the image without
// the feet's polynomials and Z as a band (mo_work_long); the block is written by mo_solve_long itself, and only behind the factor.
template <bool FLEET>
__global__ __launch_bounds__(64) void wg_morisawa_solve_long_kernel(const wg_morisawa_model_t model, const wg_morisawa_model_t *models, int B,
                                                                    int smax, const wg_rel_step_t *steps, const int *n_steps,
                                                                    const double *init_feet, const double *com0, double *blocks,
                                                                    int *status) {
  extern __shared__ double wg_mo_lds[];
  const int b = blockIdx.x;
  if (b >= B) return;
  const MoLayout L = mo_layout_long(smax);
  const wg_morisawa_model_t m = FLEET ? models[b] : model;
  const int rc = mo_solve_long(MoWaveExec(), m, smax, steps + (size_t)b * smax, n_steps[b], init_feet + 6 * (size_t)b,
                               com0 + 3 * (size_t)b, wg_mo_lds, L, blocks + (size_t)b * L.words, nullptr);
  if (threadIdx.x == 0) status[b] = rc;
}

// The re-plan (wg_morisawa_resolve_*): a wave per gait around mo_resolve, in mo_solve's work area.  The gait's factor block is
// read over consecutive words, its rows into the padded pitch; in the substitution lane i owns row i as in mo_lu, so a column
// access stays on distinct banks.  factor_of (may be null: block 0) is checked here, everything else by mo_replan_ok; a refused
// gait writes its status and nothing else.
template <bool FLEET>
__global__ __launch_bounds__(64) void wg_morisawa_resolve_kernel(const wg_morisawa_model_t model, const wg_morisawa_model_t *models, int B,
                                                                 int smax, const double *factors, int n_factors, const int *factor_of,
                                                                 const wg_rel_step_t *steps, const double *init_feet, const double *com0,
                                                                 double *blocks, int *status) {
  extern __shared__ double wg_mo_lds[];
  const int b = blockIdx.x;
  if (b >= B) return;
  const MoLayout L = mo_layout(smax);
  const wg_morisawa_model_t m = FLEET ? models[b] : model;
  const int f = factor_of ? factor_of[b] : 0;
  int rc = WG_MORISAWA_BAD_INPUT;
  if (f >= 0 && f < n_factors)
    rc = mo_resolve(MoWaveExec(), m, smax, factors + (size_t)f * L.words, steps + (size_t)b * smax, init_feet + 6 * (size_t)b,
                    com0 + 3 * (size_t)b, wg_mo_lds, L);
  if (threadIdx.x == 0) status[b] = rc;
  if (rc != WG_OK) return;
  double *blk = blocks + (size_t)b * L.words;
  for (int e = threadIdx.x; e < L.words; e += 64) blk[e] = mo_image_word(wg_mo_lds, L, e);
}

// Its long twin around mo_resolve_long: the band in LDS at pitch 16, the feet's polynomials from the lanes to the block, the work
// area mo_work_long's; a lane per position and side in the forward pass, per row of the window in the backward pass.
template <bool FLEET>
__global__ __launch_bounds__(64) void wg_morisawa_resolve_long_kernel(const wg_morisawa_model_t model, const wg_morisawa_model_t *models,
                                                                      int B, int smax, const double *factors, int n_factors,
                                                                      const int *factor_of, const wg_rel_step_t *steps,
                                                                      const double *init_feet, const double *com0, double *blocks,
                                                                      int *status) {
  extern __shared__ double wg_mo_lds[];
  const int b = blockIdx.x;
  if (b >= B) return;
  const MoLayout L = mo_layout_long(smax);
  const wg_morisawa_model_t m = FLEET ? models[b] : model;
  const int f = factor_of ? factor_of[b] : 0;
  int rc = WG_MORISAWA_BAD_INPUT;
  if (f >= 0 && f < n_factors)
    rc = mo_resolve_long(MoWaveExec(), m, smax, factors + (size_t)f * L.words, steps + (size_t)b * smax, init_feet + 6 * (size_t)b,
                         com0 + 3 * (size_t)b, wg_mo_lds, L, blocks + (size_t)b * L.words);
  if (threadIdx.x == 0) status[b] = rc;
}

__global__ void wg_morisawa_clock_kernel(double t_start, double T, int count, double *clock) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double t = t_start;
  for (int k = 0; k < count; k++) {
    clock[k] = t;
    t += T;
  }
}

struct MoOut {
  double *zx, *zy, *com, *left, *right;
  int *ltype, *rtype;
};
constexpr int kMoSampleChunk = 8;

// LONG: blocks of the long layout, which carry the header tag; one text, two bindings (the short binding's instructions are
// those of the kernel before it had the parameter)
template <bool LONG>
__global__ __launch_bounds__(64) void wg_morisawa_sample_kernel(int B, int smax, const double *blocks, const int *status, const double *clock,
                                                                int lcap, MoOut O, int *length) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const MoLayout L = LONG ? mo_layout_long(smax) : mo_layout(smax);
  const double *blk = blocks + (size_t)b * L.words;
  int len = status ? status[b] : WG_OK;
  if (len >= 0) len = (LONG ? mo_block_ok_long(blk, smax) : mo_block_ok(blk, smax)) ? mo_count(clock, lcap, blk[3]) : WG_MORISAWA_BAD_INPUT;
  if (len > lcap) len = WG_MORISAWA_CAPACITY;
  if (blockIdx.y == 0 && length) length[b] = len;
  if (len <= 0) return;
  const size_t Bs = (size_t)B;
  const int k0 = blockIdx.y * kMoSampleChunk;
  for (int k = k0; k < k0 + kMoSampleChunk && k < lcap; k++) {
    MoSample o;
    mo_sample(blk, L, clock[k < len ? k : len - 1], o);       // past the walk: its last sample again
    const size_t r = (size_t)k;
    if (O.zx) O.zx[r * Bs + b] = o.zx;
    if (O.zy) O.zy[r * Bs + b] = o.zy;
    if (O.com)
      for (int c = 0; c < 4; c++) O.com[(r * 4 + c) * Bs + b] = o.com[c];
    if (O.left)
      for (int c = 0; c < 6; c++) O.left[(r * 6 + c) * Bs + b] = o.left[c];
    if (O.right)
      for (int c = 0; c < 6; c++) O.right[(r * 6 + c) * Bs + b] = o.right[c];
    if (O.ltype) O.ltype[r * Bs + b] = o.ltype;
    if (O.rtype) O.rtype[r * Bs + b] = o.rtype;
  }
}

}  // namespace wg
