// wg_tick_tables_math.hpp -- the arithmetic of the Herdt-2010 tick's per-model tables, once, for the host (wg::build_tables:
// wg_mpc_configure, wg_mpc_block) and for the kernel (wg_tick_kernels.hpp: wg_mpc_blocks_kernel, one wavefront per model).
//
//   RigidBodySystem::compute_dyn_cjerk       src/PreviewControl/rigid-body-system.cpp:377-452          (Sv, Sz, Uv, Uz)
//   GeneratorVelRef::build_invariant_part    src/ZMPRefTrajectoryGeneration/generator-vel-ref.cpp:587-614   (Q_b)
//   ql0002_ on blockdiag(Q_b, Q_b), eps = 1e-8: diagonal test qld.cpp:814-843, factor :859-890, its inverse :937-975
//
// Plain C++ that a HIP translation unit compiles for both sides, like wg_dimitrov_math.hpp: tt_build is a list of phases; a
// phase is a loop over independent outputs, `for (e = x.lane(); e < count; e += x.lanes())`, and x.sync() stands between a phase
// and the next one that reads what it wrote.  The host runs it with one lane and no fence (TtHostExec), the kernel with the 64
// lanes of a wavefront.  Lanes only split work between independent entries; every stored double is produced by the operations,
// in the order, of the serial loops this text replaces:
//   * Q_b: one (i, j) per lane, k ascending, the three `+=` of the weights in their order;
//   * diagonal test: a maximum over pairs, a row i per lane and the lanes' maxima folded in lane order -- every candidate
//     is folded into a running value that starts at +0.0 and never leaves [+0.0, inf), so the grouping cannot show (models
//     with a field that is not finite are refused before: no NaN takes part);
//   * R2: row by row -- the diagonal entry by every lane (sqrt first), then the quotients of the row, a column j > i per lane;
//     each entry's `temp` subtracts R(k, j) R(k, i) for k ascending, exactly as the column-by-column loop did;
//   * Z2: a row i per lane, the recurrence in j as it is, over the whole 2N x 2N matrix (the cross block's signed zeros are part
//     of the result; z2_cross_sign records them).
// The library is built with -ffp-contract=off, / and sqrt are IEEE on both sides: host and kernel give the same bytes.
//
// The work area (TtWork: Q_b, the packed factor, Z and the lanes' partial maxima, 57.6 KB) is LDS in the kernel.  Uv and Uz are
// closed forms of (i - j, T, h): generated where Q_b needs them, never read back.  The tables themselves are written at the very
// end, every element of every array once, zeros behind the parts the model's N uses: a block has one writer per byte.
// A FAILED FACTOR (blocks_ok == 0: the diagonal test or a pivot below eps) leaves R2, Z2 and the sign words all zero, on the host
// and on the device.  Nothing reads them then: the solver's set-up calls the problem view's factor() -- the only reader of
// R2 / Z2 / z2sign, through herdt_constant_blocks (wg_ql_herdt.hpp) -- only under `prob.blocks_ok` (wg_ql_device.hpp, ql_solve's
// set-up: `if (!need_shift && prob.blocks_ok) factored = prob.factor(...)`) and runs the generic recurrences otherwise.
#pragma once
#include <cmath>
#include <cstddef>

#include "../../include/wg_mpc.h"
#ifdef __HIP__
#define WG_TT_HD __host__ __device__
#else
#define WG_TT_HD
#endif
#define WG_TT_INLINE WG_TT_HD inline __attribute__((always_inline))

namespace wg {

constexpr int kNMaxH = 32;   // largest horizon
constexpr int kSMax = 4;     // largest number of previewed steps

// Condensed cart-table maps + invariant Hessian block, built once per model
// (RigidBodySystem::compute_dyn_cjerk, rigid-body-system.cpp:377-452;
//  GeneratorVelRef::build_invariant_part, generator-vel-ref.cpp:587-614).
struct TickTables {
  double Sv[kNMaxH][3], Sz[kNMaxH][3];
  double Uv[kNMaxH][kNMaxH], Uz[kNMaxH][kNMaxH];
  double Qb[kNMaxH][kNMaxH];
  // gait-independent part of ql0002's set-up for C = blockdiag(Qb, Qb) + border (wg_ql_herdt.hpp):
  double R2[2 * kNMaxH * (2 * kNMaxH + 1) / 2];   // packed Cholesky factor of blockdiag(Qb, Qb), qld.cpp:859-890
  double Z2[4 * kNMaxH * kNMaxH];                 // its inverse, column-major ld 2N, qld.cpp:937-975
  double diag_b;                                  // diagonal test over the constant block, qld.cpp:814-843
  int blocks_ok;
  int ql_sums;                                    // the compact view's decision-only sums (wg_ql_view.hpp: kSumsGuarded / Ordered / Doubt) and, in bits 8 - 9, its sweeps' norm chain (kNormsSeeded / Exact / Doubt)
  // Z2 is blockdiag(Zb, Zb) with zeros in between, but the recurrence leaves SIGNED zeros in the upper-right block
  // (-(x * 0) / r); bit i + j*N = sign of Z2(i, N + j).  The kernel fetches only Zb and re-creates the rest from this.
  unsigned long long z2_cross_sign[(kNMaxH * kNMaxH + 63) / 64];
};

// One model's block of wg_mpc_block*: the wg_model_t as given, zeros up to kMpcBlockTables, the TickTables, zeros up to a
// multiple of 128 bytes.  76 032 bytes whatever N is (TickTables is laid out for kNMaxH).
constexpr size_t kMpcBlockTables = 256;
constexpr size_t kMpcBlockBytes = (kMpcBlockTables + sizeof(TickTables) + 127) & ~(size_t)127;
static_assert(sizeof(wg_model_t) <= kMpcBlockTables && sizeof(wg_model_t) % 8 == 0 && sizeof(TickTables) % 8 == 0, "blocks are written in 8-byte words");

struct TtWork {
  double Qb[kNMaxH * kNMaxH];                     // leading dimension N
  double R2[2 * kNMaxH * (2 * kNMaxH + 1) / 2];   // packed, R(i, j) at j (j + 1) / 2 + i
  double Z2[4 * kNMaxH * kNMaxH];                 // column-major, leading dimension 2N
  double part[64];                                // the lanes' maxima of the diagonal test
};

struct TtHostExec {
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() const {}
};

// a double is finite iff x - x == 0 (inf - inf and nan - nan are nan)
WG_TT_INLINE bool tt_finite(double x) { return x - x == 0.0; }

// The most steps a horizon can preview, from SupportFSM::set_support_state as wg_tick_device.hpp states it: a previewed support
// changes at the first instant pi with time + 1e-6 + pi*T >= time_limit, and every change sets time_limit = time + pi*T +
// step_period - T/10, so two changes are k = ceil((step_period - T/10 - 1e-6) / T) instants apart.  A change at pi = 1 is not
// counted (`if (pi != 1) ++step_number`) and one at pi = 0 belongs to the current support: the earliest counted change is at
// pi = 2, the most a horizon of N instants holds is 1 + floor((N - 2) / k).  The 1e-9 keeps k from being rounded UP past the
// FSM's own figure (a smaller k only refuses more).  The kernels hold wg::kSMax steps: models beyond are refused.
WG_TT_INLINE int tt_max_prw_steps(const wg_model_t &m) {
  const double q = (m.step_period - m.T / 10.0 - 1e-6) / m.T - 1e-9;
  if (!(q == q)) return m.N;                                       // NaN: refuse
  const int k = q <= 1.0 ? 1 : (q >= (double)m.N ? m.N : (int)ceil(q));
  return 1 + (m.N - 2) / k;
}

// the step class of a model: true = "previews at most two steps" (what the compact view, N == 16, is sized for), false = "up
// to four".  Pure arithmetic on the model's fields, no environment: the same on the host and in a kernel.
WG_TT_INLINE bool tt_two_step_class(const wg_model_t &m) { return m.N == 16 && m.N * m.T <= 2.0 * m.step_period + 1e-12; }

// What a block can be made of: whatever wg_mpc_configure accepts (N in 2 .. 32, T / Tctrl == 20, at most four previewed steps)
// without a matrix-core Gramian, and with every field the tables or these tests are computed from finite.
WG_TT_INLINE bool tt_model_ok(const wg_model_t &m) {
  if (m.N < 2 || m.N > kNMaxH) return false;
  if (m.flags & (WG_FLAG_GRAMIAN_MFMA_F64 | WG_FLAG_GRAMIAN_MFMA_F32)) return false;
  if (!tt_finite(m.T) || !tt_finite(m.Tctrl) || !tt_finite(m.com_height_qp) || !tt_finite(m.alpha) || !tt_finite(m.beta) ||
      !tt_finite(m.gamma) || !tt_finite(m.step_period))
    return false;
  const double r = m.T / m.Tctrl;                                  // (int)(T / Tctrl) == WG_SAMPLES_PER_TICK, without the cast of an inf
  if (!(r >= (double)WG_SAMPLES_PER_TICK && r < (double)(WG_SAMPLES_PER_TICK + 1))) return false;
  return tt_max_prw_steps(m) <= kSMax;
}

// entries of the lower-triangular Toeplitz maps (rigid-body-system.cpp:377-452), i = row (instant), j = column
WG_TT_INLINE double tt_uv(unsigned i, unsigned j, double T) { return j <= i ? (2 * (i - j) + 1) * T * T * 0.5 : 0.0; }
WG_TT_INLINE double tt_uz(unsigned i, unsigned j, double T, double h) {
  return j <= i ? (1 + 3 * (i - j) + 3 * (i - j) * (i - j)) * T * T * T / 6.0 - T * h / 9.81 : 0.0;
}

// The tables of model m into t, every element of every array (zeros behind the parts N uses); ql_sums is stored as given.
// qb_override (N x N, row-major; host only) replaces the loop's Q_b: the matrix-core Gramian of wg_gramian_batch
// (WG_FLAG_GRAMIAN_MFMA_*); everything derived from Q_b (factor blocks, diagonal test) then follows the override.
// m.N must be in 2 .. kNMaxH.  t may be global memory that nothing has written yet: it is only written, in the last phase.
template <class X>
WG_TT_HD inline void tt_build(const X x, const wg_model_t &m, TtWork &W, TickTables &t, int ql_sums, const double *qb_override = nullptr) {
  const int N = m.N, M = 2 * N;
  const double T = m.T, h = m.com_height_qp;
  const double alpha = m.alpha, beta = m.beta, gamma = m.gamma;
  const int l0 = x.lane(), S = x.lanes();
  const double vsmall = 1e-8;

  // ---- Q_b = beta I + alpha Uv'Uv + gamma Uz'Uz, generator-vel-ref.cpp:587-614 ----
  for (int e = l0; e < N * N; e += S) {
    const int i = e / N, j = e - i * N;
    double pj = 0.0, pv = 0.0, pz = 0.0;
    for (int k = 0; k < N; k++) {
      pj += ((k == i) ? 1.0 : 0.0) * ((k == j) ? 1.0 : 0.0);
      pv += tt_uv(k, i, T) * tt_uv(k, j, T);
      pz += tt_uz(k, i, T, h) * tt_uz(k, j, T, h);
    }
    double q = 0.0;
    q += pj * beta;
    q += pv * alpha;
    q += pz * gamma;
    W.Qb[e] = qb_override ? qb_override[e] : q;
  }
  x.sync();
  // ---- constant factor blocks: exactly ql0002's recurrences on blockdiag(Qb, Qb), eps = 1e-8 ----
  auto g2 = [&](int i, int j) -> double {
    if (i < N && j < N) return W.Qb[i * N + j];
    if (i >= N && j >= N) return W.Qb[(i - N) * N + (j - N)];
    return 0.0;
  };
  {
    double dl = 0.0;
    for (int i = l0; i < M; i += S) {
      const double wdi = g2(i, i);
      dl = (dl >= vsmall - wdi) ? dl : vsmall - wdi;
      for (int j = i + 1; j < M; ++j) {
        const double gjj = g2(j, j), gij = g2(i, j);
        double ga = -((wdi <= gjj) ? wdi : gjj);
        const double gb = fabs(wdi - gjj) + fabs(gij);
        if (gb > 0.0) ga += gij * gij / gb;
        dl = (dl >= ga) ? dl : ga;
      }
    }
    if (l0 < 64) W.part[l0] = dl;
  }
  x.sync();
  double diag = 0.0;
  for (int l = 0; l < S && l < 64; ++l) diag = (diag >= W.part[l]) ? diag : W.part[l];
  bool ok = diag <= 0.0;
  auto R = [&](int i, int j) -> double & { return W.R2[(size_t)j * (j + 1) / 2 + i]; };
  auto Z = [&](int i, int j) -> double & { return W.Z2[(size_t)i + (size_t)j * M]; };
  // ---- the factor, row by row: every lane computes the diagonal entry (so the exit is uniform), a column j > i per lane ----
  for (int i = 0; i < M && ok; ++i) {
    double temp = g2(i, i);
    for (int k = 0; k < i; ++k) temp -= R(k, i) * R(k, i);
    if (temp < vsmall) { ok = false; break; }
    const double rii = sqrt(temp);
    if (l0 == 0) R(i, i) = rii;
    for (int j = i + 1 + l0; j < M; j += S) {
      double tq = g2(i, j);
      for (int k = 0; k < i; ++k) tq -= R(k, j) * R(k, i);
      R(i, j) = tq / rii;
    }
    x.sync();
  }
  // ---- its inverse: a row reads the factor and its own entries to the left ----
  if (ok)
    for (int i = l0; i < M; i += S) {
      for (int j = 0; j < i; ++j) Z(i, j) = 0.0;
      Z(i, i) = 1.0 / R(i, i);
      for (int j = i; j < M - 1; ++j) {
        double sum = 0.0;
        for (int k = i; k <= j; ++k) sum += Z(i, k) * R(k, j + 1);
        Z(i, j + 1) = -sum / R(j + 1, j + 1);
      }
    }
  x.sync();

  // ---- the tables: every element of every array once, zero behind the used part (and throughout R2 / Z2 / the sign words
  // when the factor failed) ----
  for (int e = l0; e < kNMaxH * 3; e += S) {
    const unsigned i = (unsigned)(e / 3);
    const int c = e - 3 * (int)i;
    double sv = 0.0, sz = 0.0;
    if ((int)i < N) {
      sv = c == 0 ? 0.0 : (c == 1 ? 1.0 : (i + 1) * T);
      sz = c == 0 ? 1.0 : (c == 1 ? (i + 1) * T : (i + 1) * (i + 1) * T * T * 0.5 - h / 9.81);
    }
    (&t.Sv[0][0])[e] = sv; (&t.Sz[0][0])[e] = sz;
  }
  for (int e = l0; e < kNMaxH * kNMaxH; e += S) {
    const int i = e / kNMaxH, j = e - i * kNMaxH;
    const bool in = i < N && j < N;
    (&t.Uv[0][0])[e] = in ? tt_uv(i, j, T) : 0.0;
    (&t.Uz[0][0])[e] = in ? tt_uz(i, j, T, h) : 0.0;
    (&t.Qb[0][0])[e] = in ? W.Qb[i * N + j] : 0.0;
  }
  const int nr = M * (M + 1) / 2;
  for (int e = l0; e < 2 * kNMaxH * (2 * kNMaxH + 1) / 2; e += S) t.R2[e] = (ok && e < nr) ? W.R2[e] : 0.0;
  for (int e = l0; e < 4 * kNMaxH * kNMaxH; e += S) t.Z2[e] = (ok && e < M * M) ? W.Z2[e] : 0.0;
  for (int w = l0; w < (kNMaxH * kNMaxH + 63) / 64; w += S) {
    unsigned long long bits = 0ull;
    if (ok)
      for (int b = 0; b < 64; ++b) {
        const int e = w * 64 + b;
        if (e >= N * N) break;
        const int i = e % N, j = e / N;
        if (__builtin_signbit(Z(i, N + j))) bits |= 1ull << b;
      }
    t.z2_cross_sign[w] = bits;
  }
  if (l0 == 0) { t.diag_b = diag; t.blocks_ok = ok ? 1 : 0; t.ql_sums = ql_sums; }
}

}  // namespace wg
