// wg_ql_view.hpp -- what a QL solve works on: the footprint of one QP (QlDims), the partition of a wave's LDS slice and its
// global slots into the solver's arrays (QlView and its carve_* layouts), the accessors of Z, G, A and R, the dense problem
// policies (DenseProbT, DenseRegProb) and the traits ql_solve asks a policy for, the result and resume records, and the
// instrumentation macros of the attribution builds (WG_REP / WG_SINK); those of the profile build are wg_prof.hpp's.
//
// Hessian G, Z (= R^-1, later rotated), packed R, the constraint matrix A and all vectors live in the wave's LDS slice unless
// the layout says otherwise; leading dimensions are odd so that both row and column sweeps are bank-conflict free for 8-byte
// accesses.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wg_wave.hpp"
#include "wg_prof.hpp"

namespace wg {

// LDS footprint of one QP (in doubles, then ints).  Host and device agree on it.
struct QlDims {
  int n, m, mmax;
  int ldg, ldz, lda;
  bool dense;   // G and A held as LDS matrices (false: the problem view regenerates them)
  bool a_lds;   // dense only: A staged in LDS (false: read in place from global memory -- large QPs)
  int nsc;      // length of each of the four scratch vectors: n, or the static length of the compact view's ordered sums
  bool bounds;  // xl / xu held in LDS (false: the problem view supplies them -- constants for the Herdt QP)
  bool z_lds;   // Z held in LDS (false: the caller points QlView::Z at a per-problem slot in global memory -- large n, where
                // Z is the operand that caps the residency; it is streamed lane-parallel, never on a serial chain)
  bool wab_lds; // wa and b held in LDS (false: in a per-block slot of global memory -- they are read lane-parallel once per
                // iteration, early enough for an L2 round trip to hide; freeing them is what lets an eighth gait onto the CU)
  bool cold_lds; // d, wd, wx held in LDS (false: in the global slot too -- the gradient, the saved diagonal and the saved
                 // iterate are read lane-parallel, d once per iteration, the others a few times per solve)
  int r_cols;    // > 0: the LDS holds only the first r_cols columns of R plus one working column (QlView::nact_cap): a solve
                 // whose active set would grow past r_cols stops with kQlCapHit and is repeated with R in global memory
  bool g_lds;    // dense only: G staged in LDS (false: read in place from global memory, only its diagonal -- the one part ql0002
                 // writes, :814-854 -- is kept in LDS.  G is cold once Z = R^-1 exists: the residual refresh and the
                 // objective-increase test read it a few times per solve)
  __host__ __device__ QlDims(int n_, int m_, int mmax_, bool dense_ = true, bool a_lds_ = true, int nsc_ = 0,
                             bool bounds_ = true, bool z_lds_ = true, bool wab_lds_ = true, bool cold_lds_ = true, int r_cols_ = 0,
                             bool g_lds_ = true)
      : n(n_), m(m_), mmax(mmax_), ldg(n_ | 1), ldz(n_ | 1), lda(mmax_ | 1), dense(dense_), a_lds(a_lds_),
        nsc(nsc_ > n_ ? nsc_ : n_), bounds(bounds_), z_lds(z_lds_), wab_lds(wab_lds_), cold_lds(cold_lds_),
        r_cols(r_cols_ > 0 && r_cols_ < n_ ? r_cols_ : 0), g_lds(g_lds_) {}
  __host__ __device__ int r_tail() const { return r_cols ? r_cols * (r_cols + 1) / 2 : n * (n + 1) / 2; }
  __host__ __device__ int r_len() const { return r_tail() + n; }
  __host__ __device__ int n_doubles() const {
    return (dense ? (g_lds ? n * ldg : n) + (a_lds ? n * lda : 0) : 0) + (z_lds ? n * ldz : 0) + r_len()   // [G | diag(G), A,] [Z,] R
           + ((bounds ? 8 : 6) - (cold_lds ? 0 : 3)) * n   // x [d] ww [wd wx] lam [xl xu]
           + (wab_lds ? (m + n) + m : 0)            // wa, b (inner)
           + 4 * nsc + 8;                           // scratch + scalar slots
  }
  __host__ __device__ size_t bytes() const {
    return (size_t)n_doubles() * 8 + (size_t)((n + 1) & ~1) * 4;
  }
};

constexpr int kQlCapHit = -7777;                          // QlResult::ifail of a solve stopped by QlView::nact_cap
struct QlView {
  int n, m, me, mn, ldg, ldz, lda;
  int r_tail = 0;                                          // offset of the n scratch entries behind R's columns
  int nact_cap = 0;                                        // > 0: stop (kQlCapHit) when the active set would exceed it
  double *G, *Z, *R, *A;
  double *Gdiag = nullptr;                                 // dense view with G read in place: the diagonal's LDS copy
  double *Rf;                                              // where the Cholesky factor of G is formed on the way to Z = R^-1 (dead
                                                           // afterwards): R itself, or a full-size array when R is capped
  double *x, *d, *ww, *wd, *wx, *lam, *xl, *xu, *wa, *b;
  double *sc0, *sc1, *sc2, *sc3, *slot;
  int *iact;
  // kBounds / kWabLds mirror QlDims::bounds / wab_lds at compile time (a run-time choice between an LDS and a global array
  // would make the pointer generic and every access through it a flat_ instruction); ext_wab: [wa (mmax + nmax) | b (mmax)]
  // kColdLds mirrors QlDims::cold_lds: false puts d | wd | wx at ext_cold, ext_cold_ld doubles apart
  template <bool kBounds = true, bool kWabLds = true, bool kColdLds = true>
  __device__ __forceinline__ void carve(double *base, const QlDims &D, int me_, double *ext_wab = nullptr, int ext_b_off = 0,
                                        double *ext_cold = nullptr, int ext_cold_ld = 0) {
    n = D.n; m = D.m; me = me_; mn = D.m + D.n; ldg = D.ldg; ldz = D.ldz; lda = D.lda;
    r_tail = D.r_tail(); nact_cap = D.r_cols;
    double *p = base;
    G = nullptr; A = nullptr;
    if (D.dense) {
      if (D.g_lds) { G = p; p += n * ldg; }
      else { Gdiag = p; p += n; }                          // the caller points G (and ldg) at the problem's own array
    }
    Z = nullptr;
    if (D.z_lds) { Z = p; p += n * ldz; }
    R = p; p += D.r_len(); Rf = R;
    if (D.dense && D.a_lds) { A = p; p += n * lda; }
    if constexpr (kColdLds) { x = p; p += n;  d = p; p += n;  ww = p; p += n;  wd = p; p += n;  wx = p; p += n; lam = p; p += n; }
    else {
      // lean layout (element view): the four scratch vectors come right behind R -- like R they are dead outside the solve, so the
      // tick's pre-solve overlay may run over both (the smaller R's LDS part, the more gaits fit a CU) -- and x, which must
      // survive the solve, after them
      sc0 = p; p += D.nsc; sc1 = p; p += D.nsc; sc2 = p; p += D.nsc; sc3 = p; p += D.nsc;
      x = p; p += n; ww = p; p += n; lam = p; p += n; d = ext_cold; wd = ext_cold + ext_cold_ld; wx = ext_cold + 2 * ext_cold_ld;
    }
    if constexpr (kBounds) { xl = p; p += n; xu = p; p += n; } else { xl = nullptr; xu = nullptr; }
    if constexpr (kWabLds) { wa = p; p += m + n; b = p; p += m; } else { wa = ext_wab; b = ext_wab + ext_b_off; }
    if constexpr (kColdLds) { sc0 = p; p += D.nsc; sc1 = p; p += D.nsc; sc2 = p; p += D.nsc; sc3 = p; p += D.nsc; }
    slot = p; p += 8;
    iact = reinterpret_cast<int *>(p);
  }
  // Same partition laid out for the compile-time maxima (NMAX, MMAX), whatever the actual n, m: every array then sits at
  // a constant offset from the wave's LDS base (immediate offsets in the ds instructions, no address registers), and Z's
  // leading dimension is the constant NMAX|1.  No G / A matrices (compact views only).
  template <int NMAX, int MMAX, int NSC, bool kExt = false>   // kExt: wa / b live in ext_wab (global memory), known at compile time
  __device__ void carve_fixed(double *base, int n_, int m_, int me_, double *ext_wab = nullptr) {
    n = n_; m = m_; me = me_; mn = m_ + n_; ldg = NMAX | 1; ldz = NMAX | 1; lda = MMAX | 1;
    r_tail = n_ * (n_ + 1) / 2; nact_cap = 0;
    double *p = base;
    G = nullptr; A = nullptr;
    Z = p; p += NMAX * (NMAX | 1);
    R = p; p += NMAX * (NMAX + 1) / 2 + NMAX; Rf = R;
    x = p; p += NMAX;  d = p; p += NMAX;  ww = p; p += NMAX;  wd = p; p += NMAX;
    wx = p; p += NMAX; lam = p; p += NMAX; xl = nullptr; xu = nullptr;     // bounds come from the problem view
    if constexpr (kExt) { wa = ext_wab; b = ext_wab + (MMAX + NMAX); }
    else { wa = p; p += MMAX + NMAX; b = p; p += MMAX; }
    sc0 = p; p += NSC; sc1 = p; p += NSC; sc2 = p; p += NSC; sc3 = p; p += NSC;
    slot = p; p += 8;
    iact = reinterpret_cast<int *>(p);
  }
  // Element view with the horizon known at compile time (NMAX = 2N + 2 kSMax, MMAX = 1 + 4N + 5 kSMax): the lean partition of
  // carve<false, false, false> laid out for the model's LARGEST problem whatever n and m the tick has, so that every LDS array
  // sits at a constant offset from the wave's base (immediates in the ds instructions instead of address registers) and Z's
  // leading dimension is the constant NMAX:   x | ww | lam | slot | iact | sc0 sc1 sc2 sc3 | R.
  // R comes last: its length -- r_cols columns and one working column, or all n -- is the one thing the column cap decides.  The
  // tick's pre-solve overlay lies over sc0 .. R (dead outside the solve).  Z, wa | b and d | wd | wx live in the per-block global
  // slot (the caller passes them: constants behind one base).  Same bytes as QlDims(NMAX, MMAX, ...).bytes().
  template <int NMAX, int MMAX>
  __device__ __forceinline__ void carve_fixed_elem(double *base, int n_, int m_, int me_, int r_cols, double *z_ext, double *wa_ext,
                                                    double *b_ext, double *d_ext, double *wd_ext, double *wx_ext, double *rf_ext) {
    n = n_; m = m_; me = me_; mn = m_ + n_; ldg = NMAX | 1; ldz = NMAX; lda = MMAX | 1;   // Z is global here: whole cache lines per column
    const bool capped = r_cols > 0 && r_cols < n_;
    nact_cap = capped ? r_cols : 0;
    r_tail = capped ? r_cols * (r_cols + 1) / 2 : n_ * (n_ + 1) / 2;
    G = nullptr; A = nullptr; xl = nullptr; xu = nullptr;
    double *p = base;
    x = p; p += NMAX; ww = p; p += NMAX; lam = p; p += NMAX;
    slot = p; p += 8;
    iact = reinterpret_cast<int *>(p); p += ((NMAX + 1) & ~1) / 2;
    sc0 = p; p += NMAX; sc1 = p; p += NMAX; sc2 = p; p += NMAX; sc3 = p; p += NMAX;
    R = p;
    Z = z_ext; wa = wa_ext; b = b_ext; d = d_ext; wd = wd_ext; wx = wx_ext; Rf = rf_ext;
  }
  // The dense ql0001_ boundary at a size known at compile time (the Herdt QP: NMAX = 36, MMAX = 76): G and A are read in place
  // (the caller points G / A at the problem's own arrays, leading dimensions NMAX / MMAX), wa | b live in the block's global
  // slot; Z, R and the vectors sit at constant LDS offsets:  Z | R | x d ww wd wx lam | xl xu | diag(G) | sc0..sc3 | slot | iact
  template <int NMAX, int MMAX>
  __device__ __forceinline__ void carve_fixed_dense(double *base, int n_, int m_, int me_, double *ext_wab) {
    n = n_; m = m_; me = me_; mn = m_ + n_; ldg = NMAX; ldz = NMAX | 1; lda = MMAX;
    r_tail = n_ * (n_ + 1) / 2; nact_cap = 0;
    double *p = base;
    Z = p; p += NMAX * (NMAX | 1);
    R = p; p += NMAX * (NMAX + 1) / 2 + NMAX; Rf = R;
    x = p; p += NMAX; d = p; p += NMAX; ww = p; p += NMAX; wd = p; p += NMAX; wx = p; p += NMAX; lam = p; p += NMAX;
    xl = p; p += NMAX; xu = p; p += NMAX;
    Gdiag = p; p += NMAX;
    wa = ext_wab; b = ext_wab + (MMAX + NMAX);
    sc0 = p; p += NMAX; sc1 = p; p += NMAX; sc2 = p; p += NMAX; sc3 = p; p += NMAX;
    slot = p; p += 8;
    iact = reinterpret_cast<int *>(p);
    G = nullptr; A = nullptr;
  }
  template <int NMAX> static constexpr size_t fixed_dense_bytes() {
    return 8 * (size_t)(NMAX * (NMAX | 1) + NMAX * (NMAX + 1) / 2 + NMAX + 9 * NMAX + 4 * NMAX + 8) + 4 * (size_t)((NMAX + 1) & ~1);
  }
  // doubles in front of sc0 in that layout (where the tick's overlay starts)
  template <int NMAX> static constexpr int fixed_elem_head() { return 3 * NMAX + 8 + ((NMAX + 1) & ~1) / 2; }
};

#define Zm(i, j) q.Z[(i) + (j) * q.ldz]
// G and A go through the problem view `prob` (DenseProb: LDS matrices; HerdtProb: regenerated on the fly)
#define Gm(i, j) prob.G(q, (i), (j))
#define Am(k, i) prob.A(q, (k), (i))

struct QlView;
template <bool kGLds, int kNMc = 0>         // where G lives is known at compile time (ds_ or global_ accesses, never flat_)
struct DenseProbT {
  static constexpr bool kCompact = false;
  static constexpr bool kNanExact = true;   // the ql0001_ boundary takes anybody's QP: NaN iterates end the way the reference ends them (scan_nan_exact)
  static constexpr bool kHasFactor = false;    // no structure to exploit: ql0002's own Cholesky and inverse
  static constexpr bool kRowOps = false;   // no structured row products: rows are read element by element
  static constexpr int kNM = kNMc;     // 0: no compile-time bound on n; > 0: n <= kNM (the Herdt-sized boundary kernel: the
                                       // compile-time-bounded forms of the sweep, the back substitution and the ordered sums)
  static constexpr bool kWideN = false;  // 64 <= n <= 128 is not known at compile time: the wide (two rows / columns per lane) forms by test
  static constexpr int kFixedLdz = kNMc > 0 ? (kNMc | 1) : 0;   // > 0: Z in LDS with this leading dimension (carve_fixed_dense)
  __device__ __forceinline__ double G(const QlView &q, int i, int j) const;
  __device__ __forceinline__ double A(const QlView &q, int k, int i) const;
  __device__ __forceinline__ double Gd(const QlView &q, int i) const;
  __device__ __forceinline__ void setGd(const QlView &q, int i, double v) const;
  __device__ __forceinline__ double xl(const QlView &q, int i) const;
  __device__ __forceinline__ double xu(const QlView &q, int i) const;
};
typedef DenseProbT<true> DenseProb;
// The dense boundary at a size known at compile time (n <= NM, m <= MM <= 128) with the constraint matrix kept as REGISTER ROWS:
// lane k carries row k (ar0) and row 64 + k (ar1) of A, loaded once per QP -- the violation scan, which walks every row in every
// iteration, then reads no memory but x (LDS broadcasts); the new normal is written out by the lane that owns the row.  Every
// other access to A (once per solve, or in the residual refresh) still reads it in place.
template <int NM, int MM>
struct DenseRegProb : DenseProbT<false, NM> {
  static constexpr bool kRegRows = true;
  double ar0[NM], ar1[NM];
  __device__ __forceinline__ void load_rows(const QlView &q, int lane) {
    const int m = q.m;
    const int mc = m > 0 ? m - 1 : 0;          // a bounds-only QP (m == 0) must not read row -1: row 0 of the caller's buffer exists (mmax >= 1)
    const int k0 = lane < m ? lane : mc, k1 = lane + 64 < m ? lane + 64 : mc;
#pragma unroll
    for (int i = 0; i < NM; ++i) { ar0[i] = q.A[k0 + i * q.lda]; ar1[i] = q.A[k1 + i * q.lda]; }
  }
  // ww[i] = A(k, i), i < n: the owner of row k writes it (compile-time column indices: the rows stay in registers)
  __device__ __forceinline__ void row_to(const QlView &q, int k, double *dst, int lane) const {
    const int n = q.n;
    if (lane == (k & 63)) {
#pragma unroll
      for (int i = 0; i < NM; ++i)
        if (i < n) dst[i] = k < 64 ? ar0[i] : ar1[i];
    }
  }
};
template <class P, class = void> struct HasRegRows { static constexpr bool value = false; };
template <class P> struct HasRegRows<P, typename std::enable_if<P::kRegRows>::type> { static constexpr bool value = true; };
#define Rp(i, j) q.R[(j) * ((j) + 1) / 2 + (i)]
#define Rf(i, j) q.Rf[(j) * ((j) + 1) / 2 + (i)]        // the same packing, in the factorisation's array

// ---- attribution builds (never shipped): -DWG_REPEAT_PHASE=k executes the idempotent phase k of every active-set iteration
// TWICE (same results: each of these phases only reads the solver state it does not write); the difference of the hardware
// counters against the plain build is that phase's share (tools/phase_attribution.sh).  The memory clobber makes the second
// pass reload its operands instead of being folded into the first.
#ifdef WG_REPEAT_PHASE
#define WG_REP(id) for (int wg_rep_ = 0; wg_rep_ < (((WG_REPEAT_PHASE) == (id)) ? 2 : 1); ++wg_rep_, ({ asm volatile("" ::: "memory"); }))
// a phase whose results live in registers only would lose its first pass to dead-code elimination: the sink "uses" them
#define WG_SINK(x) asm volatile("" ::"v"(x))
#else
#define WG_REP(id)
#define WG_SINK(x) do {} while (0)
#endif

// per-lane parameters of the active constraints, for problem views that supply a fast residual refresh
struct NoActiveParams {};
template <class P, class = void> struct ActiveParamsOf { typedef NoActiveParams type; };
template <class P> struct ActiveParamsOf<P, typename std::enable_if<P::kCompact>::type> { typedef typename P::ActiveParams type; };

// decision-only sums under certificates (wg_ql_guard.hpp): a policy that declares kGuardedSums carries `sums_mode`
// (kSumsGuarded / kSumsOrdered / kSumsDoubt); every other policy keeps the reference's order and compiles none of it
template <class P, class = void> struct GuardedSumsOf { static constexpr bool value = false; };
template <class P> struct GuardedSumsOf<P, typename std::enable_if<P::kGuardedSums>::type> { static constexpr bool value = true; };
enum : int { kSumsGuarded = 0, kSumsOrdered = 1, kSumsDoubt = 2, kSumsMask = 3 };
// the sweep's norm chain from seeds, checked once (wg_ql_norms.hpp): a policy that declares kSeededNorms (it carries
// `sums_mode` as well) keeps the mode in bits 8 - 9 of that word -- kNormsSeeded / kNormsExact (the exact chain throughout) /
// kNormsDoubt (tests: the check reports a mismatch in every sweep); every other policy compiles none of it
template <class P, class = void> struct SeededNormsOf { static constexpr bool value = false; };
template <class P> struct SeededNormsOf<P, typename std::enable_if<P::kSeededNorms>::type> { static constexpr bool value = true; };
enum : int { kNormsSeeded = 0, kNormsExact = 1 << 8, kNormsDoubt = 2 << 8, kNormsMask = 3 << 8 };
// the back substitution's bottom rows at their own lengths (bs_row's kExact, wg_ql_phases.hpp): a policy that declares
// kExactBacksub; every other policy keeps the rounded-up heads
template <class P, class = void> struct ExactBacksubOf { static constexpr bool value = false; };
template <class P> struct ExactBacksubOf<P, typename std::enable_if<P::kExactBacksub>::type> { static constexpr bool value = true; };
constexpr int kQlDoubt = -7778;                            // QlResult::ifail of a guarded solve that must be run again (ql_solve_guarded)

struct QlResult {
  int ifail, n_iter, nact, hist_len;
};
// The scalar state of ql0002's main loop between two iterations: what a solve stopped by QlView::nact_cap (kQlCapHit) hands to
// its continuation.  The arrays (x, multipliers, active set, Z, R, wa) stay where they are; the caller moves R to its larger
// home, clears the cap and calls ql_solve again with `valid` set: the solve goes on where it stopped, same arithmetic.
struct QlResume {
  int valid = 0;
  int nact, info, iterc, itref, iflag, jfinc, knext, st, hist_len;
  double xmag, vfact, res, ratio, diag;
};

template <bool kGLds, int kNMc> __device__ __forceinline__ double DenseProbT<kGLds, kNMc>::G(const QlView &q, int i, int j) const {
  if constexpr (kGLds) return q.G[i + j * q.ldg];
  else {
    const double g = q.G[i + j * q.ldg], dg = q.Gdiag[i];  // both requested: the select costs no round trip
    return i == j ? dg : g;
  }
}
template <bool kGLds, int kNMc> __device__ __forceinline__ double DenseProbT<kGLds, kNMc>::A(const QlView &q, int k, int i) const { return q.A[k + i * q.lda]; }
template <bool kGLds, int kNMc> __device__ __forceinline__ double DenseProbT<kGLds, kNMc>::Gd(const QlView &q, int i) const {
  if constexpr (kGLds) return q.G[i + i * q.ldg]; else return q.Gdiag[i];
}
template <bool kGLds, int kNMc> __device__ __forceinline__ void DenseProbT<kGLds, kNMc>::setGd(const QlView &q, int i, double v) const {
  if constexpr (kGLds) q.G[i + i * q.ldg] = v; else q.Gdiag[i] = v;
}
template <bool kGLds, int kNMc> __device__ __forceinline__ double DenseProbT<kGLds, kNMc>::xl(const QlView &q, int i) const { return q.xl[i]; }
template <bool kGLds, int kNMc> __device__ __forceinline__ double DenseProbT<kGLds, kNMc>::xu(const QlView &q, int i) const { return q.xu[i]; }

}  // namespace wg
