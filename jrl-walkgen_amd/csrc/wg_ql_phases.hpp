// wg_ql_phases.hpp -- the phases of one active-set iteration of the QL solver (wg_ql_device.hpp: ql_solve), each in the forms
// the problem views need: rotation norms, the products with Z (zt_times_ww*, z_rows_times), back substitution (backsub,
// backsub_lds), ordered sums, the Givens sweeps (sweep_flat, sweep), the NaN-exact violation scan, the ratio test (pick_drop*),
// xmag_sum, the deletion of a constraint, the linear-independence test, and the register Cholesky / inverse of the set-up.
// Line numbers (qld.cpp:...) are those of ql0002_ in the reference's src/Mathematics/qld.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wg_wave.hpp"
#include "wg_ql_view.hpp"

namespace wg {

// Prefetch group size of the wide (64 < n <= 128) forms: entries of Z requested together ahead of the add chains / rotations.
// Eight is what a 256-register kernel carries (the dense boundary kernel); the element view is compiled for 168 registers --
// three waves per SIMD -- and takes groups of four: measured 7 % slower per wave and, with twelve gaits on a CU instead of eight,
// 7 % faster overall.
#ifndef WG_ELEM_GRP
#define WG_ELEM_GRP 4
#endif

// norm of a rotation, qld.cpp:1921-1926 / 2005-2010:  t = max(|p|,|q|);  t * sqrt((p/t)^2 + (q/t)^2).
// This sits on the sequential chain of every sweep.  One of the two quotients is x/|x| = +-1 EXACTLY (IEEE division is
// exact there), its square is exactly 1.0, and a + b == b + a: so only the other quotient is a real division.  Same
// bits as the reference's two divisions for finite operands (0/0 stays NaN); half the divide latency on the chain.
// sqrt(x) for 1 <= x <= 2: the compiler's own correctly-rounded f64 expansion (v_rsq_f64 + two coupled Newton steps,
// same operations in the same order) without its range scaling (ldexp in, ldexp out) and special-value select, which
// are exact no-ops on this interval.  Five dependent instructions shorter; bit-identical result.
__device__ __forceinline__ double sqrt_1to2(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y;
  double h = y * 0.5;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  double d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  d = __builtin_fma(-g, g, x);
  g = __builtin_fma(d, h, g);
  return g;
}
__device__ __forceinline__ double givens_norm(double p, double qq) {
  const double ap = fabs(p), aq = fabs(qq);
  const bool pbig = ap >= aq;                      // maxd(): a >= b ? a : b
  // the value of the select (finite operands) in one instruction; __builtin_fmax would first canonicalise both operands
  // (two more v_max_f64) -- NaN operands give NaN either way, and that result is discarded wherever it can arise
  double t;
  asm("v_max_f64 %0, |%1|, |%2|" : "=v"(t) : "v"(p), "v"(qq));
  const double d = (pbig ? qq : p) / t;            // |d| <= 1
  const double x = 1.0 + d * d;
  return t * sqrt_1to2(x);                         // x is in [1, 2], or NaN (which stays NaN)
}
// The same norm for operands whose non-zero magnitudes lie in [2^-400, 2^404] (sweep_range_ok), five instructions shorter:
//   * min / max of the magnitudes in one instruction each: the quotient enters only through its square, and
//     (|x| / |y|)^2 == (x / y)^2 bit for bit;
//   * the division is the compiler's own f64 expansion (v_rcp_f64, two Newton steps, quotient, residual, correction) without
//     v_div_scale_f64 / v_div_fixup_f64: with 0 <= a <= t and t in that range both scalings are the identity and the fix-up
//     passes the quotient through whenever it is >= 2^-27; below that d * d < 2^-54 and 1 + d * d is exactly 1 whatever the
//     last bits of d.  t == 0 (both operands zero) gives NaN here as 0/0 does there: the caller discards it.
__device__ __forceinline__ double givens_norm_fast(double p, double qq) {
  double t, a;
  asm("v_max_f64 %0, |%1|, |%2|" : "=v"(t) : "v"(p), "v"(qq));
  asm("v_min_f64 %0, |%1|, |%2|" : "=v"(a) : "v"(p), "v"(qq));
  double r = __builtin_amdgcn_rcp(t);
  double e = __builtin_fma(-t, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-t, r, 1.0);
  r = __builtin_fma(r, e, r);
  const double q0 = a * r;
  const double rem = __builtin_fma(-t, q0, a);
  const double d = __builtin_fma(rem, r, q0);
  const double x = 1.0 + d * d;
  return t * sqrt_1to2(x);
}
}  // namespace wg
// the same chain from seeds made ahead of it and checked once against givens_norm_fast: one text for host and device
#define WG_NORMS_FN __device__ __forceinline__
#define WG_NORMS_RSQ(x) __builtin_amdgcn_rsq(x)
#define WG_NORMS_EXACT(p, q) ::wg::givens_norm_fast(p, q)
#include "wg_ql_norms.hpp"
namespace wg {
// every entry of s[lo, hi) is zero or has its magnitude in [2^-400, 2^400] (then every norm of a sweep over them, being at
// least its larger operand and at most sqrt(n) times the largest entry, is zero or in [2^-400, 2^404]); wave-uniform
template <bool kOnePass = false>                          // kOnePass: hi - lo <= 64 (the caller's n <= 64)
__device__ __forceinline__ bool sweep_range_ok(const double *s, int lo, int hi, int lane) {
  if constexpr (kOnePass) {                                 // one entry per lane: no lane-dependent loop, no exec-mask juggling
    const int j = lo + lane;
    const bool in = j < hi;
    const double v = fabs(s[in ? j : lo]);
    return __ballot(in && !(v == 0.0 || (v >= 0x1p-400 && v <= 0x1p400))) == 0ull;
  }
  bool bad = false;
  for (int j = lo + lane; j < hi; j += 64) {
    const double v = fabs(s[j]);
    bad = bad || !(v == 0.0 || (v >= 0x1p-400 && v <= 0x1p400));
  }
  return __ballot(bad) == 0ull;
}
// qld.cpp:1921-1930 / 2005-2014
__device__ __forceinline__ void givens(double p, double qq, double &ga, double &gb, double &nrm) {
  const double sum = givens_norm(p, qq);
  ga = p / sum;
  gb = qq / sum;
  nrm = sum;
}
__device__ __forceinline__ bool significant(double base, double delta_abs) {
  double temp = base + delta_abs * wg_kconst(.1);
  double tempa = base + delta_abs * wg_kconst(.2);
  if (temp <= base) return false;
  if (tempa <= temp) return false;
  return true;
}

// s[i] = sum_j Z(j,i) * ww[j]   (qld.cpp:2071-2085); lane i owns s[i]
template <int NM = 0, int GRP = 8, bool kWide = false>   // NM > 0: n <= NM known at compile time (the wide form is left out)
__device__ __forceinline__ void zt_times_ww(const QlView &q, double *s, int lane) {   // kWide: 64 <= n <= 128 known at compile time
  const int n = q.n;
  if (kWide || ((NM == 0 || NM > 64) && n > 64 && n <= 128)) {
    // two columns per lane in ONE pass (the second pass of the strided form has n - 64 useful lanes), loads in groups of
    // eight ahead of the two add chains: at this size Z may live in global memory (L2), where every exposed round trip
    // costs hundreds of cycles
    // surplus lanes all shadow column 0: one address per load instruction (it coalesces to a single request on a line lane 0 has
    // just fetched) instead of 56 more scattered ones -- the column walk is bound by the address path, not by the bytes
    const int i0 = lane, i1 = lane + 64 < n ? lane + 64 : 0;
    const double *z0 = q.Z + (size_t)i0 * q.ldz, *z1 = q.Z + (size_t)i1 * q.ldz;
    double a0 = 0.0, a1 = 0.0;
    int j = 0;
    for (; j + GRP <= n; j += GRP) {
      double u0[GRP], u1[GRP], w[GRP];
      // (z0 + j) + e, two pointer steps: as an index the sum j + e is formed in int first, and the kernels' registers are allotted differently
#pragma unroll
      for (int e = 0; e < GRP; ++e) { u0[e] = *(z0 + j + e); u1[e] = *(z1 + j + e); w[e] = q.ww[j + e]; }
#pragma unroll
      for (int e = 0; e < GRP; ++e) { a0 += u0[e] * w[e]; a1 += u1[e] * w[e]; }
    }
    for (; j < n; ++j) { const double w = q.ww[j]; a0 += z0[j] * w; a1 += z1[j] * w; }
    s[i0] = a0;
    if (lane + 64 < n) s[i1] = a1;
    WG_WSYNC();
    return;
  }
  for (int i = lane; i < n; i += 64) {
    double acc = 0.0;
    WG_UNROLL
    for (int j = 0; j < n; ++j) acc += Zm(j, i) * q.ww[j];
    s[i] = acc;
  }
  WG_WSYNC();
}

// The same product for the fixed N = 32 view (Z global, leading dimension NH * 2 + 8 = 72) and a constraint normal whose entries
// are known to be exact zeros outside the row ranges [0, r], [NH, NH + r] and [2 NH, n) (a CoP row of instant r of the Herdt QP;
// r = -1: a foot-placement row, nothing in the jerk columns): the rows of Z in between are not read.  Their products are +-0.0 and
// the sums -- started from +0.0, never -0.0 -- do not change when they are left out: the same bits for 2 (NH - 1 - r) / n fewer
// bytes of Z, on average 46 % of the walk at NH = 32, which is what this kernel is bound by (Z lives in global memory).
// FOUR lanes per column: lane L owns column 16 p + L / 4 in pass p and the two rows j0 + 2 (L & 3), + 1 of every eight-row block
// -- the four lanes of a column read 64 contiguous bytes, so a load instruction touches 16 cache lines instead of 64 and an
// eight-row block of all 72 columns costs 80 line requests instead of 288 (the column walk is bound by its requests).
// The eight products of a block reach every lane of the quad by DPP (quad_perm broadcasts, no LDS) and are added in row order: the
// same adds in the same order as zt_times_ww's, less those of exact zeros (whole blocks: the rows of a block past the row's instant
// carry exact zeros; rows past n -- block 8 only -- are masked to +0.0, which never changes a sum that cannot be -0.0).
template <int K>
__device__ __forceinline__ double wg_quad_bcast(double v) {   // lane K of every quad to the whole quad
  constexpr int ctrl = K * 0x55;                              // quad_perm:[K,K,K,K]
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), ctrl, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), ctrl, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <int NH>
__device__ __forceinline__ void zt_times_ww_cop_tiled(const QlView &q, double *s, int lane, int r, bool tail) {
  constexpr int L = 2 * NH + 8;                               // q.ldz of carve_fixed_elem
  constexpr int NP = (L + 15) / 16;                           // passes of sixteen columns
  const int n = q.n;
  const int h = lane & 3, cq = lane >> 2;
  const double2 *zb[NP];
  bool colok[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int c = 16 * p + cq;
    colok[p] = c < n;
    zb[p] = reinterpret_cast<const double2 *>(q.Z + (size_t)(colok[p] ? c : 0) * L + 2 * h);   // lanes without a column: column 0
  }
  double acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = 0.0;
  struct Blk { double2 u[NP]; double w0, w1; };
  auto load = [&](Blk &B, int j0) {                           // rows j0 .. j0 + 7 (j0 a multiple of 8): requested, not waited for
#pragma unroll
    for (int p = 0; p < NP; ++p) B.u[p] = zb[p][j0 >> 1];
    B.w0 = q.ww[j0 + 2 * h]; B.w1 = q.ww[j0 + 2 * h + 1];
  };
  auto sum = [&](const Blk &B, bool last) {
    const int jr = 2 * NH + 2 * h;                            // the last block's rows (the only one that can reach past n)
    const bool ok0 = !last || jr < n, ok1 = !last || jr + 1 < n;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      double p0 = B.u[p].x * B.w0, p1 = B.u[p].y * B.w1;
      if (last) { p0 = ok0 ? p0 : 0.0; p1 = ok1 ? p1 : 0.0; }
      double a = acc[p];
      a += wg_quad_bcast<0>(p0); a += wg_quad_bcast<0>(p1);
      a += wg_quad_bcast<1>(p0); a += wg_quad_bcast<1>(p1);
      a += wg_quad_bcast<2>(p0); a += wg_quad_bcast<2>(p1);
      a += wg_quad_bcast<3>(p0); a += wg_quad_bcast<3>(p1);
      acc[p] = a;
    }
  };
  const int nb = (r >> 3) + 1;                                // blocks of each jerk range that carry entries (r = -1: none)
  // x blocks, y blocks, then the step columns' rows 2 NH .. n - 1 -- unless the normal has no entry there (a CoP row of an instant in
  // the current support phase: exact zeros, whose products leave the sums unchanged)
  const int total = 2 * nb + (tail ? 1 : 0);
  auto start = [&](int idx) { return idx < nb ? 8 * idx : (idx < 2 * nb ? NH + 8 * (idx - nb) : 2 * NH); };
  // the next block is requested before the current one is summed (two register sets taking turns)
  Blk A, B;
  load(A, start(0));
  for (int idx = 0;;) {
    if (idx + 1 >= total) { sum(A, tail); break; }
    load(B, start(idx + 1)); sum(A, false); ++idx;
    if (idx + 1 >= total) { sum(B, tail); break; }
    load(A, start(idx + 1)); sum(B, false); ++idx;
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
    if (h == 0 && colok[p]) s[16 * p + cq] = acc[p];
  WG_WSYNC();
}

// r0 = sum_{j0 <= j < j1} Z(i0, j) * s[j], r1 the same for row i1 (j ascending, from +0.0): rows i0 = lane and i1 = lane + 64
// of a matrix of 64 < n <= 128 rows in ONE pass, the entries of eight columns requested together ahead of the two add chains
// (with Z in global memory an exposed entry is an L2 round trip; one register set only: this sits where many values are live).
// Surplus lanes shadow a real row.
template <int GRP = 8>
__device__ __forceinline__ void z_rows_times(const QlView &q, const double *s, int j0, int j1, int lane, double &r0, double &r1) {
  const int n = q.n, ldz = q.ldz;
  // lanes without a second row all shadow row 64 (n > 64 here; one coalesced request per load instead of a second copy of the first set's)
  const int i0 = lane < n ? lane : n - 1, i1 = lane + 64 < n ? lane + 64 : (n > 64 ? 64 : i0);
  const double *z0 = q.Z + i0, *z1 = q.Z + i1;
  constexpr int kG = GRP;
  double a0 = 0.0, a1 = 0.0;
  int j = j0;
  for (; j + kG <= j1; j += kG) {
    double u0[kG], u1[kG], w[kG];
#pragma unroll
    for (int e = 0; e < kG; ++e) { u0[e] = z0[(j + e) * ldz]; u1[e] = z1[(j + e) * ldz]; w[e] = s[j + e]; }
#pragma unroll
    for (int e = 0; e < kG; ++e) { a0 += u0[e] * w[e]; a1 += u1[e] * w[e]; }
  }
  if (j < j1) {                                             // the odd columns: requested together (clamped), added in order
    double u0[kG - 1], u1[kG - 1];
#pragma unroll
    for (int e = 0; e < kG - 1; ++e) { const int jj = j + e < j1 ? j + e : j1 - 1; u0[e] = z0[jj * ldz]; u1[e] = z1[jj * ldz]; }
#pragma unroll
    for (int e = 0; e < kG - 1; ++e)
      if (j + e < j1) { const double w = s[j + e]; a0 += u0[e] * w; a1 += u1[e] * w; }
  }
  r0 = a0; r1 = a1;
}

// ww[0..nact) = R^-1 s[0..nact)   (qld.cpp:1824-1851): rows from the bottom up, inner sums ascending in j.
// nact <= 64: lane j keeps ww[j] in a register; row i's products R(i,j)*ww[j] are formed lane-parallel and
// summed in index order through v_readlane (no LDS round trip on the dependent chain).
__device__ __forceinline__ void backsub(const QlView &q, const double *s, int nact, int lane) {
  if (nact <= 60) {
    const bool mine = lane < nact;
    const double sreg = mine ? s[lane] : 0.0;
    const double dreg = mine ? Rp(lane, lane) : 1.0;
    double w = 0.0;
    double rrow = (nact >= 2 && lane == nact - 1) ? Rp(nact - 2, lane) : 0.0;   // R(i, lane) of the next row to do
    for (int i = nact - 1; i >= 0; --i) {
      double sum = 0.0;
      if (i < nact - 1) {
        const double p = (lane > i && mine) ? rrow * w : 0.0;
        sum = lane_sum_ordered(p, i + 1, nact);
      }
      const double v = (rl(sreg, i) - sum) / rl(dreg, i);
      if (lane == i) w = v;
      if (i >= 1) rrow = (lane > i - 1 && mine) ? Rp(i - 1, lane) : 0.0;          // prefetch row i-1
    }
    if (mine) q.ww[lane] = w;
    WG_WSYNC();
    return;
  }
  for (int i = nact - 1; i >= 0; --i) {
    double sum = 0.0;
    WG_UNROLL
    for (int j = i + 1; j < nact; ++j) sum += Rp(i, j) * q.ww[j];
    double v = (s[i] - sum) / Rp(i, i);
    if (lane == 0) q.ww[i] = v;
    WG_WSYNC();
  }
}

// Back substitution for n <= 36 (the compact view), restructured around its dependent chain.
// Row j needs sum_{k>j} R(j,k) w_k summed ascending in k, and its FIRST term carries the value produced last (w_{j+1}):
// the additions of a row are one chain, (nact-j-1) x 8 cycles plus the divide, and nothing else may sit on it.
//   * lane k keeps w_k and forms the products R(j-1,k) w_k for the NEXT row while the current row's chain runs; they
//     go to a double-buffered LDS vector (entries outside (j, nact) are written as +0.0: adding them changes nothing);
//   * every lane then runs the row's chain redundantly on LDS-broadcast operands, the first chunk prefetched one row
//     ahead, the first term formed in registers from R(j,j+1) and the w just computed.
// The v_readlane form above costs ~40 cycles per term (two readlanes + add, serialised); this one ~8.
// buf: 2 * kBsLen doubles of LDS (the four scratch vectors are contiguous).
// one row of backsub_lds: P = {terms k = j+2 .. j+9, R(j, j+1)} prefetched by the previous row, Nx receives the same for
// row j-1.  Two copies of this body with P / Nx swapped make the hand-over a renaming instead of nine register moves.
struct BsState { double w, wprev, rr, sreg, dreg, rsd; int col, nact, lane; bool mine; };   // rsd: R(lane, lane + 1), the first term's coefficient of row `lane`
// kHead: what is known about the row's length at compile time (the rows go from the bottom up, so the r-th row from the bottom has
// r terms): -1 nothing (three uniform branches per row), 0 no term, 4 / 8 at most so many (the prefetched head only: entries
// past the row are +0.0), 9 more than eight (head and tail loop, no test) -- backsub_lds unrolls the first nine rows that way
// kExact (the compact view): kHead = 0 .. 8 is the row's length itself.  The row adds its kHead terms and requests the kHead
// LDS-borne terms of the next row, nothing else: what the rounded-up heads add and read beyond the row are +0.0 entries, and a sum
// that starts from +0.0 is never -0.0, so x + (+0.0) is x bit for bit -- 20 dependent adds and 16 LDS reads per nine rows less
template <int kBsLen, int kHead = -1, bool kExact = false>  // kBsLen: length of each of the two product buffers (>= nact + 12)
__device__ __forceinline__ void bs_row(const QlView &q, double *buf, int j, BsState &S, const double (&P)[9], double (&Nx)[9]) {
  const double *bj = buf + (j & 1) * kBsLen;
  double *bn = buf + ((j & 1) ^ 1) * kBsLen;
  const int jn = j >= 1 ? j - 1 : 0, jnn = j >= 2 ? j - 2 : 0;
  const int nact = S.nact, lane = S.lane;
  // products of the next row (j-1) with the multipliers known so far (k >= j+1); nothing here waits on LDS: R(j-1, .)
  // was fetched one row ahead, and a wave's LDS operations execute in order (the barrier only pins the compiler)
  {
    const double val = (lane >= j + 1 && S.mine) ? S.rr * S.w : 0.0;
    // no exec-mask juggling on the chain's path: lanes past the buffer hold +0.0 (they are beyond nact) and write it to the
    // last slot, which is +0.0 anyway (kBsLen >= nact + 12)
    if constexpr (kBsLen <= 64) bn[lane < kBsLen ? lane : kBsLen - 1] = val;
    else bn[lane] = val;
    S.rr = Rp(jnn, S.col);
  }
  __builtin_amdgcn_wave_barrier();
  {
    // the eight terms through ONE address register with constant offsets (the scalar address arithmetic and the move into a vector
    // register were repeated for every pair), the superdiagonal entry from the register its row's lane loaded before the first row
    typedef __attribute__((address_space(3))) double lds_f64;
    const lds_f64 *np = (const lds_f64 *)(bn + j + 1);
    asm volatile("" : "+v"(np));
    constexpr int kNext = kExact && kHead < 8 ? kHead : 8;  // the next row has one term more than this one, the first from registers
#pragma unroll
    for (int e = 0; e < kNext; ++e) Nx[e] = np[e];          // prefetch: the next row's first terms
    Nx[8] = rl(S.rsd, jn);
  }
  const double sj = rl(S.sreg, j), dj = rl(S.dreg, j);
  double sum = 0.0;
  if constexpr (kExact && kHead >= 1 && kHead <= 8) {
    sum += P[8] * S.wprev;
#pragma unroll
    for (int e = 0; e < kHead - 1; ++e) sum += P[e];
  } else
  if constexpr (kHead >= 4) {
    sum += P[8] * S.wprev;
    sum += P[0]; sum += P[1]; sum += P[2]; sum += P[3];
    if constexpr (kHead >= 8) { sum += P[4]; sum += P[5]; sum += P[6]; sum += P[7]; }
    if constexpr (kHead >= 9) {
      // the tail through one walking address register: entries up to nact + 6 <= kBsLen - 6 are read (nact <= kBsLen - 12), no clamp
      typedef __attribute__((address_space(3))) double lds_f64;
      const lds_f64 *tp = (const lds_f64 *)(bj + j + 10);
      asm volatile("" : "+v"(tp));
      double a0 = tp[0], a1 = tp[1], a2 = tp[2], a3 = tp[3];
      for (int k = j + 10; k < nact; k += 4) {
        const double b0 = tp[4], b1 = tp[5], b2 = tp[6], b3 = tp[7];
        sum += a0; sum += a1; sum += a2; sum += a3;
        a0 = b0; a1 = b1; a2 = b2; a3 = b3;
        tp += 4;
      }
    }
  } else if constexpr (kHead == 0) {
  } else
  if (j + 1 < nact) {
    sum += P[8] * S.wprev;
    sum += P[0]; sum += P[1]; sum += P[2]; sum += P[3];
    if (j + 6 < nact) {
      sum += P[4]; sum += P[5]; sum += P[6]; sum += P[7];
      if (j + 10 < nact) {
        typedef __attribute__((address_space(3))) double lds_f64;
        const lds_f64 *tp = (const lds_f64 *)(bj + j + 10);
        asm volatile("" : "+v"(tp));
        double a0 = tp[0], a1 = tp[1], a2 = tp[2], a3 = tp[3];
        for (int k = j + 10; k < nact; k += 4) {
          const double b0 = tp[4], b1 = tp[5], b2 = tp[6], b3 = tp[7];
          sum += a0; sum += a1; sum += a2; sum += a3;
          a0 = b0; a1 = b1; a2 = b2; a3 = b3;
          tp += 4;
        }
      }
    }
  }
  const double v = (sj - sum) / dj;
  if (lane == j) S.w = v;
  S.wprev = v;
}
template <int kBsLen = 48, bool kExact = false>             // nact <= 64 (one multiplier per lane) and nact + 12 <= kBsLen; kExact: bs_row
__device__ __forceinline__ void backsub_lds(const QlView &q, const double *s, int nact, int lane, double *buf) {
  BsState S;
  S.mine = lane < nact; S.nact = nact; S.lane = lane;
  if constexpr (kBsLen <= 64) {
    // loads from clamped addresses and selects: a load under a lane-dependent condition is an exec-mask save / restore
    const int ml = S.mine ? lane : 0;
    const double sv = s[ml], dv = Rp(ml, ml);
    S.sreg = S.mine ? sv : 0.0;
    S.dreg = S.mine ? dv : 1.0;
  } else {                                                  // the 168-register kernels (N = 32) keep the predicated form: measured
    S.sreg = S.mine ? s[lane] : 0.0;
    S.dreg = S.mine ? Rp(lane, lane) : 1.0;
  }
  if constexpr (kBsLen <= 64) {
    const int zl = lane < kBsLen ? lane : kBsLen - 1; buf[zl] = 0.0; buf[kBsLen + zl] = 0.0;
    const int rlc = lane + 1 < nact ? lane : 0;              // rows without a first term (the last one, lanes past it) read R(0, 1): unused
    S.rsd = Rp(rlc, rlc + 1);
  }
  else {
    for (int e = lane; e < kBsLen; e += 64) { buf[e] = 0.0; buf[kBsLen + e] = 0.0; }
    const int rlc = lane + 1 < nact ? lane : 0;
    S.rsd = Rp(rlc, rlc + 1);
  }
  S.col = S.mine ? lane : 0;
  S.w = 0.0; S.wprev = 0.0;
  S.rr = Rp(nact >= 2 ? nact - 2 : 0, S.col);               // R(j-1, lane) of the row whose products are formed next
  double A9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, B9[9];
  int j = nact - 1;
  if constexpr (kBsLen <= 64) {
    // the first nine rows unrolled with their lengths known (one uniform test per row instead of three), the rest in pairs
    if (nact > 0) { bs_row<kBsLen, 0, kExact>(q, buf, nact - 1, S, A9, B9);
    if (nact > 1) { bs_row<kBsLen, kExact ? 1 : 4, kExact>(q, buf, nact - 2, S, B9, A9);
    if (nact > 2) { bs_row<kBsLen, kExact ? 2 : 4, kExact>(q, buf, nact - 3, S, A9, B9);
    if (nact > 3) { bs_row<kBsLen, kExact ? 3 : 4, kExact>(q, buf, nact - 4, S, B9, A9);
    if (nact > 4) { bs_row<kBsLen, 4, kExact>(q, buf, nact - 5, S, A9, B9);
    if (nact > 5) { bs_row<kBsLen, kExact ? 5 : 8, kExact>(q, buf, nact - 6, S, B9, A9);
    if (nact > 6) { bs_row<kBsLen, kExact ? 6 : 8, kExact>(q, buf, nact - 7, S, A9, B9);
    if (nact > 7) { bs_row<kBsLen, kExact ? 7 : 8, kExact>(q, buf, nact - 8, S, B9, A9);
    if (nact > 8) { bs_row<kBsLen, 8, kExact>(q, buf, nact - 9, S, A9, B9);
      for (j = nact - 10; j >= 1; j -= 2) { bs_row<kBsLen, 9>(q, buf, j, S, B9, A9); bs_row<kBsLen, 9>(q, buf, j - 1, S, A9, B9); }
      if (j == 0) bs_row<kBsLen, 9>(q, buf, 0, S, B9, A9);
    }}}}}}}}}
  } else {
    for (; j >= 1; j -= 2) { bs_row<kBsLen>(q, buf, j, S, A9, B9); bs_row<kBsLen>(q, buf, j - 1, S, B9, A9); }
    if (j == 0) bs_row<kBsLen>(q, buf, 0, S, A9, B9);
  }
  if constexpr (kBsLen <= 64) {
    if (nact > 0) {                                         // lanes past nact shadow lane nact - 1: its value to its address
      const double wl = rl(S.w, nact - 1);
      q.ww[S.mine ? lane : nact - 1] = S.mine ? S.w : wl;
    }
  } else if (S.mine) q.ww[lane] = S.w;
  WG_WSYNC();
}

// ---------------------------------------------------------------------------------------------------
// Compile-time-bounded versions for n <= NM (the Herdt QP: NM = 36).  Measured on MI355X (tools/micro/lat.hip):
// a dependent fp64 add/mul costs ~8 cycles, an add fed by v_readlane ~40, a divide 71, sqrt ~100.  With static
// trip counts every LDS address is an immediate offset, so the compiler issues all loads ahead of the dependent
// chain and the ordered sums run at the 8-cycle floor.
// ---------------------------------------------------------------------------------------------------

// sum of term[0..cnt) in index order (term lives one-per-lane); scratch: NM doubles of LDS, 16-byte aligned.
#ifndef WG_OS_CHUNK
#define WG_OS_CHUNK 12
#endif
constexpr int kOsChunk = WG_OS_CHUNK;
template <int NM>
__device__ __forceinline__ double ordered_sum_lds(double term, double *scratch, int cnt, int lane) {
  {
    const double v = (lane < cnt) ? term : 0.0;
    const double vl = rl(v, NM - 1);                        // lanes past NM shadow lane NM - 1
    scratch[lane < NM ? lane : NM - 1] = lane < NM ? v : vl;
  }
  WG_WSYNC();
  // loads in groups of kOsChunk ahead of the add chain: enough to cover the LDS latency, few enough live registers
  double sum = 0.0;
#pragma unroll
  for (int i0 = 0; i0 < NM; i0 += kOsChunk) {
    double t[kOsChunk];
#pragma unroll
    for (int i = 0; i < kOsChunk; ++i) t[i] = (i0 + i < NM) ? scratch[i0 + i] : 0.0;
#pragma unroll
    for (int i = 0; i < kOsChunk; ++i) if (i0 + i < NM) sum += t[i];   // entries >= cnt are +0.0: they leave the sum unchanged
  }
  WG_WSYNC();
  return sum;
}

// The same sum in the same order as a rolled loop: the cold form behind the guarded sums (wg_ql_guard.hpp), run when a
// certificate doubts or when the knob asks for the reference's order throughout.  Code that never runs still costs the
// 256-register kernel, so the fallbacks stay small.
template <int NM>
__device__ __forceinline__ double ordered_sum_lds_rolled(double term, double *scratch, int cnt, int lane) {
  {
    const double v = (lane < cnt) ? term : 0.0;
    const double vl = rl(v, NM - 1);                        // lanes past NM shadow lane NM - 1
    scratch[lane < NM ? lane : NM - 1] = lane < NM ? v : vl;
  }
  WG_WSYNC();
  double sum = 0.0;
#pragma nounroll
  for (int i = 0; i < NM; ++i) sum += scratch[i];           // entries >= cnt are +0.0: they leave the sum unchanged
  WG_WSYNC();
  return sum;
}

// Givens sweep (qld.cpp:1992-2030) for n <= 64, written without data-dependent control flow: on a single
// resident wave every taken branch costs tens of cycles, so predicates become selects, inactive lanes shadow
// lane n-1 (same addresses, same values), and LDS operands are fetched one or two steps ahead of the
// dependent chain.
//   phase 1  chain of rotation norms (all lanes redundantly; s[c-1] prefetched); lane c records its rotation;
//   phase 2  lane c turns (p, q, norm) into (ga, gb) and publishes the pair in LDS;
//   phase 3  lane i carries row i of Z through the rotations.
//   phase 1, seeded (kSeeded: the compact N = 16 view; wg_ql_norms.hpp): from the last non-zero entry of s on the chain runs from
//            seeds -- 1/t and 1/sqrt(x) of every rotation, made lane-parallel from a scan of the squares and handed over through
//            sc0 / sc1 (dead until phase 2 writes the pairs there) -- in 11 dependent instructions per rotation instead of 23;
//            afterwards lane c recomputes its rotation in the exact form from the operands phase 2 loads anyway and compares
//            bits.  One ballot; on a mismatch (or nmode == kNormsDoubt) the exact code below runs as if nothing had happened:
//            a flag and a forward edge.  nmode == kNormsExact: the exact code alone.
template <int kLdzC = 0, bool kSeeded = false>               // kLdzC > 0: Z lives in LDS with this leading dimension (every compile-time-bounded view)
__device__ __forceinline__ void sweep_flat(const QlView &q, double *s, int nu, int nact, int lane, [[maybe_unused]] int nmode = kNormsExact PT_SW_PARAM) {
  const int n = q.n;
  if (nu - 1 <= nact) return;
  PT_SW_BEGIN
  PT_SW_COUNT(PS_N_SWEEPS);
  // Phase 1 leaves ONE value per rotation behind -- `cur` as it leaves rotation c, in chain[c - 1] -- from which lane c
  // rebuilds its rotation afterwards: q = the value that entered (chain[c], or s[nu-1] for the first one), p = s[c-1]
  // (untouched until phase 2), norm = chain[c-1] when q != 0 (then cur = norm), skipped when q == 0 (then cur = p).
  // givens_norm runs unguarded on q == 0: its result (|p|, or NaN for 0/0) is discarded by the select.
  double *chain = q.sc2;                                    // nu <= n entries
  // seeded chain: the operands of lane c's rotation as the check loaded them, and whether the check let them through
  [[maybe_unused]] bool seeded_ok = false;
  [[maybe_unused]] double sdP = 0.0, sdQ = 0.0, sdN = 0.0;
  WG_REP(3) {
  if constexpr (kSeeded) {
    seeded_ok = false;
    if (nmode != kNormsExact && sweep_range_ok<true>(s, nact, nu, lane)) {
      PT_SW_COUNT(PS_N_SEEDED);
      typedef __attribute__((address_space(3))) double lds_f64;
      double *seeds = q.sc0;                                // pairs {r, y} of rotation c at 2 c, 2 c + 1 (sc0 and sc1 are adjacent)
      int top;                                              // s[top - 1]: the last non-zero entry (nact + 1 when there is none above s[nact])
      {
        // lane L makes the seeds of rotation c = nu - 1 - L: its entry s[c] squared, the sums of the squares of s[c .. nu) by a
        // prefix scan over the lanes, and p = s[c - 1].  Lanes without a rotation compute on entries of the sweep and store nothing.
        // Zeros at the end of s (structural zeros of Z: three sweeps in ten end in one) are rotations the reference skips,
        // each handing its p on: their records are copies of s, written here, and the chain starts at the last non-zero entry.
        const int j = nu - 1 - lane;
        const bool in = j >= nact;
        const double sj = s[in ? j : nact], pj = s[j > nact ? j - 1 : nact];
        const unsigned long long nz = __ballot(in && j > nact && sj != 0.0);
        top = nz ? nu - __builtin_ctzll(nz) : nact + 1;
        if (in && j >= top - 1 && j < nu - 1) chain[j] = sj;
        const double s2 = wave_prefix_sum(in ? sj * sj : 0.0);
        const NormSeed sd = norms_seed(pj * pj, s2);
        if (j > nact && j < top) { seeds[2 * j] = sd.r; seeds[2 * j + 1] = sd.y; }
      }
      WG_WSYNC();
      // the chain, unrolled by two as below; the seeds of a rotation are fetched with its operand, one rotation ahead, through a
      // third walking pointer (the pair fetched ahead of the last rotation belongs to rotation nact: inside sc0, never used)
      const int rots = top - 1 - nact;                      // rotations below the last non-zero entry
      if (rots > 0) {
        double cur = s[top - 1];
        double pa = s[top - 2], pb;
        const lds_f64 *sp = (const lds_f64 *)(s + (top - 4));      // sp[1] = s[c - 2], sp[0] = s[c - 3]
        lds_f64 *cp = (lds_f64 *)(chain + (top - 3));              // cp[1] = chain[c - 1], cp[0] = chain[c - 2]
        const lds_f64 *dp = (const lds_f64 *)(seeds + 2 * (top - 3));   // dp[2], dp[3]: rotation c - 1;  dp[0], dp[1]: rotation c - 2
        asm volatile("" : "+v"(sp), "+v"(cp), "+v"(dp));
        double ra = dp[4], ya = dp[5], rb, yb;
        auto step = [](double p, double cur_in, double r, double y) -> double {
          double t, a;
          asm("v_max_f64 %0, |%1|, |%2|" : "=v"(t) : "v"(p), "v"(cur_in));
          asm("v_min_f64 %0, |%1|, |%2|" : "=v"(a) : "v"(p), "v"(cur_in));
          return norms_step(t, a, r, y);
        };
        for (int k = rots >> 1; k > 0; --k) {
          pb = sp[1]; rb = dp[2]; yb = dp[3];
          cur = step(pa, cur, ra, ya); cp[1] = cur;
          pa = sp[0]; ra = dp[0]; ya = dp[1];
          cur = step(pb, cur, rb, yb); cp[0] = cur;
          sp -= 2; cp -= 2; dp -= 4;
        }
        if (rots & 1) { cur = step(pa, cur, ra, ya); cp[1] = cur; }
      }
      WG_WSYNC();
      // the check: lane c's rotation in the exact form, from the operands phase 2 needs anyway (lanes without one shadow lane nu - 1)
      {
        const bool mine = lane > nact && lane < nu;
        const int c = mine ? lane : nu - 1;
        sdP = s[c - 1];
        sdQ = (c == nu - 1) ? s[nu - 1] : chain[c];
        sdN = chain[c - 1];
        const bool bad = !norms_rotation_ok(sdP, sdQ, sdN);
        seeded_ok = (__ballot(bad) == 0ull) && nmode != kNormsDoubt;
      }
      if (!seeded_ok) PT_SW_COUNT(PS_N_SEED_FALLBACK);
    }
  }
  if (kSeeded && seeded_ok) {
  } else
  if (sweep_range_ok<true>(s, nact, nu, lane)) {
    // the usual case: the shorter norm; unrolled by two so that handing the prefetched operand on is a renaming.  The operand
    // and the record are reached through two walking pointers kept in vector registers (constant offsets in the ds instructions,
    // one v_add per pair of rotations) instead of clamped indices rebuilt from the scalar counter for every access; the operand
    // fetched ahead of the LAST rotation may lie one or two entries below s (nact = 0): in the wave's LDS (s is never the first
    // array of a view; an out-of-range LDS read returns zero anyway), and never used.
    double cur = s[nu - 1];
    double pa = s[nu - 2], pb;
    int c = nu - 1;
    typedef __attribute__((address_space(3))) double lds_f64;  // s (R's working column) and the scratch vectors are LDS in every view that sweeps here
    const lds_f64 *sp = (const lds_f64 *)(s + (nu - 4));      // sp[1] = s[c - 2], sp[0] = s[c - 3]
    lds_f64 *cp = (lds_f64 *)(chain + (nu - 3));              // cp[1] = chain[c - 1], cp[0] = chain[c - 2]
    asm volatile("" : "+v"(sp), "+v"(cp));
    // pairs in a counted loop with ONE exit (the two-exit form cost a flag and a trampoline block per rotation), then the odd one
    const int rots = c - nact;                              // >= 1
    if (WG_UBOOL(cur != 0.0)) {
      // a norm is at least its larger operand: once cur is non-zero it stays non-zero, no rotation is skipped and the
      // "cur == 0 ? p : norm" select of the general form below always takes the norm
      for (int k = rots >> 1; k > 0; --k) {
        pb = sp[1];                                         // operand of the next rotation, off the chain
        cur = givens_norm_fast(pa, cur); cp[1] = cur;
        pa = sp[0];
        cur = givens_norm_fast(pb, cur); cp[0] = cur;
        sp -= 2; cp -= 2;
      }
      if (rots & 1) { cur = givens_norm_fast(pa, cur); cp[1] = cur; }
    } else {
      for (int k = rots >> 1; k > 0; --k) {
        pb = sp[1];
        { const double nrmc = givens_norm_fast(pa, cur); cur = (cur == 0.0) ? pa : nrmc; cp[1] = cur; }
        pa = sp[0];
        { const double nrmc = givens_norm_fast(pb, cur); cur = (cur == 0.0) ? pb : nrmc; cp[0] = cur; }
        sp -= 2; cp -= 2;
      }
      if (rots & 1) { const double nrmc = givens_norm_fast(pa, cur); cur = (cur == 0.0) ? pa : nrmc; cp[1] = cur; }
    }
  } else {
    double cur = s[nu - 1];
    double p = s[nu - 2];
    for (int c = nu - 1; c > nact; --c) {
      const int nx = (c - 2 >= 0) ? c - 2 : 0;
      const double p_next = s[nx];                          // operand of the next rotation, off the chain
      const double nrmc = givens_norm(p, cur);
      cur = (cur == 0.0) ? p : nrmc;
      chain[c - 1] = cur;
      p = p_next;
    }
  }
  }   // WG_REP(3)
  WG_WSYNC();
  PT_SW(PS_SW_NORMS);
  double myP = 0.0, myQ = 0.0, myN = 0.0;
  if (kSeeded && seeded_ok) {                               // the check has loaded them
    myP = sdP; myQ = sdQ; myN = (sdQ == 0.0) ? 0.0 : sdN;
  } else {
    const bool mine = lane > nact && lane < nu;
    const int c = mine ? lane : nu - 1;
    myP = s[c - 1];
    myQ = (c == nu - 1) ? s[nu - 1] : chain[c];
    const double chl = chain[c - 1];
    myN = (myQ == 0.0) ? 0.0 : chl;
  }
  WG_WSYNC();
  double *gab = q.sc0;                                      // pairs {ga, gb}; sc0 and sc1 are adjacent (2n doubles)
  bool any_skip;
  {
    const bool mine = lane > nact && lane < nu;
    const bool rot = mine && myN != 0.0;
    const double den = rot ? myN : 1.0;
    // ga == 2 marks a skipped rotation (q was 0; a rotation's |ga| = |p| / norm <= 1).  NOT gb == 0: a denormal q under a large p
    // gives gb = q / norm = 0 by underflow and ga = -1 for p < 0 -- a rotation the reference carries out (both columns change sign)
    const double ga = rot ? myP / den : 2.0;
    const double gb = rot ? myQ / den : 0.0;
    // a skipped rotation is rare: when the sweep has none -- one ballot -- phase 3 runs without the selects
    any_skip = __ballot(mine && !rot) != 0ull;
    const int cl = mine ? lane : nu - 1;                    // lanes without a rotation shadow lane nu-1 ... with ITS values
    const double ga_l = rl(ga, nu - 1), gb_l = rl(gb, nu - 1);
    const double ga_w = mine ? ga : ga_l, gb_w = mine ? gb : gb_l;
    gab[2 * cl] = ga_w; gab[2 * cl + 1] = gb_w;
    if (rot) s[lane - 1] = myN;
  }
  WG_WSYNC();
  PT_SW(PS_SW_COEFF);
  {
    // phase 3: lane i carries row i of Z through the rotations.  Operands of rotation c -- Z(i, c-1) and the pair
    // (ga, gb) -- are fetched three rotations ahead into one of three register sets used in turn (an unroll by three, so
    // that handing a set on is a renaming, not a move).
    const int i = lane < n ? lane : n - 1;                  // surplus lanes shadow row n-1
    const int ldz = q.ldz;
    double *zp = q.Z + i + (nu - 1) * ldz;                  // Z(i, c)
    double carry = zp[0];
    struct Op { double zl, ga, gb; };
    auto fetch = [&](int c) -> Op {                         // operands of rotation c (clamped: unused past the end)
      const int cc = c > nact ? c : nact + 1;
      Op o; o.zl = q.Z[i + (cc - 1) * ldz]; o.ga = gab[2 * cc]; o.gb = gab[2 * cc + 1];
      return o;
    };
    auto rotate = [&](const Op &o) {
      const bool skip = (o.ga == 2.0);
      const double t_r = o.ga * o.zl + o.gb * carry;
      const double z_r = o.ga * carry - o.gb * o.zl;
      zp[0] = skip ? carry : z_r;
      carry = skip ? o.zl : t_r;
      zp -= ldz;
    };
    auto rotate_all = [&](const Op &o) {
      const double t_r = o.ga * o.zl + o.gb * carry;
      zp[0] = o.ga * carry - o.gb * o.zl;
      carry = t_r;
      zp -= ldz;
    };
    Op s0 = fetch(nu - 1), s1 = fetch(nu - 2), s2 = fetch(nu - 3);
    int c = nu - 1;
    if (any_skip) {
      for (;;) {
        { const Op nx = fetch(c - 3); rotate(s0); s0 = nx; }
        if (--c <= nact) break;
        { const Op nx = fetch(c - 3); rotate(s1); s1 = nx; }
        if (--c <= nact) break;
        { const Op nx = fetch(c - 3); rotate(s2); s2 = nx; }
        if (--c <= nact) break;
      }
    } else {
      // Groups of three while every rotation fetched ahead exists (c - 5 > nact): ONE exit test per three rotations, the
      // operands through two walking pointers with constant offsets (no clamp, no index arithmetic), the three register sets
      // handed on where the loop closes -- the stepping loop below (clamped fetches, a test per rotation, and the moves the
      // compiler needs to make its three exits agree) took 23 instructions per rotation for 6 of arithmetic and 3 of LDS
      if constexpr (kLdzC > 0) {
        // Z in LDS with a constant leading dimension: every operand and every store of a group through THREE address registers
        // (the group's lowest column of operands, of pairs, of stores) with constant offsets -- a v_add, or a scalar add and a move
        // into a vector register, per access otherwise
        typedef __attribute__((address_space(3))) double lds_f64;
        constexpr int L = kLdzC;
        while (c - 8 > nact) {                              // six at a time: the two register sets swap roles, no moves
          const lds_f64 *zlo = (const lds_f64 *)(q.Z + i + (c - 9) * L);      // Z(i, c - 9): operand of rotation c - 8
          const lds_f64 *glo = (const lds_f64 *)(gab + 2 * (c - 8));
          lds_f64 *zst = (lds_f64 *)(q.Z + i + (c - 5) * L);                   // Z(i, c - 5): the group's last store
          asm volatile("" : "+v"(zlo), "+v"(glo), "+v"(zst));
          Op n0, n1, n2;
          n0.zl = zlo[5 * L]; n0.ga = glo[10]; n0.gb = glo[11];
          n1.zl = zlo[4 * L]; n1.ga = glo[8];  n1.gb = glo[9];
          n2.zl = zlo[3 * L]; n2.ga = glo[6];  n2.gb = glo[7];
          { const double t = s0.ga * s0.zl + s0.gb * carry; zst[5 * L] = s0.ga * carry - s0.gb * s0.zl; carry = t; }
          { const double t = s1.ga * s1.zl + s1.gb * carry; zst[4 * L] = s1.ga * carry - s1.gb * s1.zl; carry = t; }
          { const double t = s2.ga * s2.zl + s2.gb * carry; zst[3 * L] = s2.ga * carry - s2.gb * s2.zl; carry = t; }
          s0.zl = zlo[2 * L]; s0.ga = glo[4]; s0.gb = glo[5];
          s1.zl = zlo[L];     s1.ga = glo[2]; s1.gb = glo[3];
          s2.zl = zlo[0];     s2.ga = glo[0]; s2.gb = glo[1];
          { const double t = n0.ga * n0.zl + n0.gb * carry; zst[2 * L] = n0.ga * carry - n0.gb * n0.zl; carry = t; }
          { const double t = n1.ga * n1.zl + n1.gb * carry; zst[L] = n1.ga * carry - n1.gb * n1.zl; carry = t; }
          { const double t = n2.ga * n2.zl + n2.gb * carry; zst[0] = n2.ga * carry - n2.gb * n2.zl; carry = t; }
          c -= 6;
        }
        while (c - 5 > nact) {
          const lds_f64 *zlo = (const lds_f64 *)(q.Z + i + (c - 6) * L);      // Z(i, c - 6): operand of rotation c - 5
          const lds_f64 *glo = (const lds_f64 *)(gab + 2 * (c - 5));
          lds_f64 *zst = (lds_f64 *)(q.Z + i + (c - 2) * L);
          asm volatile("" : "+v"(zlo), "+v"(glo), "+v"(zst));
          Op n0, n1, n2;
          n0.zl = zlo[2 * L]; n0.ga = glo[4]; n0.gb = glo[5];
          n1.zl = zlo[L];     n1.ga = glo[2]; n1.gb = glo[3];
          n2.zl = zlo[0];     n2.ga = glo[0]; n2.gb = glo[1];
          { const double t = s0.ga * s0.zl + s0.gb * carry; zst[2 * L] = s0.ga * carry - s0.gb * s0.zl; carry = t; }
          { const double t = s1.ga * s1.zl + s1.gb * carry; zst[L] = s1.ga * carry - s1.gb * s1.zl; carry = t; }
          { const double t = s2.ga * s2.zl + s2.gb * carry; zst[0] = s2.ga * carry - s2.gb * s2.zl; carry = t; }
          s0 = n0; s1 = n1; s2 = n2;
          c -= 3;
        }
        zp = q.Z + i + c * ldz;                              // where the stepping loop goes on
      } else {
        const double *zq = q.Z + i + (c - 4) * ldz;          // Z(i, c - 4): operand of rotation c - 3
        const double *gq = gab + 2 * (c - 3);
        while (c - 8 > nact) {                              // six at a time: the two register sets swap roles, no moves
          Op n0, n1, n2;
          n0.zl = zq[0];        n0.ga = gq[0];  n0.gb = gq[1];
          n1.zl = zq[-ldz];     n1.ga = gq[-2]; n1.gb = gq[-1];
          n2.zl = zq[-2 * ldz]; n2.ga = gq[-4]; n2.gb = gq[-3];
          rotate_all(s0); rotate_all(s1); rotate_all(s2);
          s0.zl = zq[-3 * ldz]; s0.ga = gq[-6];  s0.gb = gq[-5];
          s1.zl = zq[-4 * ldz]; s1.ga = gq[-8];  s1.gb = gq[-7];
          s2.zl = zq[-5 * ldz]; s2.ga = gq[-10]; s2.gb = gq[-9];
          rotate_all(n0); rotate_all(n1); rotate_all(n2);
          zq -= 6 * ldz; gq -= 12; c -= 6;
        }
        while (c - 5 > nact) {
          Op n0, n1, n2;
          n0.zl = zq[0];        n0.ga = gq[0];  n0.gb = gq[1];
          n1.zl = zq[-ldz];     n1.ga = gq[-2]; n1.gb = gq[-1];
          n2.zl = zq[-2 * ldz]; n2.ga = gq[-4]; n2.gb = gq[-3];
          rotate_all(s0); rotate_all(s1); rotate_all(s2);
          s0 = n0; s1 = n1; s2 = n2;
          zq -= 3 * ldz; gq -= 6; c -= 3;
        }
      }
      if constexpr (kLdzC > 0) {
        // the last one to five rotations, straight-line per count: columns relative to nact through two address registers with
        // constant offsets, the operands of the first three rotations are in s0 / s1 / s2 already, the others are requested
        // together before the first rotation; ends with Z(i, nact) = carry
        typedef __attribute__((address_space(3))) double lds_f64;
        constexpr int L = kLdzC;
        lds_f64 *zb = (lds_f64 *)(q.Z + i + nact * L);        // Z(i, nact)
        const lds_f64 *gb_ = (const lds_f64 *)(gab + 2 * nact);
        asm volatile("" : "+v"(zb), "+v"(gb_));
        auto rot = [&](const Op &o, int k) {                  // rotation nact + k: stores Z(i, nact + k)
          const double t = o.ga * o.zl + o.gb * carry;
          zb[k * L] = o.ga * carry - o.gb * o.zl;
          carry = t;
        };
        auto ld = [&](int k) -> Op { Op o; o.zl = zb[(k - 1) * L]; o.ga = gb_[2 * k]; o.gb = gb_[2 * k + 1]; return o; };
        switch (c - nact) {
          case 5: { const Op o2 = ld(2), o1 = ld(1); rot(s0, 5); rot(s1, 4); rot(s2, 3); rot(o2, 2); rot(o1, 1); break; }
          case 4: { const Op o1 = ld(1); rot(s0, 4); rot(s1, 3); rot(s2, 2); rot(o1, 1); break; }
          case 3: rot(s0, 3); rot(s1, 2); rot(s2, 1); break;
          case 2: rot(s0, 2); rot(s1, 1); break;
          default: rot(s0, 1); break;
        }
        zb[0] = carry;                                        // Z(i, nact)
      } else {
      for (;;) {                                            // the last (at most five) rotations
        { const Op nx = fetch(c - 3); rotate_all(s0); s0 = nx; }
        if (--c <= nact) break;
        { const Op nx = fetch(c - 3); rotate_all(s1); s1 = nx; }
        if (--c <= nact) break;
        { const Op nx = fetch(c - 3); rotate_all(s2); s2 = nx; }
        if (--c <= nact) break;
      }
      zp[0] = carry;                                         // Z(i, nact)
      }
    }
    if (any_skip) zp[0] = carry;                             // Z(i, nact)
  }
  WG_WSYNC();
  PT_SW(PS_SW_ROWS);
}

// qld.cpp:1861-1889.  Returns kdrop (0-based) or -1; ratio updated when found.
// ---- the two SELECTIONS of an iteration once values stop being ordinary numbers (round 5) ------------------------------------
// The violation scan and the ratio test pick a row by a running comparison -- "skip unless strictly better than the best so far" --
// which the lane-parallel forms below replace by per-lane candidates and a wave arg-max (first index among equals).  The two agree
// while every compared value is an ordinary number.  Once the iterate holds a NaN they do not: the reference's `if (sumx <= cvmax)
// goto skip` does NOT skip a NaN, and with cvmax = NaN it skips nothing any more -- the LAST row that passes its other tests wins,
// which no arg-max reproduces (found on two of 2304 random Herdt-shaped QPs: the reference loops to maxit and reports ifail = 1,
// the arg-max form "converged" with ifail = 0 and a NaN solution).  So: when x (or the ratio test's operands) is not a number of
// sane size -- one compare per lane and one ballot per iteration -- the wave takes the forms below instead: scan_nan_exact
// (lane-parallel, with the reference's dense row sums and its NaN semantics) and the ratio test as the reference's own loop.
// Such a solve is lost and only has to end the way the reference's does -- but it runs maxit = 40 (m + n) iterations on the
// way, and a fleet waits for its slowest gait: the scan is lane-parallel for that reason (a first, fully serial form took 1 ms
// per iteration in the compact view, 4.5 s per lost tick).
#ifndef WG_TICK_NAN_EXACT
#define WG_TICK_NAN_EXACT 1                                // 0: the tick's views without these forms (A/B of their cost); see mpc_tick
#endif
#ifndef WG_NAN_REGIME
#define WG_NAN_REGIME 1                                    // 0: experiment builds without the NaN-regime tests (A/B of their cost)
#endif
// |v| < 2^332 (8.7e99): false for NaN, infinities and overflow-bound values.  On the exponent field of the high word -- an integer
// mask and a compare against a 32-bit literal: a 64-bit floating-point literal would be hoisted into a scalar register pair and
// kept alive (or spilled) across the active-set loop, which is what wg_kconst exists to avoid
__device__ __forceinline__ bool wg_sane(double v) { return ((unsigned)__double2hiint(v) & 0x7fffffffu) < 0x54b00000u; }

// qld.cpp:1255-1331 for an iterate that may hold NaNs and infinities, lane-parallel.  What the reference's loop does, restated:
// a row (or bound) is a CANDIDATE when it passes every test that does not involve cvmax (weight, significance of the residual;
// `sum != 0` for a bound) -- written below as the reference's own comparisons, negated, so that a NaN operand passes exactly
// where it passes there.  Candidates are visited in order (rows 1..m, then the bounds by variable) and taken unless
// `value <= cvmax`; a taken candidate's value becomes cvmax.  While every value is a number that is the first strict maximum
// above 0.  A candidate whose value is a NaN is taken (NaN <= cvmax is false) and leaves cvmax = NaN, so the NEXT candidate is
// taken whatever its value -- and if that value is a number, the running maximum starts again from it.  Hence: with L the last
// candidate whose value is a NaN, the winner is the first maximum among the candidates BEHIND L (no threshold: the first of them
// is always taken), or L itself when none follows.  Row sums are the reference's DENSE sums -- every x_i times every
// coefficient, the structural zeros included: 0 * inf and 0 * NaN are NaN there, which a view that skips its zeros would not
// produce -- one row per lane, terms in index order.
template <class P>
__device__ __forceinline__ void scan_nan_exact(const QlView &q, const P &prob, double onha, double &cvmax, double &res,
                                               double &wsel, int &knext, int lane) {
  const int n = q.n, m = q.m, me = q.me, mn = q.mn;
  struct Row { bool cand; double v, r, w; int code; };
  auto eval = [&](int pos) -> Row {
    Row o;
    if (pos < m) {
      const int k = pos;
      o.w = q.wa[k];
      const double bk = q.b[k];
      double sum = -bk, temp = fabs(bk);
      for (int i = 0; i < n; ++i) {
        double aki;
        if constexpr (P::kCompact) aki = prob.A_own(k, i); else aki = Am(k, i);
        const double t = q.x[i] * aki; sum += t; temp += fabs(t);
      }
      o.v = -sum * o.w;
      if (k + 1 <= me) o.v = fabs(o.v);
      const double tempa = temp + fabs(sum);
      const double temp2 = temp + onha * fabs(sum);
      o.cand = !(o.w <= 0.0) && !(tempa <= temp) && !(temp2 <= tempa);
      o.r = sum; o.code = k + 1;
    } else {
      const int k = pos - m;
      o.w = q.wa[m + k];
      const double xk = q.x[k], s1 = prob.xl(q, k) - xk;
      const bool upper = s1 < 0.0;
      o.v = upper ? xk - prob.xu(q, k) : s1;
      o.cand = !(o.w <= 0.0) && !(s1 == 0.0);
      o.r = -o.v; o.code = upper ? k + 1 + mn : k + 1 + m;
    }
    return o;
  };
  // the lane's j-th position, ascending in j: lane + 64 j -- or, in the compact view (whose rows' coefficients live in their
  // lanes' registers), CoP row lane + 1, foot-placement row 1 + 4N + lane, bound lane (row 0, all zeros, is never a
  // candidate).  -1: the lane has no j-th position
  auto position = [&](int j) -> int {
    if constexpr (P::kCompact) {
      if (j == 0) return (lane + 1 <= P::kCopRows && lane + 1 < m) ? lane + 1 : -1;
      if (j == 1) return (1 + P::kCopRows + lane < m) ? 1 + P::kCopRows + lane : -1;
      return lane < n ? m + lane : -1;
    } else {
      const int pos = lane + 64 * j;
      return pos < m + n ? pos : -1;
    }
  };
  const int slots = P::kCompact ? 3 : (m + n + 63) / 64;
  // pass 1: the all-numbers answer (running strict maximum above 0 = cvmax's start), and the lane's last NaN candidate
  double av = 0.0, ar = 0.0, aw = 0.0;
  int apos = -1, acode = 0;
  double nr = 0.0, nw = 0.0;
  int npos = -1, ncode = 0;
  for (int j = 0; j < slots; ++j) {
    const int pos = position(j);
    if (pos < 0) continue;
    const Row o = eval(pos);
    if (!o.cand) continue;
    if (o.v != o.v) { npos = pos; nr = o.r; nw = o.w; ncode = o.code; }
    else if (o.v > av) { av = o.v; ar = o.r; aw = o.w; apos = pos; acode = o.code; }
  }
  const int lastnan = uni(wave_max_int(npos));
  int src;
  if (lastnan >= 0) {
    // pass 2: the candidates behind the last NaN (numbers all of them): first maximum, the first one taken unconditionally
    bool any = false;
    av = 0.0; apos = -1;
    for (int j = 0; j < slots; ++j) {
      const int pos = position(j);
      if (pos <= lastnan) continue;                          // (covers pos == -1)
      const Row o = eval(pos);
      if (!o.cand) continue;
      if (!any || o.v > av) { av = o.v; ar = o.r; aw = o.w; apos = pos; acode = o.code; }
      any = true;
    }
    if (__ballot(any) == 0ull) {                             // none follows: the NaN candidate itself, cvmax = NaN
      src = __ffsll((long long)__ballot(npos == lastnan)) - 1;
      cvmax = __builtin_nan(""); res = rl(nr, src); wsel = rl(nw, src); knext = __builtin_amdgcn_readlane(ncode, src);
      return;
    }
  }
  double v = av;
  int kk = apos;
  wave_argmax_first(v, kk);
  kk = uni(kk);
  cvmax = 0.0;
  if (kk < 0) return;                                        // nothing above 0: knext / res / wsel stay what they were
  src = __ffsll((long long)__ballot(apos == kk)) - 1;
  cvmax = rl(av, src); res = rl(ar, src); wsel = rl(aw, src); knext = __builtin_amdgcn_readlane(acode, src);
}

// qld.cpp:1861-1889
__device__ __forceinline__ int pick_drop_serial_reference(const QlView &q, int nact, double res, double &ratio) {
  int kdrop = -1;
  for (int k = 0; k < nact; ++k) {
    if (q.iact[k] <= q.me) continue;
    const double w = q.ww[k];
    if (res * w >= 0.0) continue;
    const double temp = q.lam[k] / w;
    if (kdrop >= 0 && fabs(temp) >= fabs(ratio)) continue;
    kdrop = k; ratio = temp;
  }
  return kdrop;
}

// Smallest 32-bit unsigned value of the wave, wave-uniform: the six steps of wg_wave.hpp's reductions (row_shr 1, 2, 4, 8, then
// row_bcast 15 and 31 fold the rows into lane 63) with the minimum taken BY the DPP instruction -- v_min_u32 is VOP2, a lane
// without a source keeps its value because destination and second operand are one register -- two instructions per step (the
// s_nop 1 is the two wait states between a VALU write and a DPP read of the same register, which the compiler does not count
// inside an asm statement) where update_dpp + min compiles to four: copy, s_nop, v_mov_dpp, v_min.  All 64 lanes must be active.
// The statement also hides the DPP from the compiler's hazard recogniser, and only the hazard above is padded by hand: a VALU
// write of EXEC right in front of it (v_cmpx, v_readlane into EXEC) would need five wait states before a DPP and would get two.
// Its callers sit in wave-uniform code behind a ballot, where EXEC is written by scalar instructions if at all; a caller inside
// divergent code generated with v_cmpx has to pad for itself.
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  asm("s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xf bank_mask:0xf"
      : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// Largest 32-bit unsigned value of the wave, wave-uniform: wave_min_u32 with v_max_u32 -- the same six steps, the same padding,
// the same conditions on its callers (all 64 lanes active, wave-uniform code).
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  asm("s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xf bank_mask:0xf"
      : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// The violation scan's selection among the lanes' candidates -- the largest value, the smallest order key among equal values --
// for candidates whose values are POSITIVE (every test of the scan that admits a candidate has `value <= 0` as a reason to skip)
// or a NaN, which takes part in no maximum (wave_argmax_first's v_max_f64 and its `v == vmax` leave a NaN out the same way).
// Positive doubles order as their bit patterns read as unsigned integers and equal values are equal patterns, so the maximum is
// two 32-bit maxima on the DPP path (high words, then the low words of the lanes that hold the largest high word), as in the
// ratio test above; the lanes that hold it come from one ballot, and only when there are several of them -- equal violations
// of two rows, rare -- does the smallest key need a reduction of its own.  A third of the vector instructions of the 64-bit
// maximum plus index minimum; the same lane for the same operands.  Returns the winning lane, or -1 without a candidate.
__device__ __forceinline__ int scan_select_lane(double v, int key) {
  const bool cand = key >= 0 && v > 0.0;
  const unsigned hi = cand ? (unsigned)__double2hiint(v) : 0u;
  const unsigned mh = wave_max_u32(hi);
  const bool top = cand && hi == mh;
  const unsigned lo = top ? (unsigned)__double2loint(v) : 0u;
  const unsigned ml = wave_max_u32(lo);
  const bool winl = top && lo == ml;
  const unsigned long long win = __ballot(winl);
  if (win == 0ull) return -1;
  int src = __ffsll((long long)win) - 1;
  if ((win & (win - 1ull)) != 0ull) {                       // several lanes hold the maximum: the smallest key among them
    const unsigned kmin = wave_min_u32(winl ? (unsigned)key : 0xffffffffu);
    src = __ffsll((long long)__ballot(winl && (unsigned)key == kmin)) - 1;
  }
  return src;
}

template <bool kOnePass = false, bool kNan = false>      // kOnePass: nact <= 64 known at compile time (n <= 64); kNan: see above
__device__ __forceinline__ int pick_drop(const QlView &q, int nact, double res, double &ratio, int lane) {
  double best = 0.0, bestt = 0.0;
  int bidx = -1;
  // operands that are no ordinary numbers (tested on the values this form loads anyway, consumed after it: nothing waits for
  // the test): the reference's own loop decides then (see above)
  bool bad = !wg_sane(res);
  if constexpr (kOnePass) {                                 // one multiplier per lane: selects instead of a lane-dependent loop
    const bool in = lane < nact;
    const int kc = in ? lane : 0;
    const double w = q.ww[kc];
    const int ia = q.iact[kc];
    const bool cand = in & (ia > q.me) & !(res * w >= 0.0);
    const double lamv = q.lam[kc];
    const double temp = lamv / w;
    if constexpr (kNan) {
      const bool bw = !wg_sane(w), bl = !wg_sane(lamv);    // plain values: the || below have nothing to short-circuit
      bad = bad || (in && (bw || bl));
      if (__ballot(bad) != 0ull) return uni(pick_drop_serial_reference(q, nact, res, ratio));
      // Every operand is an ordinary number here, so a candidate's quotient is one too, or an infinity (res * w < 0 leaves no
      // zero divisor): the smallest |temp| is the smallest bit pattern of |temp| read as an unsigned integer, and equal
      // magnitudes are equal patterns.  Two 32-bit minima on the DPP path (high words, then the low words of the lanes that
      // hold the smallest high word) and the first lane of one ballot -- the candidate's index IS its lane -- instead of a
      // 64-bit floating-point maximum and an index minimum: 30 vector instructions for 75, the same lane for the same operands.
      // This selection exists in the kNan form only, because only there the operands are known to be ordinary numbers: a build
      // with WG_TICK_NAN_EXACT = 0 or WG_NAN_REGIME = 0 (the A/B builds) takes the 64-bit reduction below, so an A/B of the
      // NaN regime also switches the ratio test's selection.
      const unsigned hi = cand ? ((unsigned)__double2hiint(temp) & 0x7fffffffu) : 0xffffffffu;
      const unsigned lo = (unsigned)__double2loint(temp);
      const unsigned mh = wave_min_u32(hi);
      const unsigned ml = wave_min_u32(hi == mh ? lo : 0xffffffffu);
      const unsigned long long win = __ballot(cand && hi == mh && lo == ml);
      if (win == 0ull) return -1;
      const int idx = __ffsll((long long)win) - 1;
      ratio = rl(temp, idx);
      return idx;
    }
    best = cand ? -fabs(temp) : 0.0; bestt = cand ? temp : 0.0; bidx = cand ? lane : -1;
  } else
  for (int k = lane; k < nact; k += 64) {
    const double w = q.ww[k], lamv = q.lam[k];
    if constexpr (kNan) {
      const bool bw = !wg_sane(w), bl = !wg_sane(lamv);
      bad = bad || bw || bl;
    }
    if (q.iact[k] <= q.me) continue;
    if (res * w >= 0.0) continue;
    double temp = lamv / w;
    double key = -fabs(temp);          // smaller |temp| wins, first index on ties
    if (bidx < 0 || key > best) { best = key; bestt = temp; bidx = k; }
  }
  if constexpr (kNan)
    if (__ballot(bad) != 0ull) return uni(pick_drop_serial_reference(q, nact, res, ratio));
  int idx = bidx;
  double v = best;
  wave_argmax_first(v, idx);
  idx = uni(idx);
  if (idx < 0) return -1;
  // fetch the winning lane's temp
  ratio = rl(bestt, idx & 63);
  return idx;
}

// qld.cpp:2039-2058 (lql): per-lane terms, then the sum in index order.
template <class P>
__device__ __forceinline__ double xmag_sum(const QlView &q, const P &prob, double vfact, int lane) {
  const int n = q.n;
  if constexpr (P::kNM > 0) {
    const int il = lane < n ? lane : n - 1;                 // surplus lanes compute lane n - 1's term and drop it
    const double xi = q.x[il];
    const double term = fabs(xi) * vfact * (fabs(q.d[il]) + fabs(prob.Gd(q, il) * xi));
    return ordered_sum_lds<P::kNM>(term, q.sc3, n, lane);
  }
  for (int i = lane; i < n; i += 64) {
    double xi = q.x[i];
    q.sc3[i] = fabs(xi) * vfact * (fabs(q.d[i]) + fabs(prob.Gd(q, i) * xi));
  }
  WG_WSYNC();
  double sum = 0.0;
  int i = 0;
  for (; i + 8 <= n; i += 8) {                              // loads in groups of eight ahead of the add chain
    double t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = q.sc3[i + e];
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += t[e];
  }
  for (; i < n; ++i) sum += q.sc3[i];
  return sum;
}

// The same terms for a policy with guarded sums (GuardedSumsOf; n <= kNM <= 64, one term per lane): added as a balanced tree over
// the lanes -- NOT the reference's order: the caller holds the result to wg_ql_guard.hpp's certificates -- or, `ordered`
// (wave-uniform), in index order by the rolled loop.
template <class P>
__device__ __forceinline__ double xmag_sum_guarded(const QlView &q, const P &prob, double vfact, int lane, bool ordered) {
  const int n = q.n;
  const int il = lane < n ? lane : n - 1;                   // surplus lanes compute lane n - 1's term and drop it
  const double xi = q.x[il];
  const double term = fabs(xi) * vfact * (fabs(q.d[il]) + fabs(prob.Gd(q, il) * xi));
  if (ordered) return ordered_sum_lds_rolled<P::kNM>(term, q.sc3, n, lane);
  return wave_sum_tree(lane < n ? term : 0.0);
}

// qld.cpp:1992-2030.  Three phases: (1) the chain of rotation norms; (2) ga/gb of every rotation, one lane
// each; (3) every lane carries its own row of Z through the whole rotation sequence.
// n <= 64: s[] and the rotation coefficients live in registers (lane c <-> column c) and are handed
// around with v_readlane, so the dependent chain of phase 1 contains no LDS access at all.
template <int GRP = 8, bool kWide = false>                 // kWide: 64 <= n <= 128 known at compile time (only that form is compiled)
__device__ __forceinline__ void sweep(const QlView &q, double *s, int nu, int nact, int lane) {
  const int n = q.n;
  if (nu - 1 <= nact) return;
  if (!kWide && n <= 64) {
    const double sreg = (lane < nu) ? s[lane] : 0.0;
    double myP = 0.0, myQ = 0.0, myN = 0.0;
    {
      double cur = rl(sreg, nu - 1);
      for (int c = nu - 1; c > nact; --c) {
        const double p = rl(sreg, c - 1);
        double nrm;
        if (cur == 0.0) { nrm = 0.0; cur = p; }
        else { nrm = givens_norm(p, cur); if (lane == c) { myP = p; myQ = cur; } cur = nrm; }
        if (lane == c) myN = nrm;
      }
    }
    double ga = 1.0, gb = 0.0;
    if (lane > nact && lane < nu && myN != 0.0) {
      ga = myP / myN;
      gb = myQ / myN;
      s[lane - 1] = myN;
    }
    {
      const int i = lane;
      const bool act = i < n;
      double carry = act ? Zm(i, nu - 1) : 0.0;
      double zl = act ? Zm(i, nu - 2) : 0.0;            // nu - 2 >= nact >= 0 here
      for (int c = nu - 1; c > nact; --c) {
        const double zn = (act && c - 2 >= nact) ? Zm(i, c - 2) : 0.0;   // prefetch for the next rotation
        const double nc = rl(myN, c);
        if (nc == 0.0) { if (act) Zm(i, c) = carry; carry = zl; }
        else {
          const double gac = rl(ga, c), gbc = rl(gb, c);
          const double t = gac * zl + gbc * carry;
          if (act) Zm(i, c) = gac * carry - gbc * zl;
          carry = t;
        }
        zl = zn;
      }
      if (act) Zm(i, nact) = carry;
    }
    WG_WSYNC();
    return;
  }
  // phase 1: the chain of norms, as in sweep_flat: ONE value per rotation is recorded (`cur` as it leaves rotation c, in
  // chain[c - 1]); p = s[c - 1] is fetched one rotation ahead, off the chain.  Phase 2 rebuilds each rotation from it:
  // sc0[c] = ga, sc1[c] = gb, sc2[c] = norm (0 marks "skipped").
  double *chain = q.sc3;
  WG_REP(3)
  if (sweep_range_ok(s, nact, nu, lane)) {                  // the usual case: the shorter norm, as in sweep_flat
    double cur = s[nu - 1];
    double pa = s[nu - 2], pb;
    int c = nu - 1;
    // operand and record through ONE index kept in a vector register (s may be LDS or, once a solve went on in the global slot,
    // global memory: the address space follows the caller, so an index, not a typed pointer): constant offsets in the loads and
    // stores, one v_add per pair of rotations instead of a clamp, a shift, an add and a move per access.  The operand fetched
    // ahead of the last rotation may lie one entry below s (nact = 0): inside the view's memory, never used.
    int iv = nu - 4;                                        // s[iv + 1] = s[c - 2], chain[iv + 2] = chain[c - 1]
    asm volatile("" : "+v"(iv));
    const int rots = c - nact;                              // >= 1: pairs in a counted loop with one exit, then the odd one (sweep_flat)
    if (WG_UBOOL(cur != 0.0)) {                             // cur stays non-zero: no select (see sweep_flat)
      for (int k = rots >> 1; k > 0; --k) {
        pb = s[iv + 1];
        cur = givens_norm_fast(pa, cur); chain[iv + 2] = cur;
        pa = s[iv];
        cur = givens_norm_fast(pb, cur); chain[iv + 1] = cur;
        iv -= 2;
      }
      if (rots & 1) { cur = givens_norm_fast(pa, cur); chain[iv + 2] = cur; }
    } else {
      for (int k = rots >> 1; k > 0; --k) {
        pb = s[iv + 1];
        { const double nrmc = givens_norm_fast(pa, cur); cur = (cur == 0.0) ? pa : nrmc; chain[iv + 2] = cur; }
        pa = s[iv];
        { const double nrmc = givens_norm_fast(pb, cur); cur = (cur == 0.0) ? pb : nrmc; chain[iv + 1] = cur; }
        iv -= 2;
      }
      if (rots & 1) { const double nrmc = givens_norm_fast(pa, cur); cur = (cur == 0.0) ? pa : nrmc; chain[iv + 2] = cur; }
    }
  } else {
    double cur = s[nu - 1];
    double p = s[nu - 2];
    for (int c = nu - 1; c > nact; --c) {
      const double p_next = s[(c - 2 >= 0) ? c - 2 : 0];
      const double nrmc = givens_norm(p, cur);
      cur = (cur == 0.0) ? p : nrmc;
      chain[c - 1] = cur;
      p = p_next;
    }
    WG_WSYNC();
  }
  bool any_skip = false;                                    // a skipped rotation (q == 0) is rare: phase 3 has a select-free form
  for (int c0 = nact + 1; c0 < nu; c0 += 64) {
    const int c = c0 + lane;
    const bool mine = c < nu;
    const int cc = mine ? c : nu - 1;
    const double P = s[cc - 1];
    const double Q = (cc == nu - 1) ? s[nu - 1] : chain[cc];
    const double Nn = (Q == 0.0) ? 0.0 : chain[cc - 1];
    any_skip = any_skip || (__ballot(mine && Nn == 0.0) != 0ull);
    WG_WSYNC();                                             // every lane has read s[] before any lane rewrites it
    if (mine) {
      q.sc2[c] = Nn;
      if (Nn != 0.0) {
        q.sc0[c] = P / Nn;   // ga
        q.sc1[c] = Q / Nn;   // gb
        s[c - 1] = Nn;
      }
    }
  }
  WG_WSYNC();
  if (kWide || n <= 128) {
    // phase 3 for 64 < n <= 128: two rows per lane in one pass.  Rotation c reads Z(i, c-1) BEFORE any rotation rewrites it,
    // so the row entries are independent of the carry chain: they are fetched a chunk of kSwC columns at a time, the next
    // chunk while the current one is rotated (two register sets, loop unrolled by two so that handing a set on is a renaming).
    // Everything inside a chunk is straight-line code -- no early exit between a load and its use, which is what lets the
    // compiler wait for exactly the loads it needs (with Z in global memory an exposed entry is an L2 round trip on the
    // carry chain; an earlier form with an exit test per rotation waited for ALL outstanding accesses at every step).
    // The first chunk takes the cnt % kSwC odd rotations; past-the-end addresses are clamped to column nact (loaded, unused).
    // Surplus lanes shadow their first row completely: same loads, same arithmetic, the same value stored to the same place.
    // The rotation coefficients of a chunk (LDS, broadcast reads) are fetched at the head of the chunk as well, so that no
    // step waits for an LDS round trip; when no rotation of the sweep is skipped (one ballot in phase 2) the steps run
    // without the selects.
    constexpr int kSwC = GRP;
    const int i0 = lane;
    // lanes without a second row all mirror row 64 when there is one (ONE address per load and per store -- the same value to the
    // same place as lane 0's second row -- instead of a second copy of the first set's 56); with n <= 64 they mirror their own first row
    const int i1 = lane + 64 < n ? lane + 64 : (n > 64 ? 64 : lane);
    const int ldz = q.ldz;
    double *z0 = q.Z + i0, *z1 = q.Z + i1;
    double carry0 = z0[(nu - 1) * ldz], carry1 = z1[(nu - 1) * ldz];
    struct Co { double ga[kSwC], gb[kSwC], nr[kSwC]; };
    auto coef = [&](Co &o, int c) {                          // coefficients of rotations c, c-1, .. (clamped: unused past the end)
#pragma unroll
      for (int k = 0; k < kSwC; ++k) {
        const int cc = (c - k) > nact ? (c - k) : nact + 1;
        o.ga[k] = q.sc0[cc]; o.gb[k] = q.sc1[cc]; o.nr[k] = q.sc2[cc];
      }
    };
    auto rows = [&](double (&p0)[kSwC], double (&p1)[kSwC], int c) {   // Z(i, c-1-k): the entries rotations c, c-1, .. read
#pragma unroll
      for (int k = 0; k < kSwC; ++k) {
        const int cc = (c - 1 - k) > nact ? (c - 1 - k) : nact;
        p0[k] = z0[cc * ldz]; p1[k] = z1[cc * ldz];
      }
    };
    auto step = [&](auto may_skip, int c, double zl0, double zl1, double ga, double gb, double nrm) {
      const double t0 = ga * zl0 + gb * carry0, w0 = ga * carry0 - gb * zl0;
      const double t1 = ga * zl1 + gb * carry1, w1 = ga * carry1 - gb * zl1;
      if constexpr (decltype(may_skip)::value) {
        const bool skip = (nrm == 0.0);
        z0[c * ldz] = skip ? carry0 : w0;
        z1[c * ldz] = skip ? carry1 : w1;
        carry0 = skip ? zl0 : t0;
        carry1 = skip ? zl1 : t1;
      } else {
        z0[c * ldz] = w0; z1[c * ldz] = w1;
        carry0 = t0; carry1 = t1;
      }
    };
    auto run = [&](auto may_skip) {
      int c = nu - 1;                                        // the next rotation
      {
        const int rem = (nu - 1 - nact) % kSwC;
        if (rem) {
          double h0[kSwC], h1[kSwC];
          Co hc;
          rows(h0, h1, c); coef(hc, c);
#pragma unroll
          for (int k = 0; k < kSwC - 1; ++k)
            if (k < rem) step(may_skip, c - k, h0[k], h1[k], hc.ga[k], hc.gb[k], hc.nr[k]);
          c -= rem;
        }
      }
      if (c > nact) {                                        // a whole number of chunks is left
        double a0[kSwC], a1[kSwC], b0[kSwC], b1[kSwC];
        Co cc;                                               // one set: read at the head of its chunk (one LDS wait per chunk)
        rows(a0, a1, c);
        for (;;) {
          rows(b0, b1, c - kSwC); coef(cc, c);
#pragma unroll
          for (int k = 0; k < kSwC; ++k) step(may_skip, c - k, a0[k], a1[k], cc.ga[k], cc.gb[k], cc.nr[k]);
          c -= kSwC;
          if (c <= nact) break;
          rows(a0, a1, c - kSwC); coef(cc, c);
#pragma unroll
          for (int k = 0; k < kSwC; ++k) step(may_skip, c - k, b0[k], b1[k], cc.ga[k], cc.gb[k], cc.nr[k]);
          c -= kSwC;
          if (c <= nact) break;
        }
      }
    };
    if (any_skip) run(std::true_type{}); else run(std::false_type{});
    z0[nact * ldz] = carry0;
    z1[nact * ldz] = carry1;
    WG_WSYNC();
    return;
  }
  if constexpr (!kWide)
  for (int i = lane; i < n; i += 64) {
    double carry = Zm(i, nu - 1);
    for (int c = nu - 1; c > nact; --c) {
      if (q.sc2[c] == 0.0) { Zm(i, c) = carry; carry = Zm(i, c - 1); continue; }
      double ga = q.sc0[c], gb = q.sc1[c];
      double zl = Zm(i, c - 1);
      double t = ga * zl + gb * carry;
      Zm(i, c) = ga * carry - gb * zl;
      carry = t;
    }
    Zm(i, nact) = carry;
  }
  WG_WSYNC();
}

// qld.cpp:1903-1982.  nu = number of R columns taking part (nact, or nact+1
// when the S column rides along).  Returns the new nact.
__device__ __forceinline__ int drop_constraint(const QlView &q, int kdrop, int nu, int nact, int lane) {
  const int n = q.n;
  if (lane == 0) {
    int code = q.iact[kdrop];
    int ia = code - 1;
    if (code > q.mn) ia -= n;
    q.wa[ia] = -q.wa[ia];
  }
  WG_WSYNC();
  for (int k = kdrop; k < nact - 1; ++k) {
    double ga, gb, nrm;
    givens(Rp(k, k + 1), Rp(k + 1, k + 1), ga, gb, nrm);   // redundant on all lanes
    WG_WSYNC();
    for (int i = lane; i <= k; i += 64) {
      double t = Rp(i, k + 1);
      Rp(i, k + 1) = Rp(i, k);
      Rp(i, k) = t;
    }
    WG_WSYNC();
    if (lane == 0) { Rp(k + 1, k + 1) = 0.0; Rp(k, k) = nrm; }
    WG_WSYNC();
    for (int c = k + 1 + lane; c < nu; c += 64) {
      double rk = Rp(k, c), rk1 = Rp(k + 1, c);
      double t = ga * rk + gb * rk1;
      Rp(k + 1, c) = ga * rk1 - gb * rk;
      Rp(k, c) = t;
    }
    for (int i = lane; i < n; i += 64) {
      double zk = Zm(i, k), zk1 = Zm(i, k + 1);
      double t = ga * zk + gb * zk1;
      Zm(i, k + 1) = ga * zk1 - gb * zk;
      Zm(i, k) = t;
    }
    if (lane == 0) { q.iact[k] = q.iact[k + 1]; q.lam[k] = q.lam[k + 1]; }
    WG_WSYNC();
  }
  return nact - 1;
}

// qld.cpp:1547-1658
template <class P>
__device__ __forceinline__ bool independent_coordinate(const QlView &q, const P &prob, int knext, int nact, double vsmall, int lane) {
  const int n = q.n, m = q.m;
  int k1 = 0;
  if (knext > m) { k1 = knext - m; if (k1 > n) k1 -= n; }
  bool found = false;
  for (int i = 1 + lane; i <= n; i += 64) {
    double suma;
    if (knext <= m) suma = Am(knext - 1, i - 1);
    else { suma = 0.0; if (i == k1) suma = (knext > q.mn) ? -1.0 : 1.0; }
    double sumb = fabs(suma);
    WG_UNROLL
    for (int k = 0; k < nact; ++k) {
      int kk = q.iact[k];
      double temp;
      if (kk <= m) temp = q.ww[k] * Am(kk - 1, i - 1);
      else {
        kk -= m; temp = 0.0;
        if (kk == i) temp = q.ww[kk - 1];
        kk -= n;
        if (kk == i) temp = -q.ww[kk - 1];
      }
      suma -= temp;
      sumb += fabs(temp);
    }
    if (knext <= m && suma <= vsmall) continue;
    if (significant(sumb, fabs(suma))) found = true;
  }
  return __any(found) != 0;
}

// Cholesky factor of G (qld.cpp:859-890) and Z = R^-1 (:937-975) for n <= NM <= 64 with one COLUMN of R / one ROW of Z per
// lane, in registers, the loops over rows and columns unrolled (compile-time register indices): entry (i, j) of the factor is
// temp = G(i, j) - sum_{k < i} R(k, j) R(k, i), k ascending -- lane j holds R(., j), R(k, i) comes from lane i's registers
// (v_readlane, both indices known at compile time) -- then R(i, j) = temp / R(i, i); row i of the inverse is
// Z(i, c) = -(sum_{k < c} Z(i, k) R(k, c)) / R(c, c), k ascending, with the exact zeros Z(i, k < i) = +0.0 left in (their
// products are +-0.0 and the sum, started from +0.0, does not move).  The same operations in the same order as the loops they
// replace, without their two LDS hand-overs per row: 27 k cycles instead of 240 k at n = 36.
// Returns false -- R and Z untouched -- when a pivot falls below vsmall: the caller then takes the generic path, which finds
// the same pivot and applies ql0002's diagonal shift.
template <int NM, class P>
__device__ __forceinline__ bool chol_inverse_regs(const QlView &q, const P &prob, double vsmall, int lane) {
  const int n = q.n;
  const int j = lane < n ? lane : n - 1;                    // surplus lanes shadow the last column / row
  double r[NM];
#pragma unroll
  for (int k = 0; k < NM; ++k) r[k] = 0.0;
  bool ok = true;
#pragma unroll
  for (int i = 0; i < NM; ++i) {
    if (i < n) {
      const int jj = j > i ? j : i;                         // finished columns (j < i) walk column i along: unused
      double temp = prob.G(q, i, jj);
#pragma unroll
      for (int k = 0; k < i; ++k) temp -= r[k] * rl(r[k], i);
      const double tpiv = rl(temp, i);
      ok = ok && !(tpiv < vsmall);
      const double rii = sqrt(tpiv);
      const double quo = temp / rii;
      r[i] = (j == i) ? rii : ((j > i) ? quo : r[i]);
    }
  }
  if (!WG_UBOOL(ok)) return false;
  if (lane < n) {
#pragma unroll
    for (int k = 0; k < NM; ++k)
      if (k <= j) Rf(k, j) = r[k];
  }
  WG_WSYNC();
  // ---- Z = R^-1: lane i owns row i ----
  const int i = j;
  double z[NM];
#pragma unroll
  for (int k = 0; k < NM; ++k) z[k] = 0.0;
  {
    double rdiag = 0.0;
#pragma unroll
    for (int k = 0; k < NM; ++k) rdiag = (k == i) ? r[k] : rdiag;     // R(i, i): the lane's own diagonal
    const double zd = 1.0 / rdiag;
#pragma unroll
    for (int k = 0; k < NM; ++k) z[k] = (k == i) ? zd : z[k];
  }
#pragma unroll
  for (int c = 1; c < NM; ++c) {
    if (c < n) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < c; ++k) sum += z[k] * Rf(k, c);
      const double zc = -sum / Rf(c, c);
      z[c] = (i < c) ? zc : z[c];
    }
  }
  if (lane < n) {
#pragma unroll
    for (int k = 0; k < NM; ++k)
      if (k < n) Zm(i, k) = z[k];
  }
  WG_WSYNC();
  return true;
}

// ---- blocks of ql_solve's main loop ----
// add the new constraint, :1764-1771 (one lane)
__device__ __forceinline__ void ql_activate(const QlView &q, int nact, int knext, double parnew, double wsel, int lane, int n, int mn) {
  if (lane == 0) {
    q.lam[nact] = parnew;
    q.iact[nact] = knext;
    int ia = knext - 1;
    if (knext > mn) ia -= n;
    q.wa[ia] = -wsel;                                   // = -wa[ia]: a store, not a read-modify-write
  }
}
// ql0001 epilogue, :497-608: ql0002's info as the caller's ifail
__device__ __forceinline__ int ql_ifail_of(int info) {
  int ifail = 0;
  if (info == 1) ifail = 1;
  else if (info == 2) ifail = 2;
  else if (info < 0) ifail = -info + 10;
  return ifail;
}

}  // namespace wg
