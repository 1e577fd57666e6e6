// wg_footcons_device.hpp -- the Dimitrov-2008 pipeline between the feet trajectories and the tick, on the device:
//
//   wg_footcons_kernel<kBuild, kRes>   polytope queues of B feet trajectories: <false / true, false> the whole trajectories
//                                      (wg_foot_constraints_batch_dev), <false / true, true> behind wg_footcons_resume_kernel the
//                                      samples that arrived since the last call (wg_foot_constraints_append_dev)
//                                      <.., .., true> the same with a sole per gait (wg_foot_constraints_fleet_dev, _append_fleet_dev)
//       FootConstraintsAsLinearSystem::BuildLinearConstraintInequalities  src/Mathematics/FootConstraintsAsLinearSystem.cpp:258-539
//       ComputeLinearSystem :97-256, FindSimilarConstraints :55-92, ComputeConvexHull::DoComputeConvexHull ConvexHull.cpp:88-203
//   wg_dimitrov_select_kernel          the queue walk of one tick (wg_dimitrov_select_polys_dev, wg_dimitrov_walk_dev)
//   wg_dimitrov_follow_select_kernel   the same per gait, at the gait's own clock, where its own queue allows (wg_dimitrov_follow_dev)
//       ZMPConstrainedQPFastFormulation::BuildConstraintMatrices  ZMPConstrainedQPFastFormulation.cpp:785-796, 822-835
//
// Queues.  The host call (wg_footcons.cpp) walks one gait sample by sample.  Here the inputs are the time-major arrays
// wg_zmpdisc_full_batch_dev writes ([sample][component][gait]): lanes are gaits, so that every row a wave reads is one 512-byte
// line, and the time axis is split across blocks -- grid = (gait groups of 64) x (chunks of kFcChunk samples) -- because one
// lane walking all 2-3 k samples of its gait is 64 waves on 1024 SIMDs with one dependent load after the other.  What makes
// the split possible: the support state of a sample depends on that sample alone (left stepType, left z, right z), except
// when none of the reference's three tests holds (a z exactly at the lifting threshold), where it keeps its predecessor's.
//   pass 1 (kBuild = false)  every lane classifies the samples of its chunk (independent loads, 2 bits each, kept in two
//                            registers), classifies the sample before the chunk for the boundary test (walking back while
//                            that one inherits) and counts the support changes: cnt[chunk][gait], and their sum into count[gait];
//   pass 2 (kBuild = true)   the counts of the earlier chunks give the queue position of the chunk's first polytope; the lane
//                            walks its codes again and builds a polytope at every change.  The hull (Graham scan over the 8
//                            sole corners, in the reference's std::set order) runs in that one lane on points kept in LDS laid
//                            out [slot][lane] (runtime-indexed, so not in registers; conflict-free).
// Every entry of the queue has exactly one writer: polytope q and t_start[q] the lane that finds change q, t_end[q] the lane
// that finds change q + 1, the last t_end the lane whose chunk holds the gait's last sample.  Nothing past length[b] is read.
// Resumed (kRes): the same two passes over the samples [done[b], length[b]) alone.  An entry is final once written, except the last
// one's t_end, which the next call overwrites once -- with the time of the first new change (the lane that finds it, as above) or
// with the new last sample's.  count[b] on entry is the queue position of the first new change; pass 1's atomics change it, so
// wg_footcons_resume_kernel leaves it, and done[b], behind the per-chunk counts where both passes read them.
// The geometry -- classification, corners, hull, half planes, the polytope fill -- is wg_footcons_geom.hpp, which the host call
// compiles too: the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "wg_footcons_geom.hpp"

namespace wg {

constexpr int kFcChunk = 64;             // samples per (gait, chunk) lane: 2 bits of support state each in two 64-bit registers

struct FcIn {
  int B, lcap;
  const int *length;                     // B
  const double *time;                    // lcap, shared
  const double *left, *right;            // [lcap][6][B]
  const int *ltype;                      // [lcap][B]
  double hw, hh;                         // half sole minus the margins
};
struct FcOut {
  int qcap;
  wg_zmp_polytope_t *queues;             // [B][qcap]
  double *t_start, *t_end;               // [B][qcap]
  int *count;                            // B, zeroed before pass 1
};

// what a resumed call (wg_foot_constraints_append_dev) adds: where each gait resumes, snapshot by wg_footcons_resume_kernel before
// pass 1's atomics change count[b]
struct FcRes {
  const int *from;                       // B: the first new sample (done[b] on entry), or -1: the gait sits out or was refused
  const int *base;                       // B: count[b] on entry (0 for a gait that starts), the queue position of the first new change
  int *done;                             // B, in/out: length[b] after the call
  int chunk0;                            // the launch's first chunk (first_sample / kFcChunk): blockIdx.y counts from there
};

// Before the two passes of a resumed call, one lane per gait: refuse or admit, and keep done[b] / count[b] as they were on entry
// where both passes read them (neither is read again: pass 1 adds to count[b], pass 2's closing lane writes done[b]).
__global__ void __launch_bounds__(256)
wg_footcons_resume_kernel(int B, int lcap, int first_sample, const int *__restrict__ length, const int *__restrict__ done,
                          int *__restrict__ count, int *__restrict__ from, int *__restrict__ base) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int len = length[b], d = done[b];
  const int c = d > 0 ? count[b] : 0;                     // a gait that starts ignores what count[b] holds
  int f = -1;
  if (len < 0 || len > lcap || d < 0 || d > len || d < first_sample || c < 0) {
    count[b] = WG_ERR_BAD_ARG;                            // refused (an earlier error included: sticky); done[b] and the queue stay
  } else if (d < len) {
    f = d;
    if (d == 0) count[b] = 0;
  }                                                       // else length[b] == done[b]: sits the call out, nothing is touched
  from[b] = f;
  base[b] = c;
}

// kRes = false: the whole trajectory, wg_foot_constraints_batch_dev (Z is not read).  kRes = true: the samples from Z.from[b] on.
// The chunks stay ABSOLUTE (chunk c is samples [c kFcChunk, (c + 1) kFcChunk) of every gait), so the rows a wave reads are whole
// lines however the lanes' resume points differ; a lane skips the samples of its chunk below its own.  The state before a lane's
// first new sample is found like the state before a chunk, walking back while the predecessor inherits -- across the resume point
// and across chunks: the feet arrays hold the whole walk, nothing is carried from call to call but done[b] and count[b].
// kFleet = false: the half sole minus the margins is the launch's, I.hw / I.hh (S is empty).  kFleet = true
// (wg_foot_constraints_fleet_dev, _append_fleet_dev): the gait's own, made in its lane from S.soles[b] with the launcher's expression.
// The kernel text is one; the fleet form is a third template argument, off by default, and its one argument rides behind the
// others in a struct that is empty without it: wg_footcons_kernel<kBuild, kRes> stays the kernel it was.
template <bool kFleet>
struct FcSoles {};
template <>
struct FcSoles<true> {
  const wg_sole_t *soles;                // B
};

template <bool kBuild, bool kRes, bool kFleet = false>
__global__ void __launch_bounds__(64)
wg_footcons_kernel(FcIn I, FcOut Q, int *__restrict__ cnt /* [chunks][B] */, FcRes Z, FcSoles<kFleet> S) {
  __shared__ double fc_lds[kBuild ? kFcSlots * 2 * 64 : 1];
  const int lane = threadIdx.x, b = blockIdx.x * 64 + lane;
  int chunk = blockIdx.y, crel = blockIdx.y;              // absolute, and as cnt is indexed
  if constexpr (kRes) chunk += Z.chunk0;
  if (b >= I.B) return;
  const size_t sB = (size_t)I.B;
  const int len = I.length[b], i0 = chunk * kFcChunk;
  int from = 0, cfirst = 0;                               // the first new sample, and its chunk as cnt is indexed
  if constexpr (kRes) {
    from = Z.from[b];
    if (from < 0) return;                                 // sits out or refused: wg_footcons_resume_kernel has said so
    cfirst = from / kFcChunk - Z.chunk0;
  } else if (len < 0 || len > I.lcap) {                   // a gait wg_zmpdisc_* refused (or a length the arrays cannot hold): the
    if (!kBuild) {                                        // host call's answer to n < 0
      cnt[(size_t)chunk * sB + b] = 0;
      if (chunk == 0) Q.count[b] = WG_ERR_BAD_ARG;
    }
    return;
  }
  const int n = len - i0 < kFcChunk ? len - i0 : kFcChunk;         // samples of this chunk (<= 0: past the gait's end)
  const int k0 = kRes && from > i0 ? from - i0 : 0;                // the first of them that is new
  if constexpr (kRes)
    if (n <= k0) return;                                  // nothing new here (neither pass reads cnt of such a chunk)
  int own = 0;
  if (kBuild) {
    own = n > 0 ? cnt[(size_t)crel * sB + b] : 0;
    if (own == 0 && !(n > 0 && i0 + n == len)) return;    // no change in this chunk, and not the one that closes the queue
  }
  // support state of every sample of the chunk, 2 bits each: the loads do not depend on one another
  unsigned long long code_lo = 0, code_hi = 0;
  if (!kBuild || own > 0) {
#pragma unroll 8
    for (int k = 0; k < kFcChunk; k++) {
      unsigned long long s = 0;
      if (k < n && (!kRes || k >= k0)) {
        const size_t i = (size_t)(i0 + k);
        s = (unsigned long long)fc_classify(I.ltype[i * sB + b], I.left[(i * 6 + 2) * sB + b], I.right[(i * 6 + 2) * sB + b]);
      }
      if (k < 32) code_lo |= s << (2 * k);
      else code_hi |= s << (2 * (k - 32));
    }
  }
  // the state before the first new sample: its predecessor's, walking back while that one inherits; sample 0 inherits DOUBLE_SUPPORT
  int state = kFcDouble;
  if (n > 0 && i0 + k0 > 0 && (!kBuild || own > 0)) {
    for (int j = i0 + k0 - 1; j >= 0; j--) {
      const size_t i = (size_t)j;
      const int s = fc_classify(I.ltype[i * sB + b], I.left[(i * 6 + 2) * sB + b], I.right[(i * 6 + 2) * sB + b]);
      if (s != kFcInherit) { state = s; break; }
    }
  }
  int q = 0;                                              // queue position of this chunk's first change
  if (kBuild) {
    if constexpr (kRes) q = Z.base[b];
    for (int c = cfirst; c < crel; c++) q += cnt[(size_t)c * sB + b];
  }
  const FcPts<64> P{fc_lds + lane};
  double hw = I.hw, hh = I.hh;
  if constexpr (kFleet && kBuild) {
    const wg_sole_t sole = S.soles[b];
    hw = sole.sole_w * 0.5; hh = sole.sole_h * 0.5;
    hh -= sole.constraint_y;
    hw -= sole.constraint_x;
  }
  int found = 0;
  for (int k = k0; k < n; k++) {
    if (kBuild && found == own) break;
    const int s = (int)(((k < 32 ? code_lo >> (2 * k) : code_hi >> (2 * (k - 32)))) & 3);
    const int next = s == kFcInherit ? state : s;
    const bool fresh = (i0 + k == 0) || next != state;
    state = next;
    if (!fresh) continue;
    if (kBuild) {
      const size_t i = (size_t)(i0 + k);
      const double t = I.time[i];
      if (q > 0 && q - 1 < Q.qcap) Q.t_end[(size_t)b * Q.qcap + q - 1] = t;       // resumed: may be an earlier call's last entry
      if (q < Q.qcap) {
        const double *L = I.left + i * 6 * sB + b, *R = I.right + i * 6 * sB + b;
        const double lx = L[0], ly = L[sB], lz = L[2 * sB], lth = L[3 * sB], rx = R[0], ry = R[sB], rz = R[2 * sB], rth = R[3 * sB];
        int nh = 4;
        if (state == kFcDouble) {
          fc_corners(P, 0, lx, ly, lth, hw, hh);
          fc_corners(P, 4, rx, ry, rth, hw, hh);
          nh = fc_hull8(P);
        } else if (lz < rz) {
          fc_corners(P, 0, lx, ly, lth, hw, hh);
        } else {
          fc_corners(P, 0, rx, ry, rth, hw, hh);
        }
        if (!fc_polytope(P, nh, Q.queues + (size_t)b * Q.qcap + q)) atomicMin(Q.count + b, WG_ERR_BAD_ARG);
        Q.t_start[(size_t)b * Q.qcap + q] = t;
      }
      q++;
    }
    found++;
  }
  if (!kBuild) {
    cnt[(size_t)crel * sB + b] = found;
    if (found) atomicAdd(Q.count + b, found);
  } else if (n > 0 && i0 + n == len) {                    // the lane whose chunk holds the gait's last sample
    if (q > 0 && q - 1 < Q.qcap) Q.t_end[(size_t)b * Q.qcap + q - 1] = I.time[len - 1];    // the last polytope holds until then
    if constexpr (kRes) Z.done[b] = len;
  }
}

// ---- the queue walk of one tick ------------------------------------------------------------------------------------------
// One wave per gait, four to a block.  The first entry whose interval holds t0 is found by all lanes at once (ballot); the walk
// over the N previewed instants is a chain of N compares on wave-uniform operands, lane i keeps instant i's entry; then the
// N x 248 bytes are copied as 8-byte words, lane after lane: the stores of a wave are whole lines, the loads 248-byte runs.
// A gait whose t0 lies in no interval, or whose walk passes its last entry, keeps its LAST polytope (at rest on its final support,
// the convention of wg_zmpdisc_batch_dev past a gait's length) and is reported in ran_out; no entries: zeros.
constexpr int kPolyWords = (int)(sizeof(wg_zmp_polytope_t) / 8);
static_assert(sizeof(wg_zmp_polytope_t) == 248 && kPolyWords * 8 == (int)sizeof(wg_zmp_polytope_t), "wg_zmp_polytope_t: 31 words");

// the search, the walk and the copies of gait b at t0, by its wave: what wg_dimitrov_select_kernel and the follow form below share
__device__ __forceinline__ void dimitrov_select_gait(int lane, int b, int cb, int qcap, const wg_zmp_polytope_t *__restrict__ queues,
                                                     const double *__restrict__ t_start, const double *__restrict__ t_end, double t0,
                                                     int N, double T, wg_zmp_polytope_t *__restrict__ polys, int *ran_out, int sticky) {
  const int k = cb < qcap ? cb : qcap;
  const double *ts = t_start + (size_t)b * qcap, *te = t_end + (size_t)b * qcap;
  int q = k, ran = 0, mine = 0;
  for (int base = 0; base < k && q == k; base += 64) {
    const int c = base + lane;
    const bool hit = c < k && ts[c] <= t0 && t0 <= te[c];
    const unsigned long long m = __ballot(hit);
    if (m) q = base + __ffsll((long long)m) - 1;
  }
  if (k <= 0 || q == k) {
    ran = 1;
    mine = k - 1;
  } else {
    for (int i = 0; i < N; i++) {
      if (t0 + i * T > te[q]) {                           // the reference's StartingTime + i * T against EndingTime
        q++;
        if (q == k) { q = k - 1; ran = 1; }
      }
      if (lane == i) mine = q;
    }
  }
  const unsigned long long *src = reinterpret_cast<const unsigned long long *>(queues + (size_t)b * qcap);
  unsigned long long *dst = reinterpret_cast<unsigned long long *>(polys + (size_t)b * N);
  const int words = N * kPolyWords;
  for (int base = 0; base < words; base += 64) {          // wave-uniform trip count: every lane takes part in the shuffle
    const int w = base + lane, inst = (w < words ? w : words - 1) / kPolyWords, word = w - inst * kPolyWords;
    const int e = __shfl(mine, inst);
    if (w < words) dst[w] = k > 0 ? src[(size_t)e * kPolyWords + word] : 0ull;
  }
  if (ran_out && lane == 0 && (ran || !sticky)) ran_out[b] = ran;
}

__global__ void __launch_bounds__(256)
wg_dimitrov_select_kernel(int B, int qcap, const wg_zmp_polytope_t *__restrict__ queues, const double *__restrict__ t_start,
                          const double *__restrict__ t_end, const int *__restrict__ count, double t0, int N, double T,
                          wg_zmp_polytope_t *__restrict__ polys, int *ran_out, int sticky) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  dimitrov_select_gait(lane, b, count[b], qcap, queues, t_start, t_end, t0, N, T, polys, ran_out, sticky);
}

// ---- the queue walk of one round of wg_dimitrov_follow_dev ------------------------------------------------------------------
// The same layout, with a clock and a tick count per gait.  Every operand of the decision is wave-uniform (the wave's own gait):
// the wave reads ticks[b], count[b], have[b], clock[b], the time of its last sample and, unless every queue is final, three ints
// of its walk's state, and either goes -- selects at t = clock[b], leaves the row of outs its tick writes in row[b], advances
// clock[b] by the walk's own addition and ticks[b] by one -- or leaves row[b] = -1 and touches nothing else of the gait (a refusal
// writes ticks[b] as well).  An idle gait costs these loads and one store.
//   sits out   ticks[b] < 0 (sticky), count[b] <= 0, have[b] <= 0, ticks[b] == tick_cap, or a queue that is neither final nor
//              covers the tick's last instant: clock[b] + (N - 1) T <= time[have[b] - 1], the expression t0 + i * T of the walk
//              above at i = N - 1
//   refused    (tested behind the first three) ticks[b] > tick_cap, have[b] > lcap, a clock that is not finite
__global__ void __launch_bounds__(256)
wg_dimitrov_follow_select_kernel(int B, int qcap, const wg_zmp_polytope_t *__restrict__ queues, const double *__restrict__ t_start,
                                 const double *__restrict__ t_end, const int *__restrict__ count, int lcap,
                                 const double *__restrict__ time, const int *__restrict__ have,
                                 const wg_zmpdisc_state_t *__restrict__ walk, int all_final, double *clock, int *ticks, int tick_cap,
                                 int N, double T, wg_zmp_polytope_t *__restrict__ polys, int *ran_out, int *__restrict__ row) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int tk = ticks[b], cb = count[b], hv = have[b];
  int r = -1;
  if (tk >= 0 && cb > 0 && hv > 0) {
    const double t = clock[b];
    if (tk > tick_cap || hv > lcap || !(fabs(t) <= 1.7976931348623157e308)) {
      if (lane == 0) ticks[b] = WG_ERR_BAD_ARG;
    } else if (tk < tick_cap) {
      bool go = all_final != 0;
      if (!go && walk) go = walk[b].ended && !walk[b].error && walk[b].n_samples == hv;
      if (!go) go = t + (N - 1) * T <= time[hv - 1];
      if (go) {
        dimitrov_select_gait(lane, b, cb, qcap, queues, t_start, t_end, t, N, T, polys, ran_out, 1);
        r = tk;
        if (lane == 0) {
          clock[b] = t + T;
          ticks[b] = tk + 1;
        }
      }
    }
  }
  if (lane == 0) row[b] = r;
}

}  // namespace wg
