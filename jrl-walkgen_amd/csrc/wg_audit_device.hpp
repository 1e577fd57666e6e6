// wg_audit_device.hpp -- the walk audit of a fleet on the device: for every sample of every gait, the ZMP's margin inside the
// polytope its gait's queue holds at that time, reduced to one wg_zmp_audit_t per gait.
//
//   wg_zmp_audit_kernel<kRes>           every (gait, chunk of kFcChunk samples) lane audits its samples into a partial result
//   wg_zmp_audit_combine_kernel<kRes>   one lane per gait folds its chunks' partial results, in chunk order, into audit[b]
//       ZMPConstrainedQPFastFormulation::ValidationConstraints    ZMPConstrainedQPFastFormulation.cpp:248-381 (the test at :322)
//       ZMPConstrainedQPFastFormulation::BuildConstraintMatrices  :785-796 (the entry search)
//   <false> wg_zmp_audit_dev: the samples [0, length[b]);  <true> wg_zmp_audit_append_dev: the samples [done[b], length[b])
//
// The layout is wg_footcons_kernel's, for its reason: the tracks are time-major ([sample][gait], pitch apart), so lanes are
// gaits -- every row a wave reads is one contiguous line -- and the time axis is split across blocks, grid = (gait groups of
// 64) x (chunks), because one lane walking all 2-10 k samples of its gait is 64 waves on 1024 SIMDs.  A sample's verdict depends
// on that sample and the queue alone, so the chunks are independent; what is not independent is WHICH sample is the first to
// attain the least margin, and that is why the chunks do not meet in atomics: each leaves a wg_zmp_audit_t in a buffer of the
// context ([chunk][gait]) and the second kernel folds them in ascending chunk order.  The result does not depend on the grid.
// A lane bisects its gait's queue once, for its first sample, then steps forward (au_seek); it keeps the current entry's rows
// and their norms in registers (AuRows, 32 doubles), loaded once per entry change -- a support phase lasts on the order of a
// hundred samples, so the 248-byte strided read of an entry is rare next to the two coalesced loads per sample.
// The arithmetic is wg_audit_math.hpp, which the host call compiles too: the same bytes.
// Nothing at or past length[b] is read or written; a refused gait gets its status and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include "wg_audit_math.hpp"
#include "wg_footcons_device.hpp"

namespace wg {

struct AuIn {
  int B, lcap;
  const int *length;                     // B
  const double *time;                    // lcap, shared
  const double *px, *py;                 // sample k of gait b at [k * pitch + b]
  long long pitch;
  int qcap;
  const wg_zmp_polytope_t *queues;       // [B][qcap]
  const double *t_start, *t_end;         // [B][qcap]
  const int *count;                      // B
};
// what the append form adds
struct AuRes {
  int *done;                             // B, in/out: length[b] after the call (written by the combine kernel alone)
  int first_sample;                      // the host-side lower bound on every done[b]
  int chunk0;                            // the launch's first chunk (first_sample / kFcChunk): blockIdx.y counts from there
};

constexpr int kAuRefused = -1, kAuSitsOut = -2;

// Both kernels ask this of a gait: its first sample to audit, kAuRefused or kAuSitsOut; len is its length.  Neither kernel
// writes what the other one's answer depends on before that one has run (done[b] and audit[b] belong to the combine kernel).
template <bool kRes>
__device__ __forceinline__ int au_admit(const AuIn &I, const AuRes &Z, const wg_zmp_audit_t *audit, int b, int &len) {
  len = I.length[b];
  const int cb = I.count[b];
  if (len < 0 || len > I.lcap || cb < 0) return kAuRefused;
  if constexpr (kRes) {
    const int d = Z.done[b];
    if (d < 0 || d > len || d < Z.first_sample) return kAuRefused;
    if (d > 0 && audit[b].status != WG_OK) return kAuRefused;       // an earlier refusal: sticky until done[b] == 0 restarts
    if (d == len) return kAuSitsOut;
    return d;
  }
  return 0;
}

template <bool kRes>
__global__ void __launch_bounds__(64)
wg_zmp_audit_kernel(AuIn I, AuRes Z, const wg_zmp_audit_t *__restrict__ audit, wg_zmp_audit_t *__restrict__ part /* [chunks][B] */,
                    double *__restrict__ margin_tm /* [lcap][B] or null */) {
  const int b = blockIdx.x * 64 + threadIdx.x, crel = blockIdx.y;
  if (b >= I.B) return;
  int len;
  const int from = au_admit<kRes>(I, Z, audit, b, len);
  if (from < 0) return;
  const size_t sB = (size_t)I.B;
  const int i0 = (crel + (kRes ? Z.chunk0 : 0)) * kFcChunk;
  const int n = len - i0 < kFcChunk ? len - i0 : kFcChunk;           // samples of this chunk (<= 0: past the gait's end)
  const int k0 = from > i0 ? from - i0 : 0;                          // the first of them that is new
  if (n <= k0) return;                                               // nothing to audit here: the combine kernel does not read it
  const int cb = I.count[b], K = cb < I.qcap ? cb : I.qcap;
  const double *ts = I.t_start + (size_t)b * I.qcap, *te = I.t_end + (size_t)b * I.qcap;
  const wg_zmp_polytope_t *Q = I.queues + (size_t)b * I.qcap;
  wg_zmp_audit_t A = au_empty();
  AuCursor c;
  au_place(ts, te, K, au_lower_bound(te, K, I.time[i0 + k0]), c);
  AuRows R;
  R.nrows = 0;
  int loaded = -1;
  for (int k = k0; k < n; k++) {
    const size_t i = (size_t)(i0 + k);
    const double t = I.time[i];
    const double x = I.px[i * (size_t)I.pitch + b], y = I.py[i * (size_t)I.pitch + b];
    const bool covered = au_seek(ts, te, K, t, c);
    if (covered && c.q != loaded) {
      au_load(Q + c.q, R);
      loaded = c.q;
    }
    const double m = au_sample(R, covered, x, y, i0 + k, A);
    if (margin_tm) margin_tm[i * sB + b] = m;
  }
  part[(size_t)crel * sB + b] = A;
}

template <bool kRes>
__global__ void __launch_bounds__(256)
wg_zmp_audit_combine_kernel(AuIn I, AuRes Z, const wg_zmp_audit_t *__restrict__ part, wg_zmp_audit_t *audit) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= I.B) return;
  int len;
  const int from = au_admit<kRes>(I, Z, audit, b, len);
  if (from == kAuRefused) audit[b].status = WG_ERR_BAD_ARG;           // done[b] and every other field stay
  if (from < 0) return;
  wg_zmp_audit_t A = au_empty();
  if (kRes && from > 0) A = audit[b];
  if (len > from) {
    const int c0 = kRes ? Z.chunk0 : 0;
    for (int c = from / kFcChunk; c <= (len - 1) / kFcChunk; c++) au_fold(A, part[(size_t)(c - c0) * (size_t)I.B + b]);
  }
  A.status = WG_OK;
  audit[b] = A;
  if constexpr (kRes) Z.done[b] = len;
}

}  // namespace wg
