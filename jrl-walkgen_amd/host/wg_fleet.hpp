// wg_fleet.hpp -- what the fleet programs (kajita_fleet, dimitrov_fleet, fleet_bench, latency_b1) share: the error-exit macros,
// checked device allocations, the checksum, the feeding plan of the --online modes and the command lists of the --plan modes.  Header-only host code: no kernels, and
// nothing here touches the GPU before the program calls it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/wg_mpc.h"

#define CHECK_HIP(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "FAILED: %s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)
#define CHECK_WG(e) do { int r_ = (e); if (r_ != WG_OK) { fprintf(stderr, "FAILED: %s: %s\n", #e, wg_last_error()); return 1; } } while (0)

namespace wg_fleet {

// n elements of device memory (at least one, so that an empty array still has an address); for CHECK_HIP
template <class T>
inline hipError_t dev_alloc(T **p, size_t n) {
  return hipMalloc((void **)p, sizeof(T) * (n ? n : 1));
}

// a device copy of v
template <class T>
inline hipError_t dev_upload(T **p, const std::vector<T> &v) {
  const hipError_t e = dev_alloc(p, v.size());
  return e != hipSuccess ? e : hipMemcpy(*p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice);
}

// FNV-1a, 64 bit
inline uint64_t fnv1a64(const void *data, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char *p = static_cast<const unsigned char *>(data);
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

// The walk audit of a fleet program (--audit): the verdicts' device array, their host copy, and the report.  The programs launch
// wg_zmp_audit_dev / _append_dev themselves, on their own stream behind the calls that made the tracks and the queues.
struct FleetAudit {
  wg_zmp_audit_t *d_audit = nullptr;     // [B]
  std::vector<wg_zmp_audit_t> audit;     // the verdicts, once report() has run
  int worst_gait = -1, best_gait = -1;   // the gaits of the fleet's least and largest margin (-1: every gait was refused)
  long long violated = 0;
};

// After the stream was synchronised: copies the verdicts back, holds gaits 0 and B - 1 to the host twin (wg_zmp_audit on the
// copied-back track and queue; the track is read in place through its pitch) and prints the fleet's verdict.  All d_ pointers are
// the device arrays the audit call was given; len_h, time_h their host copies.  Returns 0, or 1 after printing FAILED.
inline int audit_report(const char *prog, const char *what, FleetAudit *fa, int B, int lcap, const int *len_h, const double *time_h,
                        const double *d_px, const double *d_py, long long pitch, int qcap, const wg_zmp_polytope_t *d_queues,
                        const double *d_ts, const double *d_te, const int *d_count) {
  fa->audit.resize(B);
  CHECK_HIP(hipMemcpy(fa->audit.data(), fa->d_audit, sizeof(wg_zmp_audit_t) * B, hipMemcpyDeviceToHost));
  const size_t span = (size_t)(lcap - 1) * (size_t)pitch + (size_t)B;
  std::vector<double> hx(span), hy(span), ts(qcap), te(qcap);
  std::vector<wg_zmp_polytope_t> q(qcap);
  CHECK_HIP(hipMemcpy(hx.data(), d_px, sizeof(double) * span, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hy.data(), d_py, sizeof(double) * span, hipMemcpyDeviceToHost));
  for (int g : {0, B - 1}) {
    int count = 0;
    CHECK_HIP(hipMemcpy(&count, d_count + g, sizeof(int), hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(q.data(), d_queues + (size_t)g * qcap, sizeof(wg_zmp_polytope_t) * qcap, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(ts.data(), d_ts + (size_t)g * qcap, sizeof(double) * qcap, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(te.data(), d_te + (size_t)g * qcap, sizeof(double) * qcap, hipMemcpyDeviceToHost));
    wg_zmp_audit_t twin;
    memset(&twin, 0, sizeof twin);
    const int rc = wg_zmp_audit(0, len_h[g], time_h, hx.data() + g, hy.data() + g, (int)pitch, count, qcap, q.data(), ts.data(), te.data(), &twin, nullptr);
    if (rc != WG_OK || memcmp(&twin, &fa->audit[g], sizeof twin)) {
      fprintf(stderr, "FAILED: the device audit of gait %d (%s) differs from the host twin: margin %.17g at %d vs %.17g at %d\n", g, what,
              fa->audit[g].margin, fa->audit[g].worst_sample, twin.margin, twin.worst_sample);
      return 1;
    }
  }
  fa->worst_gait = fa->best_gait = -1;
  fa->violated = 0;
  long long uncovered = 0, refused = 0;
  for (int g = 0; g < B; ++g) {
    const wg_zmp_audit_t &a = fa->audit[g];
    if (a.status != WG_OK) { ++refused; continue; }
    fa->violated += a.n_violated;
    uncovered += a.n_uncovered;
    if (fa->worst_gait < 0 || a.margin < fa->audit[fa->worst_gait].margin) fa->worst_gait = g;
    if (fa->best_gait < 0 || a.margin > fa->audit[fa->best_gait].margin) fa->best_gait = g;
  }
  if (fa->worst_gait < 0) { fprintf(stderr, "FAILED: the audit refused every gait (%s)\n", what); return 1; }
  const wg_zmp_audit_t &w = fa->audit[fa->worst_gait];
  printf("%s: audit of %s: least margin %.6f m (gait %d at t = %.3f s, row %d); %lld samples violated, %lld uncovered, %lld gaits refused; "
         "largest least margin %.6f m (gait %d); gaits 0 and %d == host twin\n", prog, what, w.margin, fa->worst_gait,
         w.worst_sample >= 0 ? time_h[w.worst_sample] : 0.0, w.worst_row, fa->violated, uncovered, refused, fa->audit[fa->best_gait].margin,
         fa->best_gait, B - 1);
  return 0;
}

// The feeding plan of a fleet walked on line: wg_zmpdisc_begin_dev takes the first two steps of every gait (call 0), each of
// the n_calls wg_zmpdisc_append_dev calls behind it the next K.  Host arithmetic, done once: nothing is read back while the
// fleet walks.
struct OnlinePlan {
  int n_calls = 0;
  std::vector<wg_rel_step_t> chunks;     // [n_calls][B][K]: the steps after the first two, regrouped call by call
  std::vector<int> cns;                  // [n_calls][B]: how many of them each call gives each gait (0: its steps have run out)
  std::vector<int> len_after;            // [n_calls + 1][B]: the gait's samples once call c has run
  std::vector<int> len_ended;            // [B]: ... and once wg_zmpdisc_end_dev has
  std::vector<int> sel;                  // [n_calls + 1][B]: 1 where the gait's steps run out with call c, to be ended behind it
};

// steps [B][S], n_steps [B].  Returns -1, or the first gait with fewer than the two steps the begin call needs.
// `first`: [B] or null -- the steps the begin call takes of each gait where that is not two of every one (--plan: the support
// foot and the arc); only the times of `steps` are read then.  `models`: [B] or null -- a model per gait in place of zm.
inline int online_plan(const wg_zmpdisc_model_t &zm, const std::vector<wg_rel_step_t> &steps, const std::vector<int> &n_steps, int B,
                       int S, int K, OnlinePlan *plan, const std::vector<int> *first = nullptr,
                       const wg_zmpdisc_model_t *models = nullptr) {
  OnlinePlan &p = *plan;
  auto model = [&](int g) { return models ? &models[g] : &zm; };
  if (first) {
    int n_calls = 0;
    for (int g = 0; g < B; ++g) {
      const int f = (*first)[g], c = (n_steps[g] - f + K - 1) / K;
      if (f < 2 || f > n_steps[g]) return g;
      n_calls = c > n_calls ? c : n_calls;
    }
    p.n_calls = n_calls;
    p.chunks.clear();                                      // the steps are planned on the device: none to regroup
    p.cns.assign((size_t)n_calls * B, 0);
    p.len_after.assign((size_t)(n_calls + 1) * B, 0);
    p.len_ended.assign(B, 0);
    p.sel.assign((size_t)(n_calls + 1) * B, 0);
    for (int g = 0; g < B; ++g) {
      const wg_rel_step_t *sg = &steps[(size_t)g * S];
      const int f = (*first)[g];
      p.len_ended[g] = wg_zmpdisc_length_after(model(g), sg, n_steps[g], 1);
      for (int c = 0; c <= n_calls; ++c) {
        const int given = f + c * K < n_steps[g] ? f + c * K : n_steps[g];
        p.len_after[(size_t)c * B + g] = wg_zmpdisc_length_after(model(g), sg, given, 0);
        p.sel[(size_t)c * B + g] = given == n_steps[g] && (c == 0 || f + (c - 1) * K < n_steps[g]);
        if (c < n_calls) p.cns[(size_t)c * B + g] = (f + (c + 1) * K < n_steps[g] ? f + (c + 1) * K : n_steps[g]) - given;
      }
    }
    return -1;
  }
  int S_max = 0;
  for (int g = 0; g < B; ++g) S_max = n_steps[g] > S_max ? n_steps[g] : S_max;
  const int n_calls = p.n_calls = S_max > 2 ? (S_max - 2 + K - 1) / K : 0;
  p.chunks.resize((size_t)n_calls * B * K);
  memset(p.chunks.data(), 0, sizeof(wg_rel_step_t) * p.chunks.size());
  p.cns.assign((size_t)n_calls * B, 0);
  p.len_after.assign((size_t)(n_calls + 1) * B, 0);
  p.len_ended.assign(B, 0);
  p.sel.assign((size_t)(n_calls + 1) * B, 0);
  for (int g = 0; g < B; ++g) {
    if (n_steps[g] < 2) return g;
    const wg_rel_step_t *sg = &steps[(size_t)g * S];
    p.len_ended[g] = wg_zmpdisc_length_after(model(g), sg, n_steps[g], 1);
    for (int c = 0; c <= n_calls; ++c) {
      const int given = 2 + c * K < n_steps[g] ? 2 + c * K : n_steps[g];
      p.len_after[(size_t)c * B + g] = wg_zmpdisc_length_after(model(g), sg, given, 0);
      p.sel[(size_t)c * B + g] = given == n_steps[g] && (c == 0 || 2 + (c - 1) * K < n_steps[g]);
    }
    for (int c = 0; c < n_calls; ++c) {
      const int first = 2 + c * K, left = n_steps[g] - first, n = left < 0 ? 0 : (left < K ? left : K);
      p.cns[(size_t)c * B + g] = n;
      for (int i = 0; i < n; ++i) p.chunks[((size_t)c * B + g) * K + i] = sg[first + i];
    }
  }
  return -1;
}

// The command lists of the --plan modes: what a fleet that decides its steps while it walks would hold in device memory.  Gait g
// starts on the foot of its parity, turns on an arc whose radius and angle are its own (1 .. 5 steps), walks on with on-line steps
// and finishes on the last correct support foot: S steps for every gait, from S + 1 - (arc steps) commands.  Whole-sequence mode
// gives the whole list in one call; on line the first two commands go in front of wg_zmpdisc_begin_dev and the rest, one step
// each, K per append.
struct CommandPlan {
  int ccap = 0, n_calls = 0;
  std::vector<wg_step_cmd_t> whole;      // [B][ccap]
  std::vector<int> n_whole;              // [B]
  std::vector<int> first_steps;          // [B]: steps the support foot and the arc give
  std::vector<wg_step_cmd_t> later;      // [n_calls][B][K]: the commands behind those two, regrouped call by call
  std::vector<int> n_later;              // [n_calls][B]
};

// Returns -1, or the first gait whose list does not give S steps (cannot be for 4 <= S <= WG_ZMPDISC_MAX_STEPS).  K == 0: no cuts.
// `scale`: [B] or null -- the size of gait g's robot: its arc's radius and the lengths of its on-line steps grow with it.
inline int command_plan(int B, int S, int K, CommandPlan *plan, const double *scale = nullptr) {
  CommandPlan &p = *plan;
  p.ccap = S;
  p.whole.assign((size_t)B * S, wg_step_cmd_t{WG_STEP_NONE, 0, {0.0, 0.0, 0.0}});
  p.n_whole.assign(B, 0);
  p.first_steps.assign(B, 0);
  int most = 0;
  for (int g = 0; g < B; ++g) {
    wg_step_cmd_t *c = &p.whole[(size_t)g * S];
    const int foot = (g & 1) ? 1 : -1, most_arc = S - 3 < 5 ? S - 3 : 5, n_arc = 1 + g % most_arc;
    const double sc = scale ? scale[g] : 1.0;
    const double R = (0.4 + 0.05 * (g % 17)) * sc, deg = (n_arc - 0.5) * 0.15 / R * 180.0 / 3.14159265358979323846;
    int n = 0;
    c[n++] = wg_step_cmd_t{WG_STEP_SUPPORT_FOOT, foot, {0.0, 0.0, 0.0}};
    c[n++] = wg_step_cmd_t{WG_STEP_ARC, -foot, {0.0, (g & 2) ? -R : R, deg}};   // n_arc - 1 whole steps and the shorter last one
    p.first_steps[g] = wg_steps_count(c, 2);
    if (p.first_steps[g] != 1 + n_arc) return g;
    for (int i = 0; i < S - 2 - n_arc; ++i) c[n++] = wg_step_cmd_t{WG_STEP_ONLINE, 0, {(0.1 + 0.01 * (g % 10)) * sc, 0.0, (g % 7) - 3.0}};
    c[n++] = wg_step_cmd_t{WG_STEP_LAST_SUPPORT, 0, {0.0, 0.0, 0.0}};
    p.n_whole[g] = n;
    if (wg_steps_count(c, n) != S) return g;
    most = n - 2 > most ? n - 2 : most;
  }
  p.n_calls = K ? (most + K - 1) / K : 0;
  p.later.assign((size_t)p.n_calls * B * (K ? K : 1), wg_step_cmd_t{WG_STEP_NONE, 0, {0.0, 0.0, 0.0}});
  p.n_later.assign((size_t)p.n_calls * B, 0);
  for (int g = 0; K && g < B; ++g)
    for (int i = 2; i < p.n_whole[g]; ++i) {
      const int call = (i - 2) / K;
      p.later[((size_t)call * B + g) * K + p.n_later[(size_t)call * B + g]++] = p.whole[(size_t)g * S + i];
    }
  return -1;
}

// Such a fleet seen from the host.  --plan-host feeds these steps through the upload path: every byte wg_steps_plan_dev would
// write.  --plan (times_only) uploads none of them and only sizes its buffers: wg_steps_count steps per gait that carry the
// call's times and nothing else -- a walk's length depends only on the count and the times (wg_zmpdisc_length_after) -- but for
// gait 0, whose steps the programs check their device chain against.  Returns -1, or the first gait that does not give S steps.
// `models`: [B] or null -- gait g's steps carry its own model's support times in place of ss, ds.
inline int command_steps(const CommandPlan &p, int B, int S, double ss, double ds, bool times_only, std::vector<wg_rel_step_t> *steps,
                         std::vector<int> *n_steps, const wg_zmpdisc_model_t *models = nullptr) {
  for (int g = 0; g < B; ++g) {
    wg_rel_step_t *sg = &(*steps)[(size_t)g * S];
    if (models) { ss = models[g].t_single; ds = models[g].t_double; }
    if (times_only && g > 0) {
      const int n = (*n_steps)[g] = wg_steps_count(&p.whole[(size_t)g * S], p.n_whole[g]);
      if (n != S) return g;
      for (int i = 0; i < n; ++i) sg[i] = wg_rel_step_t{0.0, 0.0, 0.0, ss, ds, 0, 0};
      continue;
    }
    wg_step_stack_t stack = {1, 0, 0, 0};
    if (wg_steps_plan(&p.whole[(size_t)g * S], p.n_whole[g], ss, ds, &stack, S, sg, &(*n_steps)[g]) != WG_OK || stack.error ||
        (*n_steps)[g] != S)
      return g;
  }
  return -1;
}

}  // namespace wg_fleet
