// wg_fleet.hpp -- what the fleet programs (kajita_fleet, dimitrov_fleet, fleet_bench, latency_b1) share: the error-exit macros,
// checked device allocations, the checksum, and the feeding plan of the --online modes.  Header-only host code: no kernels, and
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
inline int online_plan(const wg_zmpdisc_model_t &zm, const std::vector<wg_rel_step_t> &steps, const std::vector<int> &n_steps, int B,
                       int S, int K, OnlinePlan *plan) {
  OnlinePlan &p = *plan;
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
    p.len_ended[g] = wg_zmpdisc_length_after(&zm, sg, n_steps[g], 1);
    for (int c = 0; c <= n_calls; ++c) {
      const int given = 2 + c * K < n_steps[g] ? 2 + c * K : n_steps[g];
      p.len_after[(size_t)c * B + g] = wg_zmpdisc_length_after(&zm, sg, given, 0);
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

}  // namespace wg_fleet
