// dimitrov_fleet.cpp -- the Dimitrov-2008 fleet path from plain C++ through the C ABI (no Python, no PyTorch): B step sequences
// in device memory -> wg_zmpdisc_full_batch_dev (feet trajectories, time-major) -> wg_foot_constraints_batch_dev (polytope
// queues) -> wg_dimitrov_walk_dev (n ticks: queue walk + fused tick), nothing leaves the device in between.  The Dimitrov twin of
// kajita_fleet.cpp.  Prints one line with walks/s, ticks/s and a checksum (FNV-1a, 64 bit) of the final states.
//
//   dimitrov_fleet [--batch B] [--steps S] [--ticks K] [--solver 0|1|2] [--fleet FILE]
//
// --fleet FILE runs a fleet somebody else drew instead of the built-in one (tests/test_dimitrov_walk_gpu.py compares the
// checksum with its own run of the same fleet): int32 B, int32 smax, wg_zmpdisc_model_t, B x smax wg_rel_step_t, B int32
// n_steps, B x 6 doubles init_feet, in the machine's byte order.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/wg_mpc.h"

#define CHECK_HIP(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { fprintf(stderr, "FAILED: %s: %s\n", #e, hipGetErrorString(r_)); return 1; } } while (0)
#define CHECK_WG(e) do { int r_ = (e); if (r_ != WG_OK) { fprintf(stderr, "FAILED: %s: %s\n", #e, wg_last_error()); return 1; } } while (0)

int main(int argc, char **argv) {
  int B = 4096, S = 8, K = 40, solver = WG_DIMITROV_PLDP;
  const char *fleet = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--batch") && i + 1 < argc) B = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--steps") && i + 1 < argc) S = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--ticks") && i + 1 < argc) K = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--solver") && i + 1 < argc) solver = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--fleet") && i + 1 < argc) fleet = argv[++i];
  }
  wg_zmpdisc_model_t zm;
  wg_zmpdisc_defaults(&zm);
  zm.t_single = 0.7; zm.t_double = 0.13;                       // phase boundaries off the 0.1 s grid of the previewed instants
  std::vector<wg_rel_step_t> steps;
  std::vector<int> n_steps;
  std::vector<double> feet;
  if (fleet) {
    FILE *f = fopen(fleet, "rb");
    int32_t hdr[2];
    if (!f || fread(hdr, sizeof hdr, 1, f) != 1 || hdr[0] < 1 || hdr[1] < 2 || hdr[1] > WG_ZMPDISC_MAX_STEPS) { fprintf(stderr, "FAILED: cannot read %s\n", fleet); return 1; }
    B = hdr[0]; S = hdr[1];
    steps.resize((size_t)B * S); n_steps.resize(B); feet.resize((size_t)B * 6);
    if (fread(&zm, sizeof zm, 1, f) != 1 || fread(steps.data(), sizeof(wg_rel_step_t), steps.size(), f) != steps.size() ||
        fread(n_steps.data(), sizeof(int), B, f) != (size_t)B || fread(feet.data(), sizeof(double), feet.size(), f) != feet.size()) {
      fprintf(stderr, "FAILED: %s is short\n", fleet);
      return 1;
    }
    fclose(f);
  } else {
    if (B < 1 || S < 2 || S > WG_ZMPDISC_MAX_STEPS) { fprintf(stderr, "FAILED: need B >= 1, 2 <= steps <= %d\n", WG_ZMPDISC_MAX_STEPS); return 1; }
    steps.resize((size_t)B * S); n_steps.assign(B, S); feet.resize((size_t)B * 6);
    for (int g = 0; g < B; ++g) {                               // straight walks of varying step length: axis-aligned soles
      std::mt19937_64 rng(20080 + g);
      std::uniform_real_distribution<double> len(0.1, 0.25);
      double side = (g & 1) ? 1.0 : -1.0;
      for (int i = 0; i < S; ++i) {
        wg_rel_step_t &s = steps[(size_t)g * S + i];
        memset(&s, 0, sizeof s);
        const bool ends = i == 0 || i == S - 1;
        s.sx = ends ? 0.0 : len(rng);
        s.sy = side * (i == 0 ? 0.105 : 0.21);
        s.ss_time = zm.t_single; s.ds_time = 0.0; s.step_type = 1;
        side = -side;
      }
      const double f[6] = {0.0, 0.095, 0.0, 0.0, -0.095, 0.0};
      memcpy(&feet[(size_t)g * 6], f, sizeof f);
    }
  }
  if (K < 1) { fprintf(stderr, "FAILED: need ticks >= 1\n"); return 1; }
  CHECK_WG(wg_init(0));
  wg_dimitrov_model_t dm;
  wg_dimitrov_defaults(&dm);
  dm.solver = solver;
  CHECK_WG(wg_dimitrov_configure(&dm));

  int lcap = 0;
  for (int g = 0; g < B; ++g) {
    const int L = wg_zmpdisc_length(&zm, &steps[(size_t)g * S], n_steps[g]);
    if (L < 1) { fprintf(stderr, "FAILED: gait %d: sequence refused (%d)\n", g, L); return 1; }
    lcap = L > lcap ? L : lcap;
  }
  std::vector<double> time(lcap);
  { double t = 0.0; for (int l = 0; l < lcap; ++l) { t += zm.T; time[l] = t - zm.T; } }       // the running sum of the periods, from 0
  const int qcap = 2 * S + 8 > 64 ? 2 * S + 8 : 64;             // two polytopes per step, the rest phases either side

  wg_rel_step_t *d_steps; int *d_ns, *d_len, *d_lty, *d_count, *d_ran; double *d_feet, *d_time, *d_left, *d_right, *d_ts, *d_te;
  wg_zmp_polytope_t *d_queues; wg_dimitrov_state_t *d_states;
  const size_t row = (size_t)lcap * B, nq = (size_t)B * qcap;
  CHECK_HIP(hipMalloc((void **)&d_steps, sizeof(wg_rel_step_t) * steps.size()));
  CHECK_HIP(hipMalloc((void **)&d_ns, sizeof(int) * B));
  CHECK_HIP(hipMalloc((void **)&d_len, sizeof(int) * B));
  CHECK_HIP(hipMalloc((void **)&d_count, sizeof(int) * B));
  CHECK_HIP(hipMalloc((void **)&d_ran, sizeof(int) * B));
  CHECK_HIP(hipMalloc((void **)&d_lty, sizeof(int) * row));
  CHECK_HIP(hipMalloc((void **)&d_feet, sizeof(double) * feet.size()));
  CHECK_HIP(hipMalloc((void **)&d_time, sizeof(double) * lcap));
  CHECK_HIP(hipMalloc((void **)&d_left, sizeof(double) * 6 * row));
  CHECK_HIP(hipMalloc((void **)&d_right, sizeof(double) * 6 * row));
  CHECK_HIP(hipMalloc((void **)&d_ts, sizeof(double) * nq));
  CHECK_HIP(hipMalloc((void **)&d_te, sizeof(double) * nq));
  CHECK_HIP(hipMalloc((void **)&d_queues, sizeof(wg_zmp_polytope_t) * nq));
  CHECK_HIP(hipMalloc((void **)&d_states, sizeof(wg_dimitrov_state_t) * B));
  CHECK_HIP(hipMemcpy(d_steps, steps.data(), sizeof(wg_rel_step_t) * steps.size(), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(d_ns, n_steps.data(), sizeof(int) * B, hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(d_feet, feet.data(), sizeof(double) * feet.size(), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(d_time, time.data(), sizeof(double) * lcap, hipMemcpyHostToDevice));
  std::vector<wg_dimitrov_state_t> states(B);
  memset(states.data(), 0, sizeof(wg_dimitrov_state_t) * B);
  for (int g = 0; g < B; ++g) states[g].starting = 1;
  hipStream_t st;
  CHECK_HIP(hipStreamCreate(&st));
  double sec = 0.0, sec_walk = 0.0;
  for (int rep = 0; rep < 2; ++rep) {                          // the second pass is the timed one
    CHECK_HIP(hipMemcpyAsync(d_states, states.data(), sizeof(wg_dimitrov_state_t) * B, hipMemcpyHostToDevice, st));
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    CHECK_WG(wg_zmpdisc_full_batch_dev(&zm, B, S, d_steps, d_ns, d_feet, lcap, nullptr, nullptr, nullptr, nullptr, d_left, d_lty, d_right,
                                       nullptr, d_len, st));
    CHECK_WG(wg_foot_constraints_batch_dev(B, lcap, d_len, d_time, d_left, d_lty, d_right, 0.24, 0.138, 0.02, 0.02, qcap, d_queues, d_ts,
                                           d_te, d_count, st));
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    CHECK_WG(wg_dimitrov_walk_dev(B, qcap, d_queues, d_ts, d_te, d_count, 0.0, K, d_states, nullptr, d_ran, 0, st));
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();
    sec = std::chrono::duration<double>(t2 - t0).count();
    sec_walk = std::chrono::duration<double>(t2 - t1).count();
  }
  std::vector<int> count(B), ran(B);
  CHECK_HIP(hipMemcpy(states.data(), d_states, sizeof(wg_dimitrov_state_t) * B, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(count.data(), d_count, sizeof(int) * B, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(ran.data(), d_ran, sizeof(int) * B, hipMemcpyDeviceToHost));
  int n_ran = 0, max_count = 0;
  for (int g = 0; g < B; ++g) {
    if (count[g] < 1 || count[g] > qcap) { fprintf(stderr, "FAILED: gait %d: %d polytopes (capacity %d)\n", g, count[g], qcap); return 1; }
    n_ran += ran[g];
    max_count = count[g] > max_count ? count[g] : max_count;
  }
  uint64_t h = 1469598103934665603ull;
  const unsigned char *p = reinterpret_cast<const unsigned char *>(states.data());
  for (size_t i = 0; i < sizeof(wg_dimitrov_state_t) * B; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  double far = 0.0;
  for (int g = 0; g < B; ++g) far = states[g].xk[0] > far ? states[g].xk[0] : far;
  printf("dimitrov_fleet: %d walks (<= %d steps, <= %d samples, <= %d polytopes) x %d ticks in %.2f ms = %.0f walks/s; the walk alone "
         "%.2f ms = %.0f ticks/s; %d gaits ran out of their queue; farthest CoM %.3f m; checksum %016llx\n", B, S, lcap, max_count, K,
         sec * 1e3, B / sec, sec_walk * 1e3, (double)B * K / sec_walk, n_ran, far, (unsigned long long)h);
  wg_shutdown();
  return 0;
}
