// morisawa_fleet.cpp -- Morisawa-2007 analytic walks for a fleet from plain C++ through the C ABI (no Python, no PyTorch): B step
// sequences in device memory -> wg_morisawa_walk_dev (one linear system per gait solved in a wavefront, then CoM, ZMP and both
// feet sampled on the control loop's clock), nothing leaves the device in between.  Gait 0 walks TestMorisawa2007's short
// straight walk where --steps allows it; gait 0 and gait B - 1 are checked against the host twins (wg_morisawa_solve +
// wg_morisawa_sample on the same input, bit for bit); the others vary step length, heading and first foot.
//
// With --heights LO:HI gait b walks at its own CoM height, LO + (HI - LO) b / (B - 1), and with its own support times (a table of
// multiples of T): a model per gait through wg_morisawa_walk_fleet_dev.
//
// With --long the walk goes through the long family (wg_morisawa_long_*: Z eliminated as a band) and --steps may be up to 64.
//
// With --replan K one gait is solved (wg_morisawa[_long]_solve_dev, B = 1) and K candidate plans -- other steps, the same times and
// height -- are re-planned from its block's kept factor on the same stream (wg_morisawa[_long]_resolve_dev: no Z, no elimination);
// the first and the last candidate's blocks are checked against the host's full solves of those plans, byte for byte.
//
// With --audit the walks are judged where they lie: on the same stream, with no synchronisation in between, the sampler's feet and
// natures go through wg_foot_constraints_batch_dev and its ZMP through wg_zmp_audit_dev against those queues; only the verdicts
// come back (32 bytes per gait).  Gaits 0 and B - 1 are held to the host twin wg_zmp_audit.  With --replan K every candidate is
// sampled and audited behind the re-plan, and the candidate whose ZMP keeps the largest margin is named.
//
// Prints a checksum (FNV-1a, 64 bit, over the gaits' checksums of their own rows of CoM, ZMP and feet) and the milliseconds per fleet.
//
//   morisawa_fleet [--batch B] [--steps S] [--heights LO:HI] [--long] [--replan K] [--audit]
#include <chrono>
#include <cstdlib>
#include <random>

#include "wg_fleet.hpp"

using wg_fleet::dev_alloc;
using wg_fleet::dev_upload;

int main(int argc, char **argv) {
  int B = 4096, S = 7, replan = 0;
  bool heights = false, lng = false, audit = false;
  double h_lo = 0.7116911, h_hi = 0.7116911;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--batch") && i + 1 < argc) B = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--steps") && i + 1 < argc) S = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--long")) lng = true;
    else if (!strcmp(argv[i], "--audit")) audit = true;
    else if (!strcmp(argv[i], "--replan") && i + 1 < argc) {
      replan = atoi(argv[++i]);
      if (replan < 1) { fprintf(stderr, "FAILED: need --replan K with K >= 1\n"); return 1; }
      B = replan;
    }
    else if (!strcmp(argv[i], "--heights") && i + 1 < argc) {
      heights = sscanf(argv[++i], "%lf:%lf", &h_lo, &h_hi) == 2;
      if (!heights || !(h_lo > 0.0) || !(h_hi >= h_lo) || !(h_hi < 1e3)) { fprintf(stderr, "FAILED: need --heights LO:HI with 0 < LO <= HI\n"); return 1; }
    }
  }
  const int cap = lng ? WG_MORISAWA_LONG_MAX_STEPS : WG_MORISAWA_MAX_STEPS;
  if (replan && heights) { fprintf(stderr, "FAILED: --replan shares one factor: the candidates have one height and one model\n"); return 1; }
  if (replan) B = replan;
  if (B < 1 || S < 2 || S > cap) { fprintf(stderr, "FAILED: need B >= 1, 2 <= steps <= %d%s\n", cap, lng ? "" : " (--long: 64)"); return 1; }
  // the two families have one argument list per call: --long chooses the set
  const auto length_fn = lng ? wg_morisawa_long_length : wg_morisawa_length;
  const auto block_bytes_fn = lng ? wg_morisawa_long_block_bytes : wg_morisawa_block_bytes;
  const auto walk_fn = lng ? wg_morisawa_long_walk_dev : wg_morisawa_walk_dev;
  const auto walk_fleet_fn = lng ? wg_morisawa_long_walk_fleet_dev : wg_morisawa_walk_fleet_dev;
  const auto solve_fn = lng ? wg_morisawa_long_solve : wg_morisawa_solve;
  const auto sample_fn = lng ? wg_morisawa_long_sample : wg_morisawa_sample;
  CHECK_WG(wg_init(0));
  wg_morisawa_model_t base;
  wg_morisawa_defaults(&base);                                // 5 ms, 0.78 / 0.02 s supports, 0.07 m step height
  std::vector<wg_morisawa_model_t> models(B, base);
  std::vector<wg_rel_step_t> steps((size_t)B * S);
  std::vector<int> n_steps(B, S);
  std::vector<double> feet((size_t)B * 6), com0((size_t)B * 3);
  static const int single_ticks[] = {140, 156, 160, 120}, double_ticks[] = {4, 8, 12, 20};
  for (int g = 0; g < B; ++g) {
    std::mt19937_64 rng(20070 + g);
    std::uniform_real_distribution<double> len(0.1, 0.25), turn(-5.0, 5.0);
    double side = (g & 1) ? 1.0 : -1.0;
    for (int i = 0; i < S; ++i) {
      wg_rel_step_t &s = steps[(size_t)g * S + i];
      memset(&s, 0, sizeof s);
      const bool ends = i == 0 || i == S - 1;
      s.sx = ends ? 0.0 : (g == 0 ? 0.2 : len(rng));
      s.sy = side * (i == 0 ? 0.105 : 0.19);
      s.theta = (ends || g == 0) ? 0.0 : turn(rng);
      s.step_type = 1;
      side = -side;
    }
    const double f[6] = {0.0, 0.09, 0.0, 0.0, -0.09, 0.0};
    memcpy(&feet[(size_t)g * 6], f, sizeof f);
    com0[(size_t)g * 3 + 0] = 0.0316054587;
    com0[(size_t)g * 3 + 1] = 0.0;
    com0[(size_t)g * 3 + 2] = heights && B > 1 ? h_lo + (h_hi - h_lo) * g / (B - 1) : h_lo;
    if (heights) {
      models[g].t_single = single_ticks[g % 4] * base.T;
      models[g].t_double = double_ticks[(g / 4) % 4] * base.T;
    }
  }
  const double t_start = 2.0 * base.t_single;                 // the reference's queue starts there
  std::vector<int> len_g(B);
  int L = 0;
  for (int g = 0; g < B; ++g) {
    len_g[g] = length_fn(&models[g], S, t_start);
    if (len_g[g] < 1) { fprintf(stderr, "FAILED: gait %d has %d samples\n", g, len_g[g]); return 1; }
    L = len_g[g] > L ? len_g[g] : L;
  }
  const size_t bb = block_bytes_fn(S);

  wg_rel_step_t *d_steps; int *d_ns, *d_status, *d_len, *d_lt, *d_rt; double *d_feet, *d_com0, *d_zx, *d_zy, *d_com, *d_left, *d_right;
  wg_morisawa_model_t *d_models; void *d_blocks;
  CHECK_HIP(dev_upload(&d_steps, steps));
  CHECK_HIP(dev_upload(&d_ns, n_steps));
  CHECK_HIP(dev_upload(&d_feet, feet));
  CHECK_HIP(dev_upload(&d_com0, com0));
  CHECK_HIP(dev_upload(&d_models, models));
  CHECK_HIP(hipMalloc(&d_blocks, bb * B));
  CHECK_HIP(dev_alloc(&d_status, B));
  CHECK_HIP(dev_alloc(&d_len, B));
  CHECK_HIP(dev_alloc(&d_zx, (size_t)L * B));
  CHECK_HIP(dev_alloc(&d_zy, (size_t)L * B));
  CHECK_HIP(dev_alloc(&d_com, (size_t)L * 4 * B));
  CHECK_HIP(dev_alloc(&d_left, (size_t)L * 6 * B));
  CHECK_HIP(dev_alloc(&d_right, (size_t)L * 6 * B));
  CHECK_HIP(dev_alloc(&d_lt, (size_t)L * B));
  CHECK_HIP(dev_alloc(&d_rt, (size_t)L * B));
  hipStream_t st;
  CHECK_HIP(hipStreamCreate(&st));
  double sec = 0.0;
  // --audit: the shared time array, the queues and the verdicts; the three launches behind whatever made the samples
  const int qcap = 2 * S + 4;                                 // a polytope per support phase: two per step and the ends
  const wg_sole_t sole{0.24, 0.138, 0.02, 0.02};
  std::vector<double> time_h(L);
  double *d_time = nullptr, *d_ts = nullptr, *d_te = nullptr;
  wg_zmp_polytope_t *d_queues = nullptr;
  int *d_count = nullptr;
  wg_fleet::FleetAudit fa;
  if (audit) {
    double t = 0.0;
    for (int l = 0; l < L; ++l) { time_h[l] = t; t += base.T; }
    CHECK_HIP(dev_upload(&d_time, time_h));
    CHECK_HIP(dev_alloc(&d_queues, (size_t)B * qcap));
    CHECK_HIP(dev_alloc(&d_ts, (size_t)B * qcap));
    CHECK_HIP(dev_alloc(&d_te, (size_t)B * qcap));
    CHECK_HIP(dev_alloc(&d_count, B));
    CHECK_HIP(dev_alloc(&fa.d_audit, B));
  }
  auto audit_launch = [&]() -> int {
    if (int rc = wg_foot_constraints_batch_dev(B, L, d_len, d_time, d_left, d_lt, d_right, sole.sole_w, sole.sole_h, sole.constraint_x,
                                               sole.constraint_y, qcap, d_queues, d_ts, d_te, d_count, st)) return rc;
    return wg_zmp_audit_dev(B, L, d_len, d_time, d_zx, d_zy, B, qcap, d_queues, d_ts, d_te, d_count, fa.d_audit, nullptr, st);
  };
  if (replan) {
    const auto solve_dev_fn = lng ? wg_morisawa_long_solve_dev : wg_morisawa_solve_dev;
    const auto resolve_dev_fn = lng ? wg_morisawa_long_resolve_dev : wg_morisawa_resolve_dev;
    void *d_fac;
    int *d_fst;
    CHECK_HIP(hipMalloc(&d_fac, bb));
    CHECK_HIP(dev_alloc(&d_fst, 1));
    for (int rep = 0; rep < 2; ++rep) {                        // the second pass is the timed one: factor once, K plans from it
      CHECK_HIP(hipStreamSynchronize(st));
      const auto t0 = std::chrono::steady_clock::now();
      CHECK_WG(solve_dev_fn(&base, 1, S, d_steps, d_ns, d_feet, d_com0, d_fac, d_fst, st));
      CHECK_WG(resolve_dev_fn(&base, B, S, d_fac, 1, nullptr, d_steps, d_feet, d_com0, d_blocks, d_status, st));
      if (audit) {
        const auto sample_dev_fn = lng ? wg_morisawa_long_sample_dev : wg_morisawa_sample_dev;
        CHECK_WG(sample_dev_fn(B, S, d_blocks, d_status, t_start, base.T, L, d_zx, d_zy, nullptr, d_left, d_lt, d_right, nullptr, d_len, st));
        CHECK_WG(audit_launch());
      }
      CHECK_HIP(hipStreamSynchronize(st));
      sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    std::vector<int> status(B);
    std::vector<double> blocks(bb / sizeof(double) * B), blk(bb / sizeof(double));
    CHECK_HIP(hipMemcpy(status.data(), d_status, sizeof(int) * B, hipMemcpyDeviceToHost));
    CHECK_HIP(hipMemcpy(blocks.data(), d_blocks, bb * B, hipMemcpyDeviceToHost));
    for (int g = 0; g < B; ++g)
      if (status[g] != WG_OK) { fprintf(stderr, "FAILED: candidate %d: status %d\n", g, status[g]); return 1; }
    for (int g : {0, B - 1}) {                                 // the full solve of the candidate's plan on the host: the same bytes
      int hs = 0;
      CHECK_WG(solve_fn(&base, 1, S, &steps[(size_t)g * S], &n_steps[g], &feet[(size_t)g * 6], &com0[(size_t)g * 3], blk.data(), &hs));
      if (hs != WG_OK || memcmp(blk.data(), &blocks[bb / sizeof(double) * g], bb)) {
        fprintf(stderr, "FAILED: the re-planned block of candidate %d differs from the full solve's\n", g);
        return 1;
      }
    }
    printf("morisawa_fleet: %d candidate plans%s of %d steps re-planned from one kept factor in %.2f ms = %.0f plans/s (one solve "
           "included); candidates 0 and %d == full solves by bytes; checksum %016llx\n", B, lng ? " (long family)" : "", S, sec * 1e3, B / sec,
           B - 1, (unsigned long long)wg_fleet::fnv1a64(blocks.data(), bb * B));
    if (audit) {
      if (wg_fleet::audit_report("morisawa_fleet", "the candidates' ZMP (sampled, queued and audited behind the re-plan, in the time above)", &fa, B,
                                 L, len_g.data(), time_h.data(), d_zx, d_zy, B, qcap, d_queues, d_ts, d_te, d_count)) return 1;
      printf("morisawa_fleet: best candidate %d (least margin %.6f m)\n", fa.best_gait, fa.audit[fa.best_gait].margin);
    }
    wg_shutdown();
    return 0;
  }
  for (int rep = 0; rep < 2; ++rep) {                          // the second pass is the timed one
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    if (heights)
      CHECK_WG(walk_fleet_fn(d_models, base.T, B, S, d_steps, d_ns, d_feet, d_com0, d_blocks, d_status, t_start, L, d_zx, d_zy,
                             d_com, d_left, d_lt, d_right, d_rt, d_len, st));
    else
      CHECK_WG(walk_fn(&base, B, S, d_steps, d_ns, d_feet, d_com0, d_blocks, d_status, t_start, L, d_zx, d_zy, d_com, d_left,
                       d_lt, d_right, d_rt, d_len, st));
    if (audit) CHECK_WG(audit_launch());
    CHECK_HIP(hipStreamSynchronize(st));
    sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  std::vector<int> status(B), len_h(B);
  CHECK_HIP(hipMemcpy(status.data(), d_status, sizeof(int) * B, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(len_h.data(), d_len, sizeof(int) * B, hipMemcpyDeviceToHost));
  for (int g = 0; g < B; ++g) {
    if (status[g] != WG_OK) { fprintf(stderr, "FAILED: gait %d: status %d\n", g, status[g]); return 1; }
    if (len_h[g] != len_g[g]) { fprintf(stderr, "FAILED: gait %d has %d samples, not %d\n", g, len_h[g], len_g[g]); return 1; }
  }
  std::vector<double> zx((size_t)L * B), zy((size_t)L * B), com((size_t)L * 4 * B), left((size_t)L * 6 * B), right((size_t)L * 6 * B);
  CHECK_HIP(hipMemcpy(zx.data(), d_zx, sizeof(double) * zx.size(), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(zy.data(), d_zy, sizeof(double) * zy.size(), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(com.data(), d_com, sizeof(double) * com.size(), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(left.data(), d_left, sizeof(double) * left.size(), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(right.data(), d_right, sizeof(double) * right.size(), hipMemcpyDeviceToHost));
  // a gait against the host twins, one gait at a time
  auto check_gait = [&](int g) -> int {
    std::vector<double> blk(bb / sizeof(double)), hzx(L), hzy(L), hcom((size_t)L * 4), hl((size_t)L * 6), hr((size_t)L * 6);
    int hs = 0, hlen = 0;
    CHECK_WG(solve_fn(&models[g], 1, S, &steps[(size_t)g * S], &n_steps[g], &feet[(size_t)g * 6], &com0[(size_t)g * 3], blk.data(), &hs));
    CHECK_WG(sample_fn(1, S, blk.data(), &hs, t_start, base.T, L, hzx.data(), hzy.data(), hcom.data(), hl.data(), nullptr, hr.data(), nullptr,
                       &hlen));
    bool same = hs == WG_OK && hlen == len_g[g];
    for (int l = 0; same && l < L; ++l) {
      same = zx[(size_t)l * B + g] == hzx[l] && zy[(size_t)l * B + g] == hzy[l];
      for (int c = 0; c < 4; ++c) same = same && com[((size_t)l * 4 + c) * B + g] == hcom[(size_t)l * 4 + c];
      for (int c = 0; c < 6; ++c) same = same && left[((size_t)l * 6 + c) * B + g] == hl[(size_t)l * 6 + c] && right[((size_t)l * 6 + c) * B + g] == hr[(size_t)l * 6 + c];
    }
    if (!same) { fprintf(stderr, "FAILED: device walk of gait %d differs from the host twins\n", g); return 1; }
    return 0;
  };
  if (check_gait(0) || (B > 1 && check_gait(B - 1))) return 1;
  std::vector<double> own;                                    // a gait's own rows; the checksum is over the gaits' checksums, in order
  std::vector<unsigned long long> sums(B);
  double far = 0.0;
  for (int g = 0; g < B; ++g) {
    own.clear();
    for (int l = 0; l < len_g[g]; ++l) {
      own.push_back(zx[(size_t)l * B + g]);
      own.push_back(zy[(size_t)l * B + g]);
      for (int c = 0; c < 4; ++c) own.push_back(com[((size_t)l * 4 + c) * B + g]);
      for (int c = 0; c < 6; ++c) { own.push_back(left[((size_t)l * 6 + c) * B + g]); own.push_back(right[((size_t)l * 6 + c) * B + g]); }
    }
    sums[g] = wg_fleet::fnv1a64(own.data(), own.size() * sizeof(double));
    const double x = com[((size_t)(len_g[g] - 1) * 4) * B + g];
    far = x > far ? x : far;
  }
  const unsigned long long sum = wg_fleet::fnv1a64(sums.data(), sums.size() * sizeof(sums[0]));
  if (heights) printf("morisawa_fleet: CoM heights %.4f .. %.4f m and support times per gait (a model per gait)\n", h_lo, h_hi);
  printf("morisawa_fleet: %d analytic walks%s of %d steps (up to %d samples) in %.2f ms = %.0f walks/s; gait 0 ends at x = %.4f m (%d samples), "
         "farthest %.2f m; gaits 0 and %d == host twins; checksum %016llx\n", B, lng ? " (long family)" : "", S, L, sec * 1e3, B / sec,
         com[((size_t)(len_g[0] - 1) * 4) * B + 0], len_g[0], far, B - 1, sum);
  if (audit && wg_fleet::audit_report("morisawa_fleet", "the walks' ZMP (queues and audit behind the walk, in the time above)", &fa, B, L,
                                      len_g.data(), time_h.data(), d_zx, d_zy, B, qcap, d_queues, d_ts, d_te, d_count)) return 1;
  wg_shutdown();
  return 0;
}
