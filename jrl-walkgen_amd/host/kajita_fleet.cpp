// kajita_fleet.cpp -- the Kajita stage-1 fleet path from plain C++ through the C ABI (no Python, no PyTorch): B step sequences
// in device memory -> wg_zmpdisc_batch_dev (ZMP reference queues, time-major) -> wg_preview_run_batch_dev (cart-table CoM),
// nothing leaves the device in between.  Gait 0 walks TestKajita2003's StraightWalking sequence and is checked against
// the host-pointer entry points on the same input (bit for bit); the others vary step length and heading.
//
// With --online K the same walks are fed K steps per call instead: wg_zmpdisc_begin_dev on the first two steps, then
// { wg_zmpdisc_append_dev on the next K; wg_preview_run_batch_dev on the rows that became safe } until the steps run out,
// wg_zmpdisc_end_dev and the remaining rows.  Every step is walked once, and the CoM trajectories -- hence the checksum
// (FNV-1a, 64 bit, over all of them) that both modes print -- are those of the whole-sequence mode.
//
// With --ragged gait g walks its own number of steps, between S/2 and S.  Whole-sequence mode: wg_zmpdisc_batch_dev, then ONE
// wg_preview_run_batch_dev over the longest gait.  With --online K the feeding plan runs out early for some gaits: they are
// ended (wg_zmpdisc_end_dev with `select`) behind the call that gave them their last step while the others walk on, and the
// preview is wg_preview_follow_dev behind every zmpdisc call, fed by the `length` array those calls leave on the device -- the
// host does no arithmetic on sample counts and reads nothing back.  Both modes print one checksum over each gait's OWN rows
// [0, len_g - nl + 1) of the CoM trajectories (the rows past them exist only in the whole-sequence mode): the same one.
//
// With --plan the steps are decided on the device: the only step input uploaded is a command list per gait (support foot, an arc
// of the gait's own radius and angle, on-line steps, last support: wg_fleet::command_plan), and wg_steps_plan_dev writes the steps
// into the array wg_zmpdisc_* reads, on the same stream -- the whole list in front of wg_zmpdisc_batch_dev, or with --online K the
// first two commands in front of wg_zmpdisc_begin_dev and K in front of every wg_zmpdisc_append_dev, the preview following each
// gait's own queue as with --ragged (the arcs differ, so the gaits' sample counts do between the calls).  Buffers are sized with
// wg_steps_count and wg_zmpdisc_length_after.  --plan-host is its host-fed twin: the same lists through wg_steps_plan and the
// upload path above, with or without --online K.  Both print the same checksum.
//
// With --heights LO:HI gait b walks at its own CoM height, zc = LO + (HI - LO) b / (B - 1): its gains are made on the device
// (wg_riccati_gains_batch_dev, one lane per gait, on the same stream in front of the walk) and every preview call above is its
// fleet form (wg_preview_run_fleet_dev, wg_preview_follow_fleet_dev), which reads the gains per gait; the context's configured
// gains play no part.  Works with every mode above.  At the end every gait's status must be 0, and gait 0 AND gait B - 1 are
// checked against the one-gait host path configured with that gait's own wg_riccati_gains.
//
// With --audit (whole-sequence modes) the walks are judged where they lie, behind the chain above and on its stream:
// wg_zmpdisc_full_batch_dev gives the same sequences' feet, wg_foot_constraints_batch_dev their polytope queues, and
// wg_zmp_audit_dev audits the ZMP reference (pitch B) and the ZMP the preview realises, zmp2_tm [L][2][B], in place (pitch 2 B)
// against them.  Only the verdicts come back; the fleet's least margin, its gait and time, and the violated count are printed,
// gaits 0 and B - 1 are held to the host twin wg_zmp_audit.  The chain's own outputs and its checksum do not change.
//
//   kajita_fleet [--batch B] [--steps S] [--online K] [--ragged] [--plan | --plan-host] [--heights LO:HI] [--audit]
#include <chrono>
#include <cstdlib>
#include <random>

#include "wg_fleet.hpp"

using wg_fleet::dev_alloc;
using wg_fleet::dev_upload;

int main(int argc, char **argv) {
  int B = 4096, S = 16, K = 0;
  bool ragged = false, heights = false, audit = false;
  double zc_lo = 0.8078, zc_hi = 0.8078;
  int planned = 0;                                            // 1: --plan (steps planned on the device), 2: --plan-host
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--batch") && i + 1 < argc) B = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--steps") && i + 1 < argc) S = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--ragged")) ragged = true;
    else if (!strcmp(argv[i], "--audit")) audit = true;
    else if (!strcmp(argv[i], "--plan")) planned = 1;
    else if (!strcmp(argv[i], "--plan-host")) planned = 2;
    else if (!strcmp(argv[i], "--heights") && i + 1 < argc) {
      heights = sscanf(argv[++i], "%lf:%lf", &zc_lo, &zc_hi) == 2;
      if (!heights || !(zc_lo > 0.0) || !(zc_hi >= zc_lo) || !(zc_hi < 1e3)) { fprintf(stderr, "FAILED: need --heights LO:HI with 0 < LO <= HI\n"); return 1; }
    }
    else if (!strcmp(argv[i], "--online") && i + 1 < argc) { K = atoi(argv[++i]); if (K < 1 || K > WG_ZMPDISC_MAX_STEPS) { fprintf(stderr, "FAILED: need 1 <= --online K <= %d\n", WG_ZMPDISC_MAX_STEPS); return 1; } }
  }
  if (B < 1 || S < 2 || S > WG_ZMPDISC_MAX_STEPS) { fprintf(stderr, "FAILED: need B >= 1, 2 <= steps <= %d\n", WG_ZMPDISC_MAX_STEPS); return 1; }
  if (planned && (ragged || S < 4)) { fprintf(stderr, "FAILED: --plan needs steps >= 4 and no --ragged\n"); return 1; }
  if (audit && K) { fprintf(stderr, "FAILED: --audit goes with the whole-sequence modes (no --online)\n"); return 1; }
  const bool on_device = planned == 1;
  CHECK_WG(wg_init(0));
  wg_zmpdisc_model_t zm;
  wg_zmpdisc_defaults(&zm);                                   // 5 ms, 1.6 s preview, 0.78 / 0.02 s supports, 0.07 m step height
  // preview gains for the same sampling period / window (PreviewControl::ComputeOptimalWeights)
  const int nl = (int)(zm.preview_time / zm.T);
  double Kg[4];
  std::vector<double> F(nl);
  CHECK_WG(wg_riccati_gains(zm.T, 0.8078, 1.0, 1e-6, nl, WG_RICCATI_WITHOUT_INITIALPOS, Kg, F.data()));
  wg_preview_gains_t pg = {zm.T, 0.8078, Kg[0], {Kg[1], Kg[2], Kg[3]}, nl, 0};
  CHECK_WG(wg_preview_configure(&pg, F.data()));
  // --heights: a CoM height per gait; K_tm, F_tm and the status are written by the device in front of every walk
  std::vector<double> zc(B, 0.8078);
  if (heights)
    for (int g = 0; g < B; ++g) zc[g] = B > 1 ? zc_lo + (zc_hi - zc_lo) * g / (B - 1) : zc_lo;

  std::vector<wg_rel_step_t> steps((size_t)B * S);
  std::vector<int> n_steps(B, S);
  std::vector<double> feet((size_t)B * 6);
  for (int g = 0; g < B; ++g) {
    if (ragged) {                                              // S/2 .. S steps, at least the two the begin call takes
      const int lo = S / 2 > 2 ? S / 2 : 2;
      n_steps[g] = lo + (int)(std::mt19937_64(7700 + g)() % (unsigned)(S - lo + 1));
    }
    std::mt19937_64 rng(20100 + g);
    std::uniform_real_distribution<double> len(0.1, 0.25), turn(-5.0, 5.0);
    double side = (g & 1) ? 1.0 : -1.0;
    for (int i = 0; i < S; ++i) {
      wg_rel_step_t &s = steps[(size_t)g * S + i];
      memset(&s, 0, sizeof s);
      const bool ends = i == 0 || i == n_steps[g] - 1;
      s.sx = ends ? 0.0 : (g == 0 ? 0.2 : len(rng));
      s.sy = side * (i == 0 ? 0.105 : 0.21);
      s.theta = (ends || g == 0) ? 0.0 : turn(rng);
      s.ss_time = zm.t_single; s.ds_time = zm.t_double; s.step_type = 1;
      side = -side;
    }
    const double f[6] = {0.0094903, 0.095, 0.0, 0.0094903, -0.095, 0.0};
    memcpy(&feet[(size_t)g * 6], f, sizeof f);
  }
  // --plan, --plan-host: the steps come from command lists.  On the host they are the twin's input, and with --plan what the
  // buffers are sized by and gait 0 is checked against -- none of them is uploaded then
  wg_fleet::CommandPlan cp;
  if (planned) {
    if (wg_fleet::command_plan(B, S, K, &cp) >= 0 || wg_fleet::command_steps(cp, B, S, zm.t_single, zm.t_double, on_device, &steps, &n_steps) >= 0) {
      fprintf(stderr, "FAILED: the command lists do not give %d steps\n", S);
      return 1;
    }
    if (heights && on_device && B > 1) {                      // --heights checks gait B - 1 as well: its steps from the host twin, like gait 0's
      const size_t g = (size_t)B - 1;
      wg_step_stack_t stack = {1, 0, 0, 0};
      if (wg_steps_plan(&cp.whole[g * cp.ccap], cp.n_whole[g], zm.t_single, zm.t_double, &stack, S, &steps[g * S], &n_steps[g]) != WG_OK ||
          stack.error || n_steps[g] != S) {
        fprintf(stderr, "FAILED: the command list of gait %zu does not give %d steps\n", g, S);
        return 1;
      }
    }
  }
  // samples of every gait, L those of the longest (without --ragged: of all)
  std::vector<int> len_g(B);
  int L = 0, Lmin = 1 << 30;
  for (int g = 0; g < B; ++g) {
    len_g[g] = wg_zmpdisc_length(&zm, &steps[(size_t)g * S], n_steps[g]);
    if (len_g[g] < nl) { fprintf(stderr, "FAILED: sequence of %d samples\n", len_g[g]); return 1; }
    L = len_g[g] > L ? len_g[g] : L;
    Lmin = len_g[g] < Lmin ? len_g[g] : Lmin;
  }
  const int Lrun = L - nl + 1;

  wg_rel_step_t *d_steps; int *d_ns, *d_len, *d_done = nullptr, *d_sel = nullptr; double *d_feet, *d_zx, *d_zy, *d_state, *d_com;
  wg_step_cmd_t *d_cmds = nullptr, *d_later = nullptr; wg_step_stack_t *d_stack = nullptr; int *d_ncmds = nullptr, *d_nlater = nullptr;
  const std::vector<wg_step_stack_t> fresh(B, wg_step_stack_t{1, 0, 0, 0});
  if (on_device) {                                            // the steps' array is only written by the device
    CHECK_HIP(dev_alloc(&d_steps, steps.size()));
    CHECK_HIP(hipMemset(d_steps, 0, sizeof(wg_rel_step_t) * steps.size()));
    CHECK_HIP(dev_alloc(&d_ns, B));
    CHECK_HIP(dev_upload(&d_cmds, cp.whole));
    CHECK_HIP(dev_upload(&d_ncmds, K ? std::vector<int>(B, 2) : cp.n_whole));
    CHECK_HIP(dev_alloc(&d_stack, B));
  } else {
    CHECK_HIP(dev_upload(&d_steps, steps));
    CHECK_HIP(dev_upload(&d_ns, n_steps));
  }
  CHECK_HIP(dev_upload(&d_feet, feet));
  CHECK_HIP(dev_alloc(&d_len, B));
  CHECK_HIP(dev_alloc(&d_zx, (size_t)L * B));
  CHECK_HIP(dev_alloc(&d_zy, (size_t)L * B));
  CHECK_HIP(dev_alloc(&d_state, (size_t)8 * B));
  CHECK_HIP(dev_alloc(&d_com, (size_t)Lrun * 6 * B));
  double *d_zc = nullptr, *d_Ktm = nullptr, *d_Ftm = nullptr; int *d_status = nullptr;
  if (heights) {
    CHECK_HIP(dev_upload(&d_zc, zc));
    CHECK_HIP(dev_alloc(&d_Ktm, (size_t)4 * B));
    CHECK_HIP(dev_alloc(&d_Ftm, (size_t)nl * B));
    CHECK_HIP(dev_alloc(&d_status, B));
  }
  const wg_preview_fleet_t fleet = {zm.T, nl, 0, d_zc, d_Ktm, d_Ftm};
  // the preview calls of every mode below: the context's gains, or with --heights each gait's own
  auto preview_batch = [&](int n, const double *zx_, const double *zy_, double *com_, hipStream_t s_) {
    return heights ? wg_preview_run_fleet_dev(B, n, &fleet, zx_, zy_, d_state, com_, nullptr, 1, s_)
                   : wg_preview_run_batch_dev(B, n, zx_, zy_, d_state, com_, nullptr, 1, s_);
  };
  // --online: the walk's state blobs and the feeding plan.  Without --ragged every gait has the same n_steps: nothing ends early
  wg_fleet::OnlinePlan plan;
  wg_zmpdisc_state_t *d_walk = nullptr; wg_rel_step_t *d_chunks = nullptr; int *d_cns = nullptr;
  if (K) {
    if (wg_fleet::online_plan(zm, steps, n_steps, B, S, K, &plan, on_device ? &cp.first_steps : nullptr) >= 0) return 1;    // S >= 2: cannot be
    CHECK_HIP(dev_alloc(&d_walk, B));
    if (on_device) {                                          // one call's steps and counts, written in front of every append
      CHECK_HIP(dev_alloc(&d_chunks, (size_t)B * K));
      CHECK_HIP(dev_alloc(&d_cns, B));
      CHECK_HIP(dev_upload(&d_later, cp.later));
      CHECK_HIP(dev_upload(&d_nlater, cp.n_later));
      if (plan.n_calls != cp.n_calls) { fprintf(stderr, "FAILED: %d calls planned, %d lists\n", plan.n_calls, cp.n_calls); return 1; }
    } else {
      CHECK_HIP(dev_upload(&d_chunks, plan.chunks));
      CHECK_HIP(dev_upload(&d_cns, plan.cns));
    }
    if (ragged || on_device) {
      CHECK_HIP(dev_upload(&d_sel, plan.sel));
      CHECK_HIP(dev_alloc(&d_done, B));
    }
    if (!on_device) {
      const std::vector<int> two(B, 2);                       // the begin call takes two steps of every gait
      CHECK_HIP(hipMemcpy(d_ns, two.data(), sizeof(int) * B, hipMemcpyHostToDevice));
    }
  }
  const int n_calls = plan.n_calls;
  hipStream_t st;
  CHECK_HIP(hipStreamCreate(&st));
  double sec = 0.0;
  for (int rep = 0; rep < 2; ++rep) {                          // the second pass is the timed one
    CHECK_HIP(hipMemsetAsync(d_state, 0, sizeof(double) * 8 * B, st));
    if (on_device) CHECK_HIP(hipMemcpyAsync(d_stack, fresh.data(), sizeof(wg_step_stack_t) * B, hipMemcpyHostToDevice, st));
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    if (heights) CHECK_WG(wg_riccati_gains_batch_dev(B, zm.T, d_zc, 1.0, 1e-6, nl, WG_RICCATI_WITHOUT_INITIALPOS, d_Ktm, d_Ftm, d_status, st));
    // --plan: the steps of the call that follows, from the commands: the whole list, or the support foot and the arc
    if (on_device) CHECK_WG(wg_steps_plan_dev(B, cp.ccap, d_cmds, d_ncmds, zm.t_single, zm.t_double, d_stack, S, d_steps, d_ns, st));
    if (!K) {
      CHECK_WG(wg_zmpdisc_batch_dev(&zm, B, S, d_steps, d_ns, d_feet, L, d_zx, d_zy, d_len, st));
      CHECK_WG(preview_batch(Lrun, d_zx, d_zy, d_com, st));
    } else if (ragged || on_device) {
      // the plan says which STEPS each call gives and which gaits it ends; how many samples that makes is the device's business
      CHECK_HIP(hipMemsetAsync(d_done, 0, sizeof(int) * B, st));
      auto follow = [&]() {
        return heights ? wg_preview_follow_fleet_dev(B, L, d_len, d_done, &fleet, d_zx, d_zy, d_state, d_com, nullptr, 1, st)
                       : wg_preview_follow_dev(B, L, d_len, d_done, d_zx, d_zy, d_state, d_com, nullptr, 1, st);
      };
      auto end_selected = [&](int c) -> int {                  // the gaits whose steps ran out with call c
        const int *sel = &plan.sel[(size_t)c * B];
        bool any = false;
        for (int g = 0; g < B; ++g) any = any || sel[g];
        if (!any) return WG_OK;
        const int rc = wg_zmpdisc_end_dev(&zm, B, d_sel + (size_t)c * B, L, d_zx, d_zy, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          nullptr, d_walk, d_len, st);
        return rc != WG_OK ? rc : follow();
      };
      CHECK_WG(wg_zmpdisc_begin_dev(&zm, B, S, d_steps, d_ns, d_feet, L, d_zx, d_zy, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, d_walk, d_len, st));
      CHECK_WG(follow());
      CHECK_WG(end_selected(0));
      for (int c = 0; c < n_calls; ++c) {
        const size_t at = on_device ? 0 : (size_t)c * B;       // --plan: call c's steps are planned into the one chunk
        if (on_device) CHECK_WG(wg_steps_plan_dev(B, K, d_later + (size_t)c * B * K, d_nlater + (size_t)c * B, zm.t_single, zm.t_double,
                                                  d_stack, K, d_chunks, d_cns, st));
        CHECK_WG(wg_zmpdisc_append_dev(&zm, B, K, d_chunks + at * K, d_cns + at, L, d_zx, d_zy, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, nullptr, d_walk, d_len, st));
        CHECK_WG(follow());
        CHECK_WG(end_selected(c + 1));
      }
    } else {
      // every gait has the same support times, hence the same sample count after each call: the host knows it without
      // reading `length` back.  Rows [done, done + n) are safe once the queue holds done + n + nl - 1 samples.
      int done = 0;
      auto preview_upto = [&](int have) -> int {
        const int n = have - nl + 1 - done;
        if (n <= 0) return WG_OK;
        const int rc = preview_batch(n, d_zx + (size_t)done * B, d_zy + (size_t)done * B, d_com + (size_t)done * 6 * B, st);
        done += n;
        return rc;
      };
      CHECK_WG(wg_zmpdisc_begin_dev(&zm, B, S, d_steps, d_ns, d_feet, L, d_zx, d_zy, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, d_walk, d_len, st));
      CHECK_WG(preview_upto(plan.len_after[0]));
      for (int c = 0; c < n_calls; ++c) {
        CHECK_WG(wg_zmpdisc_append_dev(&zm, B, K, d_chunks + (size_t)c * B * K, d_cns + (size_t)c * B, L, d_zx, d_zy, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, nullptr, d_walk, d_len, st));
        CHECK_WG(preview_upto(plan.len_after[(size_t)(c + 1) * B]));
      }
      CHECK_WG(wg_zmpdisc_end_dev(&zm, B, nullptr, L, d_zx, d_zy, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_walk,
                                  d_len, st));
      CHECK_WG(preview_upto(L));
      if (done != Lrun) { fprintf(stderr, "FAILED: previewed %d rows of %d\n", done, Lrun); return 1; }
    }
    CHECK_HIP(hipStreamSynchronize(st));
    sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  if (audit) {
    const int qcap = 2 * S + 8 > 64 ? 2 * S + 8 : 64;         // two polytopes per step, the rest phases either side
    const wg_sole_t sole{0.24, 0.138, 0.02, 0.02};
    std::vector<double> time_h(L);
    { double t = 0.0; for (int l = 0; l < L; ++l) { t += zm.T; time_h[l] = t - zm.T; } }
    std::vector<int> len_run(B);
    for (int g = 0; g < B; ++g) len_run[g] = len_g[g] - nl + 1;
    double *d_time, *d_left, *d_right, *d_ts, *d_te, *d_zmp2; int *d_lty, *d_count, *d_len_run;
    wg_zmp_polytope_t *d_queues;
    wg_fleet::FleetAudit ref, real;
    CHECK_HIP(dev_upload(&d_time, time_h));
    CHECK_HIP(dev_upload(&d_len_run, len_run));
    CHECK_HIP(dev_alloc(&d_left, (size_t)L * 6 * B));
    CHECK_HIP(dev_alloc(&d_right, (size_t)L * 6 * B));
    CHECK_HIP(dev_alloc(&d_lty, (size_t)L * B));
    CHECK_HIP(dev_alloc(&d_zmp2, (size_t)Lrun * 2 * B));
    CHECK_HIP(dev_alloc(&d_queues, (size_t)B * qcap));
    CHECK_HIP(dev_alloc(&d_ts, (size_t)B * qcap));
    CHECK_HIP(dev_alloc(&d_te, (size_t)B * qcap));
    CHECK_HIP(dev_alloc(&d_count, B));
    CHECK_HIP(dev_alloc(&ref.d_audit, B));
    CHECK_HIP(dev_alloc(&real.d_audit, B));
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t0 = std::chrono::steady_clock::now();
    CHECK_WG(wg_zmpdisc_full_batch_dev(&zm, B, S, d_steps, d_ns, d_feet, L, nullptr, nullptr, nullptr, nullptr, d_left, d_lty, d_right, nullptr,
                                       d_len, st));
    CHECK_WG(wg_foot_constraints_batch_dev(B, L, d_len, d_time, d_left, d_lty, d_right, sole.sole_w, sole.sole_h, sole.constraint_x,
                                           sole.constraint_y, qcap, d_queues, d_ts, d_te, d_count, st));
    CHECK_WG(wg_zmp_audit_dev(B, L, d_len, d_time, d_zx, d_zy, B, qcap, d_queues, d_ts, d_te, d_count, ref.d_audit, nullptr, st));
    // the preview once more from rest, this time asked for the ZMP it realises; the CoM it rewrites is the same
    CHECK_HIP(hipMemsetAsync(d_state, 0, sizeof(double) * 8 * B, st));
    CHECK_WG(heights ? wg_preview_run_fleet_dev(B, Lrun, &fleet, d_zx, d_zy, d_state, d_com, d_zmp2, 1, st)
                     : wg_preview_run_batch_dev(B, Lrun, d_zx, d_zy, d_state, d_com, d_zmp2, 1, st));
    CHECK_WG(wg_zmp_audit_dev(B, Lrun, d_len_run, d_time, d_zmp2, d_zmp2 + B, 2LL * B, qcap, d_queues, d_ts, d_te, d_count, real.d_audit, nullptr, st));
    CHECK_HIP(hipStreamSynchronize(st));
    const double sec_a = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("kajita_fleet: feet, queues (<= %d polytopes), the preview's ZMP and two audits of %d walks in %.2f ms\n", qcap, B, sec_a * 1e3);
    if (wg_fleet::audit_report("kajita_fleet", "the ZMP reference", &ref, B, L, len_g.data(), time_h.data(), d_zx, d_zy, B, qcap, d_queues, d_ts,
                               d_te, d_count)) return 1;
    if (wg_fleet::audit_report("kajita_fleet", "the ZMP the preview realises (zmp2_tm in place, pitch 2 B)", &real, B, Lrun, len_run.data(),
                               time_h.data(), d_zmp2, d_zmp2 + B, 2LL * B, qcap, d_queues, d_ts, d_te, d_count)) return 1;
  }
  if (K) {                                                     // every gait must have arrived at the whole sequence's length
    std::vector<int> len_h(B);
    CHECK_HIP(hipMemcpy(len_h.data(), d_len, sizeof(int) * B, hipMemcpyDeviceToHost));
    for (int g = 0; g < B; ++g)
      if (len_h[g] != len_g[g]) { fprintf(stderr, "FAILED: gait %d ended with length %d, not %d\n", g, len_h[g], len_g[g]); return 1; }
    CHECK_HIP(hipMemcpy(d_ns, n_steps.data(), sizeof(int) * B, hipMemcpyHostToDevice));
    if (ragged || on_device) {                                 // ... and the preview at its last safe row
      CHECK_HIP(hipMemcpy(len_h.data(), d_done, sizeof(int) * B, hipMemcpyDeviceToHost));
      for (int g = 0; g < B; ++g)
        if (len_h[g] != len_g[g] - nl + 1) { fprintf(stderr, "FAILED: gait %d previewed %d rows of %d\n", g, len_h[g], len_g[g] - nl + 1); return 1; }
    }
  }
  if (heights) {                                               // every gait's gains were made
    std::vector<int> status(B);
    CHECK_HIP(hipMemcpy(status.data(), d_status, sizeof(int) * B, hipMemcpyDeviceToHost));
    for (int g = 0; g < B; ++g)
      if (status[g] != WG_OK) { fprintf(stderr, "FAILED: the gains of gait %d (zc = %g): status %d\n", g, zc[g], status[g]); return 1; }
  }
  std::vector<double> com_d((size_t)Lrun * 6 * B);
  CHECK_HIP(hipMemcpy(com_d.data(), d_com, sizeof(double) * com_d.size(), hipMemcpyDeviceToHost));
  // a gait against the host-pointer entry points, one gait at a time (with --heights: configured with its own wg_riccati_gains)
  std::vector<double> com_h;
  int len0 = 0;
  auto check_gait = [&](int g) -> int {
    if (heights) {
      CHECK_WG(wg_riccati_gains(zm.T, zc[g], 1.0, 1e-6, nl, WG_RICCATI_WITHOUT_INITIALPOS, Kg, F.data()));
      const wg_preview_gains_t own = {zm.T, zc[g], Kg[0], {Kg[1], Kg[2], Kg[3]}, nl, 0};
      CHECK_WG(wg_preview_configure(&own, F.data()));
    }
    const int Lg = len_g[g], Lrun_g = Lg - nl + 1;
    std::vector<double> zmp((size_t)Lg * 2), state_h(8, 0.0), zx(Lg), zy(Lg);
    com_h.assign((size_t)Lrun_g * 6, 0.0);
    CHECK_WG(wg_zmpdisc_batch(&zm, 1, S, &steps[(size_t)g * S], &n_steps[g], &feet[(size_t)g * 6], Lg, zmp.data(), nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, &len0));
    for (int l = 0; l < Lg; ++l) { zx[l] = zmp[2 * l]; zy[l] = zmp[2 * l + 1]; }
    CHECK_WG(wg_preview_run_batch(1, Lrun_g, zx.data(), zy.data(), state_h.data(), com_h.data(), nullptr, 1));
    for (int l = 0; l < Lrun_g; ++l)
      for (int c = 0; c < 6; ++c)
        if (com_d[((size_t)l * 6 + c) * B + g] != com_h[(size_t)l * 6 + c]) {
          fprintf(stderr, "FAILED: device chain of gait %d differs from the host entry points at step %d\n", g, l);
          return 1;
        }
    return 0;
  };
  if (heights && B > 1 && check_gait(B - 1)) return 1;
  if (check_gait(0)) return 1;                                 // last: com_h and len0 below are gait 0's
  if (heights)
    printf("kajita_fleet: CoM heights %.4f .. %.4f m, the gains of %d gaits made on the device, all status 0; gaits 0 and %d == host entry "
           "points with their own gains\n", zc[0], zc[B - 1], B, B - 1);
  const int Lrun0 = len_g[0] - nl + 1;
  if (ragged) {                                                // each gait's own rows, gait by gait
    std::vector<double> own;
    double far = 0.0;
    int n_min = S, n_max = 0;
    for (int g = 0; g < B; ++g) {
      const int rows = len_g[g] - nl + 1;
      for (int l = 0; l < rows; ++l)
        for (int c = 0; c < 6; ++c) own.push_back(com_d[((size_t)l * 6 + c) * B + g]);
      const double x = com_d[((size_t)(rows - 1) * 6) * B + g];
      far = x > far ? x : far;
      n_min = n_steps[g] < n_min ? n_steps[g] : n_min;
      n_max = n_steps[g] > n_max ? n_steps[g] : n_max;
    }
    const unsigned long long sum = wg_fleet::fnv1a64(own.data(), own.size() * sizeof(double));
    printf("kajita_fleet: %d ragged walks of %d..%d steps (%d..%d samples) in %.2f ms = %.0f walks/s; gait 0 ends at x = %.4f m (%d samples), "
           "farthest %.2f m; device chain == host entry points; checksum %016llx\n", B, n_min, n_max, Lmin, L, sec * 1e3, B / sec,
           com_h[(size_t)(Lrun0 - 1) * 6], len0, far, sum);
    wg_shutdown();
    return 0;
  }
  double far = 0.0;
  for (int g = 0; g < B; ++g) { const double x = com_d[((size_t)(Lrun - 1) * 6) * B + g]; far = x > far ? x : far; }
  const unsigned long long sum = wg_fleet::fnv1a64(com_d.data(), com_d.size() * sizeof(double));
  printf("kajita_fleet: %d walks of %d steps (%d samples each) in %.2f ms = %.0f walks/s; gait 0 ends at x = %.4f m (%d samples), "
         "farthest %.2f m; device chain == host entry points; checksum %016llx\n", B, S, L, sec * 1e3, B / sec,
         com_h[(size_t)(Lrun0 - 1) * 6], len0, far, sum);
  wg_shutdown();
  return 0;
}
