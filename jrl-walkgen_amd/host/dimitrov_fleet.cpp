// dimitrov_fleet.cpp -- the Dimitrov-2008 fleet path from plain C++ through the C ABI (no Python, no PyTorch): B step sequences
// in device memory -> wg_zmpdisc_full_batch_dev (feet trajectories, time-major) -> wg_foot_constraints_batch_dev (polytope
// queues) -> wg_dimitrov_walk_dev (n ticks: queue walk + fused tick), nothing leaves the device in between.  The Dimitrov twin of
// kajita_fleet.cpp.  Prints one line with walks/s, ticks/s and a checksum (FNV-1a, 64 bit) of the final states.
//
// With --online K the same walks are fed K steps per call instead, the twin of kajita_fleet --online: wg_zmpdisc_begin_dev on the
// first two steps (feet outputs only), then { wg_zmpdisc_append_dev on the next K; wg_foot_constraints_append_dev;
// wg_dimitrov_walk_dev on the ticks that became safe (wg_dimitrov_walk_safe_ticks, chained by wg_dimitrov_walk_time) } until the
// steps run out -- a gait of a ragged fleet whose steps have run out is ended (wg_zmpdisc_end_dev with `select`) while the others
// walk on -- then a last append of the queues and the remaining ticks.  Every sample is classified once, and the final states --
// hence the checksum -- are those of the whole-sequence mode.  ("the walk alone" is then the sum of the walk pieces, by events.)
//
// With --online K --follow the walk pieces are ONE wg_dimitrov_follow_dev behind every feeding instead: every gait has its own clock
// and tick count on the device and ticks where its own queue allows (`have` = the done array of wg_foot_constraints_append_dev,
// `walk` = the state blobs, tick_cap = --ticks).  The host does no arithmetic on lengths for walking -- no minimum over the gaits
// still walking, no wg_dimitrov_walk_safe_ticks, no wg_dimitrov_walk_time: it sizes the call's rounds from the steps it has just
// fed (the longest duration any gait was given, over the tick period, plus one; behind an end call: --ticks).  ran_out is cleared
// once and ORed on the device.  The final states, hence the checksum, are again those of the whole-sequence mode.
// With --ragged gait g of the built-in fleet walks its own number of steps, between S/2 and S (as kajita_fleet --ragged).
//
// With --plan the built-in fleet's steps are decided on the device instead (the twin of kajita_fleet --plan): the only step input
// uploaded is a command list per gait (wg_fleet::command_plan), and wg_steps_plan_dev writes the steps into the array wg_zmpdisc_*
// reads, on the same stream -- the whole list in front of wg_zmpdisc_full_batch_dev, or with --online K the support foot and the
// arc in front of wg_zmpdisc_begin_dev and K commands in front of every wg_zmpdisc_append_dev.  --plan-host is its host-fed twin:
// the same lists through wg_steps_plan and the upload path.  Both print the same checksum.
//
// With --heights LO:HI gait g walks at its own CoM height, h = LO + (HI - LO) g / (B - 1): a model per gait.  The constants are made
// on the device (wg_dimitrov_constants_batch_dev on the walk's stream, in front of every pass) and every walk or follow call is
// its fleet form (wg_dimitrov_walk_fleet_dev / wg_dimitrov_follow_fleet_dev, model_of[g] = g), in every mode above.  The program
// checks every model's status and holds gaits 0 and B - 1 to a context configured with their own model: one wg_dimitrov_walk_dev
// over the gait's final queue.  LO = HI = 0.80 prints the checksum of the run without the option.
//
// With --robots LO:HI gait g is a robot of its own size, s = LO + (HI - LO) g / (B - 1): it implies --heights (h = 0.80 s) and scales
// the sole with its margins, foot_b / h / f, the step height and the step lengths of the generated walks by s; the single support
// comes from a table of multiples of T, 0.05 s per tenth of s around 0.7 s, so every phase keeps a whole sample count.  The producers
// are then their fleet forms on the walk's stream -- wg_steps_plan_fleet_dev, wg_zmpdisc_*_fleet_dev (model_of NULL: a model per
// gait), wg_foot_constraints_fleet_dev / _append_fleet_dev -- in every mode above but --fleet.  Gaits 0 and B - 1 are held to the
// one-model path, each alone: wg_zmpdisc_full_batch_dev with its own model, wg_foot_constraints_batch_dev with its own sole, one
// walk on a context configured with its own height.  LO = HI = 1 prints the checksum of the run without the option.
//
// With --online K [--follow] --audit the feeding calls also write the ZMP reference (zmp_x_tm / zmp_y_tm), and behind every
// wg_foot_constraints_append_dev a wg_zmp_audit_append_dev folds the new samples into one verdict per gait, against the queue as
// it grows.  At the end the verdicts must be the bytes of one wg_zmp_audit_dev over the finished walks, and gaits 0 and B - 1 those
// of the host twin wg_zmp_audit; the fleet's least margin, its gait and time, and the violated count are printed.
//
//   dimitrov_fleet [--batch B] [--steps S] [--ticks K] [--solver 0|1|2] [--fleet FILE] [--online K [--follow] [--audit]] [--ragged]
//                  [--plan | --plan-host] [--heights LO:HI | --robots LO:HI]
//
// --fleet FILE runs a fleet somebody else drew instead of the built-in one (tests/test_dimitrov_walk_gpu.py compares the
// checksum with its own run of the same fleet): int32 B, int32 smax, wg_zmpdisc_model_t, B x smax wg_rel_step_t, B int32
// n_steps, B x 6 doubles init_feet, in the machine's byte order.
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <random>

#include "wg_fleet.hpp"

using wg_fleet::dev_alloc;
using wg_fleet::dev_upload;

int main(int argc, char **argv) {
  int B = 4096, S = 8, K = 40, solver = WG_DIMITROV_PLDP, online = 0;
  bool follow = false, ragged = false, heights = false, robots = false, audit = false;
  double h_lo = 0.0, h_hi = 0.0, r_lo = 1.0, r_hi = 1.0;
  int planned = 0;                                            // 1: --plan (steps planned on the device), 2: --plan-host
  const char *fleet = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--batch") && i + 1 < argc) B = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--steps") && i + 1 < argc) S = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--ticks") && i + 1 < argc) K = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--solver") && i + 1 < argc) solver = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--fleet") && i + 1 < argc) fleet = argv[++i];
    else if (!strcmp(argv[i], "--follow")) follow = true;
    else if (!strcmp(argv[i], "--ragged")) ragged = true;
    else if (!strcmp(argv[i], "--audit")) audit = true;
    else if (!strcmp(argv[i], "--plan")) planned = 1;
    else if (!strcmp(argv[i], "--plan-host")) planned = 2;
    else if (!strcmp(argv[i], "--heights") && i + 1 < argc) {
      heights = sscanf(argv[++i], "%lf:%lf", &h_lo, &h_hi) == 2;
      if (!heights || !(h_lo > 0.0) || !(h_hi >= h_lo) || !(h_hi < 1e3)) { fprintf(stderr, "FAILED: need --heights LO:HI with 0 < LO <= HI\n"); return 1; }
    }
    else if (!strcmp(argv[i], "--robots") && i + 1 < argc) {
      robots = sscanf(argv[++i], "%lf:%lf", &r_lo, &r_hi) == 2;
      if (!robots || !(r_lo > 0.0) || !(r_hi >= r_lo) || !(r_hi < 1e3)) { fprintf(stderr, "FAILED: need --robots LO:HI with 0 < LO <= HI\n"); return 1; }
    }
    else if (!strcmp(argv[i], "--online") && i + 1 < argc) { online = atoi(argv[++i]); if (online < 1 || online > WG_ZMPDISC_MAX_STEPS) { fprintf(stderr, "FAILED: need 1 <= --online K <= %d\n", WG_ZMPDISC_MAX_STEPS); return 1; } }
  }
  if (follow && !online) { fprintf(stderr, "FAILED: --follow needs --online K\n"); return 1; }
  if (audit && !online) { fprintf(stderr, "FAILED: --audit needs --online K\n"); return 1; }
  if (planned && (ragged || fleet || S < 4)) { fprintf(stderr, "FAILED: --plan needs steps >= 4, no --ragged and no --fleet\n"); return 1; }
  if (robots && (fleet || heights)) { fprintf(stderr, "FAILED: --robots goes with neither --fleet nor --heights (it implies them)\n"); return 1; }
  const bool on_device = planned == 1;
  wg_fleet::CommandPlan cp;
  wg_zmpdisc_model_t zm;
  wg_zmpdisc_defaults(&zm);
  zm.t_single = 0.7; zm.t_double = 0.13;                       // phase boundaries off the 0.1 s grid of the previewed instants
  std::vector<wg_rel_step_t> steps;
  std::vector<int> n_steps;
  std::vector<double> feet;
  // --robots: a size, a walk model and a sole per gait (without it: size 1, zm and the one sole for every gait)
  std::vector<double> size_of;
  std::vector<wg_zmpdisc_model_t> zms;
  std::vector<wg_sole_t> soles;
  const wg_sole_t sole{0.24, 0.138, 0.02, 0.02};
  if (robots) {
    if (B < 1) { fprintf(stderr, "FAILED: need B >= 1\n"); return 1; }
    static const double single[9] = {0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9};   // multiples of T, by the tenths of s around 1
    size_of.resize(B); zms.assign(B, zm); soles.assign(B, sole);
    for (int g = 0; g < B; ++g) {
      const double s = size_of[g] = B > 1 ? r_lo + (r_hi - r_lo) * g / (B - 1) : r_lo;
      const long k = lround((s - 1.0) * 10.0);
      wg_zmpdisc_model_t &m = zms[g];
      m.t_single = single[(k < -4 ? -4 : k > 4 ? 4 : k) + 4];
      m.step_height *= s; m.foot_b *= s; m.foot_h *= s; m.foot_f *= s;
      soles[g] = wg_sole_t{sole.sole_w * s, sole.sole_h * s, sole.constraint_x * s, sole.constraint_y * s};
    }
  }
  auto zm_of = [&](int g) -> const wg_zmpdisc_model_t & { return robots ? zms[g] : zm; };
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
      if (ragged) {                                             // S/2 .. S steps, at least the two the begin call takes
        const int lo = S / 2 > 2 ? S / 2 : 2;
        n_steps[g] = lo + (int)(std::mt19937_64(7700 + g)() % (unsigned)(S - lo + 1));
      }
      std::mt19937_64 rng(20080 + g);
      std::uniform_real_distribution<double> len(0.1, 0.25);
      double side = (g & 1) ? 1.0 : -1.0;
      for (int i = 0; i < S; ++i) {
        wg_rel_step_t &s = steps[(size_t)g * S + i];
        memset(&s, 0, sizeof s);
        const bool ends = i == 0 || i == n_steps[g] - 1;
        s.sx = ends ? 0.0 : len(rng) * (robots ? size_of[g] : 1.0);
        s.sy = side * (i == 0 ? 0.105 : 0.21);
        s.ss_time = zm_of(g).t_single; s.ds_time = 0.0; s.step_type = 1;
        side = -side;
      }
      const double f[6] = {0.0, 0.095, 0.0, 0.0, -0.095, 0.0};
      memcpy(&feet[(size_t)g * 6], f, sizeof f);
    }
    // --plan, --plan-host: the steps come from command lists instead.  On the host they are the twin's input, and with --plan what
    // the buffers are sized by (counts and times only) -- none of them is uploaded then
    if (planned && (wg_fleet::command_plan(B, S, online, &cp, robots ? size_of.data() : nullptr) >= 0 ||
                    wg_fleet::command_steps(cp, B, S, zm.t_single, zm.t_double, on_device, &steps, &n_steps, robots ? zms.data() : nullptr) >= 0)) {
      fprintf(stderr, "FAILED: the command lists do not give %d steps\n", S);
      return 1;
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
    const int L = wg_zmpdisc_length(&zm_of(g), &steps[(size_t)g * S], n_steps[g]);
    if (L < 1) { fprintf(stderr, "FAILED: gait %d: sequence refused (%d)\n", g, L); return 1; }
    lcap = L > lcap ? L : lcap;
  }
  std::vector<double> time(lcap);
  { double t = 0.0; for (int l = 0; l < lcap; ++l) { t += zm.T; time[l] = t - zm.T; } }       // the running sum of the periods, from 0
  const int qcap = 2 * S + 8 > 64 ? 2 * S + 8 : 64;             // two polytopes per step, the rest phases either side

  wg_rel_step_t *d_steps; int *d_ns, *d_len, *d_lty, *d_count, *d_ran; double *d_feet, *d_time, *d_left, *d_right, *d_ts, *d_te;
  wg_zmp_polytope_t *d_queues; wg_dimitrov_state_t *d_states;
  const size_t row = (size_t)lcap * B, nq = (size_t)B * qcap;
  wg_step_cmd_t *d_cmds = nullptr, *d_later = nullptr; wg_step_stack_t *d_stack = nullptr; int *d_ncmds = nullptr, *d_nlater = nullptr;
  const std::vector<wg_step_stack_t> fresh(B, wg_step_stack_t{1, 0, 0, 0});
  if (on_device) {                                            // the steps' array is only written by the device
    CHECK_HIP(dev_alloc(&d_steps, steps.size()));
    CHECK_HIP(hipMemset(d_steps, 0, sizeof(wg_rel_step_t) * steps.size()));
    CHECK_HIP(dev_alloc(&d_ns, B));
    CHECK_HIP(dev_upload(&d_cmds, cp.whole));
    CHECK_HIP(dev_upload(&d_ncmds, online ? std::vector<int>(B, 2) : cp.n_whole));
    CHECK_HIP(dev_alloc(&d_stack, B));
  } else {
    CHECK_HIP(dev_upload(&d_steps, steps));
    CHECK_HIP(dev_upload(&d_ns, n_steps));
  }
  CHECK_HIP(dev_upload(&d_feet, feet));
  CHECK_HIP(dev_upload(&d_time, time));
  CHECK_HIP(dev_alloc(&d_len, B));
  CHECK_HIP(dev_alloc(&d_count, B));
  CHECK_HIP(dev_alloc(&d_ran, B));
  CHECK_HIP(dev_alloc(&d_lty, row));
  CHECK_HIP(dev_alloc(&d_left, 6 * row));
  CHECK_HIP(dev_alloc(&d_right, 6 * row));
  CHECK_HIP(dev_alloc(&d_ts, nq));
  CHECK_HIP(dev_alloc(&d_te, nq));
  CHECK_HIP(dev_alloc(&d_queues, nq));
  CHECK_HIP(dev_alloc(&d_states, B));
  // --audit: the ZMP reference of the feeding calls (without it they are not asked for it), the audit's own done array, the verdicts
  double *d_zx = nullptr, *d_zy = nullptr; int *d_adone = nullptr;
  wg_fleet::FleetAudit fa;
  if (audit) {
    CHECK_HIP(dev_alloc(&d_zx, row));
    CHECK_HIP(dev_alloc(&d_zy, row));
    CHECK_HIP(dev_alloc(&d_adone, B));
    CHECK_HIP(dev_alloc(&fa.d_audit, B));
  }
  // --heights: a model per gait; the blocks and the status are written by the device in front of every pass
  double *d_h = nullptr; unsigned char *d_blocks = nullptr; int *d_status = nullptr, *d_model_of = nullptr;
  std::vector<double> h_of(B, dm.com_height);
  wg_dimitrov_fleet_t dfl{dm.N, dm.solver, B, 0, dm.T, dm.Tctrl, nullptr, nullptr};
  if (robots) { heights = true; h_lo = dm.com_height * r_lo; h_hi = dm.com_height * r_hi; }
  if (heights) {
    std::vector<int> ident(B);
    for (int g = 0; g < B; ++g) { h_of[g] = robots ? dm.com_height * size_of[g] : B > 1 ? h_lo + (h_hi - h_lo) * g / (B - 1) : h_lo; ident[g] = g; }
    CHECK_HIP(dev_upload(&d_h, h_of));
    CHECK_HIP(dev_upload(&d_model_of, ident));
    CHECK_HIP(dev_alloc(&d_blocks, (size_t)B * wg_dimitrov_constants_bytes()));
    CHECK_HIP(dev_alloc(&d_status, B));
    dfl.blocks = d_blocks; dfl.model_of = d_model_of;
  }
  // the walk and follow calls of every mode below: the configured model, or with --heights each gait's own
  auto walk = [&](double t_, int n_, hipStream_t s_) {
    return heights ? wg_dimitrov_walk_fleet_dev(B, &dfl, qcap, d_queues, d_ts, d_te, d_count, t_, n_, d_states, nullptr, d_ran, 0, s_)
                   : wg_dimitrov_walk_dev(B, qcap, d_queues, d_ts, d_te, d_count, t_, n_, d_states, nullptr, d_ran, 0, s_);
  };
  // the producers of every mode below: the one-model calls, or with --robots their fleet forms over a model, times and a sole per gait
  wg_zmpdisc_model_t *d_zms = nullptr; wg_sole_t *d_soles = nullptr; double *d_ss = nullptr, *d_ds = nullptr;
  wg_zmpdisc_fleet_t zfl{zm, B, 0, nullptr, nullptr};
  if (robots) {
    std::vector<double> ss(B), ds(B);
    for (int g = 0; g < B; ++g) { ss[g] = zms[g].t_single; ds[g] = zms[g].t_double; }
    CHECK_HIP(dev_upload(&d_zms, zms));
    CHECK_HIP(dev_upload(&d_soles, soles));
    CHECK_HIP(dev_upload(&d_ss, ss));
    CHECK_HIP(dev_upload(&d_ds, ds));
    zfl.models = d_zms;
  }
  auto plan_steps = [&](int ccap_, const wg_step_cmd_t *cmds_, const int *n_, int smax_, wg_rel_step_t *steps_, int *ns_, hipStream_t s_) {
    return robots ? wg_steps_plan_fleet_dev(B, ccap_, cmds_, n_, d_ss, d_ds, d_stack, smax_, steps_, ns_, s_)
                  : wg_steps_plan_dev(B, ccap_, cmds_, n_, zm.t_single, zm.t_double, d_stack, smax_, steps_, ns_, s_);
  };
  auto zd_full = [&](hipStream_t s_) {
    return robots ? wg_zmpdisc_full_fleet_dev(&zfl, B, S, d_steps, d_ns, d_feet, lcap, nullptr, nullptr, nullptr, nullptr, d_left, d_lty, d_right, nullptr, d_len, s_)
                  : wg_zmpdisc_full_batch_dev(&zm, B, S, d_steps, d_ns, d_feet, lcap, nullptr, nullptr, nullptr, nullptr, d_left, d_lty, d_right, nullptr, d_len, s_);
  };
  auto fc_batch = [&](hipStream_t s_) {
    return robots ? wg_foot_constraints_fleet_dev(B, lcap, d_len, d_time, d_left, d_lty, d_right, d_soles, qcap, d_queues, d_ts, d_te, d_count, s_)
                  : wg_foot_constraints_batch_dev(B, lcap, d_len, d_time, d_left, d_lty, d_right, sole.sole_w, sole.sole_h, sole.constraint_x,
                                                  sole.constraint_y, qcap, d_queues, d_ts, d_te, d_count, s_);
  };
  std::vector<wg_dimitrov_state_t> states(B);
  memset(states.data(), 0, sizeof(wg_dimitrov_state_t) * B);
  for (int g = 0; g < B; ++g) states[g].starting = 1;
  // --online: the walk's state blobs, the feeding plan (the steps after the first two regrouped call by call, what each call
  // leaves of every gait, which gaits end behind it), and each walk piece's ran_out
  wg_fleet::OnlinePlan plan;
  wg_zmpdisc_state_t *d_walk = nullptr; wg_rel_step_t *d_chunks = nullptr; int *d_cns = nullptr, *d_two = nullptr, *d_sel = nullptr, *d_done = nullptr;
  std::vector<int> ran_pieces;
  std::vector<hipEvent_t> ev;
  if (online) {
    const int bad = wg_fleet::online_plan(zm, steps, n_steps, B, S, online, &plan, on_device ? &cp.first_steps : nullptr, robots ? zms.data() : nullptr);
    if (bad >= 0) { fprintf(stderr, "FAILED: gait %d: --online needs two steps to begin with\n", bad); return 1; }
    CHECK_HIP(dev_alloc(&d_walk, B));
    if (on_device) {                                          // one call's steps and counts, written in front of every append
      CHECK_HIP(dev_alloc(&d_chunks, (size_t)B * online));
      CHECK_HIP(dev_alloc(&d_cns, B));
      CHECK_HIP(dev_upload(&d_later, cp.later));
      CHECK_HIP(dev_upload(&d_nlater, cp.n_later));
      if (plan.n_calls != cp.n_calls) { fprintf(stderr, "FAILED: %d calls planned, %d lists\n", plan.n_calls, cp.n_calls); return 1; }
    } else {
      CHECK_HIP(dev_upload(&d_chunks, plan.chunks));
      CHECK_HIP(dev_upload(&d_cns, plan.cns));
    }
    CHECK_HIP(dev_upload(&d_sel, plan.sel));
    CHECK_HIP(dev_upload(&d_two, std::vector<int>(B, 2)));
    CHECK_HIP(dev_alloc(&d_done, B));
    ran_pieces.reserve((size_t)(2 * plan.n_calls + 3) * B);   // never reallocated: pieces are copied into it asynchronously
  }
  // --follow: a clock and a tick count per gait, and the rounds of the follow call behind each feeding: the longest duration any
  // gait was fed (begin: the rest phase and the second step; the first step is where the walk stands), in ticks, plus one
  double *d_clock = nullptr; int *d_ticks = nullptr;
  std::vector<int> rounds;
  if (follow) {
    CHECK_HIP(dev_alloc(&d_clock, B));
    CHECK_HIP(dev_alloc(&d_ticks, B));
    auto dur = [&](const wg_rel_step_t &s, int g) { return s.ds_time != 0.0 ? s.ds_time + s.ss_time : zm_of(g).t_double + zm_of(g).t_single; };
    rounds.assign(plan.n_calls + 1, 0);
    for (int c = 0; c <= plan.n_calls; ++c) {
      double longest = 0.0;
      for (int g = 0; g < B; ++g) {
        double d = 0.0;
        const int first = on_device ? cp.first_steps[g] : 2;   // the steps the begin call takes
        if (c == 0) {
          for (int i = 1; i < first; ++i) d += dur(steps[(size_t)g * S + i], g);
          d = 2 * zm_of(g).preview_time + d;
        } else if (on_device) {
          for (int i = 0; i < plan.cns[(size_t)(c - 1) * B + g]; ++i) d += dur(steps[(size_t)g * S + first + (c - 1) * online + i], g);
        } else for (int i = 0; i < plan.cns[(size_t)(c - 1) * B + g]; ++i) d += dur(plan.chunks[((size_t)(c - 1) * B + g) * online + i], g);
        longest = d > longest ? d : longest;
      }
      const double r = longest / dm.T + 1.0;
      rounds[c] = r < (double)K ? (int)r : K;
    }
  }
  const int n_calls = plan.n_calls;
  const std::vector<int> &sel = plan.sel, &len_after = plan.len_after, &len_ended = plan.len_ended;
  hipStream_t st;
  CHECK_HIP(hipStreamCreate(&st));
  double sec = 0.0, sec_walk = 0.0;
  for (int rep = 0; rep < 2; ++rep) {                          // the second pass is the timed one
    CHECK_HIP(hipMemcpyAsync(d_states, states.data(), sizeof(wg_dimitrov_state_t) * B, hipMemcpyHostToDevice, st));
    if (on_device) CHECK_HIP(hipMemcpyAsync(d_stack, fresh.data(), sizeof(wg_step_stack_t) * B, hipMemcpyHostToDevice, st));
    if (heights) CHECK_WG(wg_dimitrov_constants_batch_dev(B, &dm, d_h, nullptr, nullptr, d_blocks, d_status, st));
    CHECK_HIP(hipStreamSynchronize(st));
    if (online) {
      // what the host knows of the fleet: every gait's samples (cur), which have ended, the samples the queues hold (done)
      std::vector<int> cur(B, 0), done(B, 0);
      std::vector<char> ended(B, 0);
      double t = 0.0;
      int ticks = 0;
      ran_pieces.clear();
      int max_ticks = 0;                                       // --follow: the rounds of the next follow call
      for (hipEvent_t e : ev) (void)hipEventDestroy(e);
      ev.clear();
      // the queues up to the feet's new lengths, then the ticks that became safe: those whose N instants lie at or before the
      // last sample of the shortest gait still walking (a gait that has ended has its final queue)
      auto grow_and_walk = [&]() -> int {
        int first = done[0], have = -1;
        for (int g = 0; g < B; ++g) {
          first = done[g] < first ? done[g] : first;
          if (!ended[g] && (have < 0 || cur[g] < have)) have = cur[g];
          done[g] = cur[g];
        }
        if (int rc = robots ? wg_foot_constraints_append_fleet_dev(B, lcap, first, d_done, d_len, d_time, d_left, d_lty, d_right, d_soles, qcap,
                                                                   d_queues, d_ts, d_te, d_count, st)
                            : wg_foot_constraints_append_dev(B, lcap, first, d_done, d_len, d_time, d_left, d_lty, d_right, sole.sole_w, sole.sole_h,
                                                             sole.constraint_x, sole.constraint_y, qcap, d_queues, d_ts, d_te, d_count, st)) return rc;
        if (audit)                                             // the new samples against the queue they have just extended
          if (int rc = wg_zmp_audit_append_dev(B, lcap, first, d_adone, d_len, d_time, d_zx, d_zy, B, qcap, d_queues, d_ts, d_te, d_count,
                                               fa.d_audit, nullptr, st)) return rc;
        if (follow) {                                          // every gait over the ticks its own queue has made safe
          hipEvent_t e0, e1;
          if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return WG_ERR_HIP;
          ev.push_back(e0); ev.push_back(e1);
          (void)hipEventRecord(e0, st);
          if (int rc = heights ? wg_dimitrov_follow_fleet_dev(B, &dfl, qcap, d_queues, d_ts, d_te, d_count, lcap, d_time, d_done, d_walk, 0,
                                                              d_clock, d_ticks, K, max_ticks, d_states, nullptr, d_ran, 0, st)
                               : wg_dimitrov_follow_dev(B, qcap, d_queues, d_ts, d_te, d_count, lcap, d_time, d_done, d_walk, 0, d_clock, d_ticks,
                                                        K, max_ticks, d_states, nullptr, d_ran, 0, st)) return rc;
          (void)hipEventRecord(e1, st);
          return WG_OK;
        }
        int n = K - ticks;
        if (have > 0) {
          const int safe = wg_dimitrov_walk_safe_ticks(t, time[have - 1]);
          if (safe < 0) return safe;
          n = safe < n ? safe : n;
        }
        if (n <= 0) return WG_OK;
        hipEvent_t e0, e1;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return WG_ERR_HIP;
        ev.push_back(e0); ev.push_back(e1);
        (void)hipEventRecord(e0, st);
        if (int rc = walk(t, n, st)) return rc;
        (void)hipEventRecord(e1, st);
        ran_pieces.resize(ran_pieces.size() + B);             // ran_out is cleared by every walk: kept piece by piece, ORed below
        if (hipMemcpyAsync(ran_pieces.data() + ran_pieces.size() - B, d_ran, sizeof(int) * B, hipMemcpyDeviceToHost, st) != hipSuccess) return WG_ERR_HIP;
        t = wg_dimitrov_walk_time(t, n);
        ticks += n;
        return WG_OK;
      };
      auto end_those_out_of_steps = [&](int c) -> int {
        bool any = false;
        for (int g = 0; g < B; ++g)
          if (sel[(size_t)c * B + g]) { any = true; ended[g] = 1; cur[g] = len_ended[g]; }
        if (!any) return WG_OK;
        max_ticks = K;                                         // an ended gait's queue is final: whatever it has left
        if (int rc = robots ? wg_zmpdisc_end_fleet_dev(&zfl, B, d_sel + (size_t)c * B, lcap, d_zx, d_zy, nullptr, nullptr, d_left, d_lty,
                                                       d_right, nullptr, d_walk, d_len, st)
                            : wg_zmpdisc_end_dev(&zm, B, d_sel + (size_t)c * B, lcap, d_zx, d_zy, nullptr, nullptr, d_left, d_lty, d_right,
                                                 nullptr, d_walk, d_len, st)) return rc;
        return grow_and_walk();
      };
      CHECK_HIP(hipMemsetAsync(d_done, 0, sizeof(int) * B, st));
      if (audit) CHECK_HIP(hipMemsetAsync(d_adone, 0, sizeof(int) * B, st));
      if (follow) {
        CHECK_HIP(hipMemsetAsync(d_clock, 0, sizeof(double) * B, st));
        CHECK_HIP(hipMemsetAsync(d_ticks, 0, sizeof(int) * B, st));
        CHECK_HIP(hipMemsetAsync(d_ran, 0, sizeof(int) * B, st));       // ORed by the follow calls, never cleared
      }
      CHECK_HIP(hipStreamSynchronize(st));
      const auto t0 = std::chrono::steady_clock::now();
      // --plan: the support foot and the arc become the steps the begin call takes
      if (on_device) CHECK_WG(plan_steps(cp.ccap, d_cmds, d_ncmds, S, d_steps, d_ns, st));
      CHECK_WG(robots ? wg_zmpdisc_begin_fleet_dev(&zfl, B, S, d_steps, on_device ? d_ns : d_two, d_feet, lcap, d_zx, d_zy, nullptr, nullptr,
                                                   d_left, d_lty, d_right, nullptr, d_walk, d_len, st)
                      : wg_zmpdisc_begin_dev(&zm, B, S, d_steps, on_device ? d_ns : d_two, d_feet, lcap, d_zx, d_zy, nullptr, nullptr, d_left,
                                             d_lty, d_right, nullptr, d_walk, d_len, st));
      for (int g = 0; g < B; ++g) cur[g] = len_after[g];
      if (follow) max_ticks = rounds[0];
      CHECK_WG(grow_and_walk());
      CHECK_WG(end_those_out_of_steps(0));
      for (int c = 0; c < n_calls; ++c) {
        const size_t at = on_device ? 0 : (size_t)c * B;       // --plan: call c's steps are planned into the one chunk
        if (on_device) CHECK_WG(plan_steps(online, d_later + (size_t)c * B * online, d_nlater + (size_t)c * B, online, d_chunks, d_cns, st));
        CHECK_WG(robots ? wg_zmpdisc_append_fleet_dev(&zfl, B, online, d_chunks + at * online, d_cns + at, lcap, d_zx, d_zy, nullptr, nullptr,
                                                      d_left, d_lty, d_right, nullptr, d_walk, d_len, st)
                        : wg_zmpdisc_append_dev(&zm, B, online, d_chunks + at * online, d_cns + at, lcap, d_zx, d_zy, nullptr, nullptr,
                                                d_left, d_lty, d_right, nullptr, d_walk, d_len, st));
        for (int g = 0; g < B; ++g)
          if (!ended[g]) cur[g] = len_after[(size_t)(c + 1) * B + g];
        if (follow) max_ticks = rounds[c + 1];
        CHECK_WG(grow_and_walk());
        CHECK_WG(end_those_out_of_steps(c + 1));
      }
      CHECK_HIP(hipStreamSynchronize(st));
      sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (follow) {
        std::vector<int> ticks_h(B);
        CHECK_HIP(hipMemcpy(ticks_h.data(), d_ticks, sizeof(int) * B, hipMemcpyDeviceToHost));
        for (int g = 0; g < B; ++g)
          if (ticks_h[g] != K) { fprintf(stderr, "FAILED: gait %d walked %d ticks of %d\n", g, ticks_h[g], K); return 1; }
      } else if (ticks != K) { fprintf(stderr, "FAILED: walked %d ticks of %d\n", ticks, K); return 1; }
      sec_walk = 0.0;
      for (size_t i = 0; i + 1 < ev.size(); i += 2) { float ms = 0.f; CHECK_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); sec_walk += ms * 1e-3; }
      std::vector<int> len_h(B);
      CHECK_HIP(hipMemcpy(len_h.data(), d_len, sizeof(int) * B, hipMemcpyDeviceToHost));
      for (int g = 0; g < B; ++g)                              // every gait must have arrived at the whole sequence's length
        if (len_h[g] != len_ended[g] || !ended[g]) { fprintf(stderr, "FAILED: gait %d ended with length %d, not %d\n", g, len_h[g], len_ended[g]); return 1; }
      continue;
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (on_device) CHECK_WG(plan_steps(cp.ccap, d_cmds, d_ncmds, S, d_steps, d_ns, st));
    CHECK_WG(zd_full(st));
    CHECK_WG(fc_batch(st));
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t1 = std::chrono::steady_clock::now();
    CHECK_WG(walk(0.0, K, st));
    CHECK_HIP(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();
    sec = std::chrono::duration<double>(t2 - t0).count();
    sec_walk = std::chrono::duration<double>(t2 - t1).count();
  }
  std::vector<int> count(B), ran(B);
  CHECK_HIP(hipMemcpy(states.data(), d_states, sizeof(wg_dimitrov_state_t) * B, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(count.data(), d_count, sizeof(int) * B, hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(ran.data(), d_ran, sizeof(int) * B, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < ran_pieces.size(); ++i) ran[i % B] |= ran_pieces[i];
  int n_ran = 0, max_count = 0;
  for (int g = 0; g < B; ++g) {
    if (count[g] < 1 || count[g] > qcap) { fprintf(stderr, "FAILED: gait %d: %d polytopes (capacity %d)\n", g, count[g], qcap); return 1; }
    n_ran += ran[g];
    max_count = count[g] > max_count ? count[g] : max_count;
  }
  if (heights) {
    std::vector<int> status(B);
    CHECK_HIP(hipMemcpy(status.data(), d_status, sizeof(int) * B, hipMemcpyDeviceToHost));
    for (int g = 0; g < B; ++g)
      if (status[g] != WG_OK) { fprintf(stderr, "FAILED: model %d (height %.4f): status %d\n", g, h_of[g], status[g]); return 1; }
    // gaits 0 and B - 1 once more, each alone: the default context configured with the gait's own model, one walk over its final queue
    // --robots: the gait's queue is made once more as well, through the one-model producers with the gait's own model and sole
    wg_dimitrov_state_t *d_one;
    CHECK_HIP(dev_alloc(&d_one, 1));
    wg_rel_step_t *d_s1 = nullptr; int *d_n1 = nullptr, *d_len1 = nullptr, *d_lty1 = nullptr, *d_count1 = nullptr;
    double *d_left1 = nullptr, *d_right1 = nullptr, *d_ts1 = nullptr, *d_te1 = nullptr; wg_zmp_polytope_t *d_q1 = nullptr;
    if (robots) {
      CHECK_HIP(dev_alloc(&d_s1, S)); CHECK_HIP(dev_alloc(&d_n1, 1)); CHECK_HIP(dev_alloc(&d_len1, 1)); CHECK_HIP(dev_alloc(&d_count1, 1));
      CHECK_HIP(dev_alloc(&d_lty1, lcap)); CHECK_HIP(dev_alloc(&d_left1, 6 * (size_t)lcap)); CHECK_HIP(dev_alloc(&d_right1, 6 * (size_t)lcap));
      CHECK_HIP(dev_alloc(&d_ts1, qcap)); CHECK_HIP(dev_alloc(&d_te1, qcap)); CHECK_HIP(dev_alloc(&d_q1, qcap));
    }
    for (int g : {0, B - 1}) {
      wg_dimitrov_model_t own = dm;
      own.com_height = h_of[g];
      CHECK_WG(wg_dimitrov_configure(&own));
      const wg_zmp_polytope_t *q_g = d_queues + (size_t)g * qcap;
      const double *ts_g = d_ts + (size_t)g * qcap, *te_g = d_te + (size_t)g * qcap;
      const int *count_g = d_count + g;
      if (robots) {
        std::vector<wg_rel_step_t> own_steps(&steps[(size_t)g * S], &steps[(size_t)g * S] + S);
        int n_own = n_steps[g];
        if (planned) {                                          // --plan keeps only the times of a gait's steps on the host: plan them here
          wg_step_stack_t stack = {1, 0, 0, 0};
          CHECK_WG(wg_steps_plan(&cp.whole[(size_t)g * S], cp.n_whole[g], zms[g].t_single, zms[g].t_double, &stack, S, own_steps.data(), &n_own));
          if (stack.error || n_own != n_steps[g]) { fprintf(stderr, "FAILED: gait %d: its command list gives %d steps (%d)\n", g, n_own, stack.error); return 1; }
        }
        CHECK_HIP(hipMemcpy(d_s1, own_steps.data(), sizeof(wg_rel_step_t) * S, hipMemcpyHostToDevice));
        CHECK_HIP(hipMemcpy(d_n1, &n_own, sizeof(int), hipMemcpyHostToDevice));
        CHECK_WG(wg_zmpdisc_full_batch_dev(&zms[g], 1, S, d_s1, d_n1, d_feet + (size_t)g * 6, lcap, nullptr, nullptr, nullptr, nullptr, d_left1, d_lty1,
                                           d_right1, nullptr, d_len1, st));
        CHECK_WG(wg_foot_constraints_batch_dev(1, lcap, d_len1, d_time, d_left1, d_lty1, d_right1, soles[g].sole_w, soles[g].sole_h,
                                               soles[g].constraint_x, soles[g].constraint_y, qcap, d_q1, d_ts1, d_te1, d_count1, st));
        q_g = d_q1; ts_g = d_ts1; te_g = d_te1; count_g = d_count1;
      }
      wg_dimitrov_state_t one;
      memset(&one, 0, sizeof one);
      one.starting = 1;
      CHECK_HIP(hipMemcpy(d_one, &one, sizeof one, hipMemcpyHostToDevice));
      CHECK_WG(wg_dimitrov_walk_dev(1, qcap, q_g, ts_g, te_g, count_g, 0.0, K, d_one, nullptr, nullptr, 0, st));
      CHECK_HIP(hipStreamSynchronize(st));
      CHECK_HIP(hipMemcpy(&one, d_one, sizeof one, hipMemcpyDeviceToHost));
      if (memcmp(&one, &states[g], sizeof one)) { fprintf(stderr, "FAILED: gait %d differs from a context configured with its own model\n", g); return 1; }
    }
    if (robots)
      printf("dimitrov_fleet: robots of size %.4f .. %.4f, a walk model, support times and a sole per gait; gaits 0 and %d == the one-model "
             "producers with their own model and sole\n", r_lo, r_hi, B - 1);
    printf("dimitrov_fleet: CoM heights %.4f .. %.4f m, the constants of %d models made on the device, all status 0; gaits 0 and %d == a "
           "context configured with their own model\n", h_lo, h_hi, B, B - 1);
  }
  if (audit) {                                                 // the folded verdicts are those of one call over the finished walks
    std::vector<int> len_h(B);
    CHECK_HIP(hipMemcpy(len_h.data(), d_len, sizeof(int) * B, hipMemcpyDeviceToHost));
    wg_fleet::FleetAudit whole;
    CHECK_HIP(dev_alloc(&whole.d_audit, B));
    CHECK_WG(wg_zmp_audit_dev(B, lcap, d_len, d_time, d_zx, d_zy, B, qcap, d_queues, d_ts, d_te, d_count, whole.d_audit, nullptr, st));
    CHECK_HIP(hipStreamSynchronize(st));
    if (wg_fleet::audit_report("dimitrov_fleet", "the ZMP reference, folded call by call behind the growing queues", &fa, B, lcap, len_h.data(),
                               time.data(), d_zx, d_zy, B, qcap, d_queues, d_ts, d_te, d_count)) return 1;
    whole.audit.resize(B);
    CHECK_HIP(hipMemcpy(whole.audit.data(), whole.d_audit, sizeof(wg_zmp_audit_t) * B, hipMemcpyDeviceToHost));
    if (memcmp(whole.audit.data(), fa.audit.data(), sizeof(wg_zmp_audit_t) * B)) { fprintf(stderr, "FAILED: the folded audits differ from one audit of the finished walks\n"); return 1; }
    printf("dimitrov_fleet: the audits folded on line == one wg_zmp_audit_dev over the finished walks, %d gaits by bytes\n", B);
  }
  const uint64_t h = wg_fleet::fnv1a64(states.data(), sizeof(wg_dimitrov_state_t) * B);
  double far = 0.0;
  for (int g = 0; g < B; ++g) far = states[g].xk[0] > far ? states[g].xk[0] : far;
  printf("dimitrov_fleet: %d walks (<= %d steps, <= %d samples, <= %d polytopes) x %d ticks in %.2f ms = %.0f walks/s; the walk alone "
         "%.2f ms = %.0f ticks/s; %d gaits ran out of their queue; farthest CoM %.3f m; checksum %016llx\n", B, S, lcap, max_count, K,
         sec * 1e3, B / sec, sec_walk * 1e3, (double)B * K / sec_walk, n_ran, far, (unsigned long long)h);
  wg_shutdown();
  return 0;
}
