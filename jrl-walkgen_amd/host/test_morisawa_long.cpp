// test_morisawa_long -- the host twins of the long Morisawa family (wg_morisawa_long_solve, _long_solve_fleet, _long_sample,
// _long_system, _long_block_unpack, _long_length: csrc/wg_morisawa.cpp), alone: no device, no Python.  Built with the host twin
// file only, so it can run under -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//         -o bin/test_morisawa_long host/test_morisawa_long.cpp csrc/wg_morisawa.cpp
// Walks of S = 2, 15 and 64 steps (and ragged fleets at smax = 2, 7, 14, 15, 64) are solved and sampled; at smax <= 14 every
// section of the block and every sample must equal the short twin's by value; at every size the stored y must come back from the
// stored w through the band alone (the dgbtrs order documented in include/wg_mpc.h) and the block and outputs must be whole
// between canaries; the refusals must leave block and outputs untouched.  Exit status 0: all of it held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/wg_mpc.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      failures++;                                \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                       \
      printf("\n");                              \
    }                                            \
  } while (0)

struct Rng {                                     // a small LCG: the same fleets everywhere
  unsigned long long s;
  double uni(double lo, double hi) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return lo + (hi - lo) * (double)(s >> 11) / 9007199254740992.0;
  }
  int below(int n) { return (int)uni(0.0, (double)n); }
};

struct Fleet {
  int B, smax;
  std::vector<wg_rel_step_t> steps;
  std::vector<int> n_steps;
  std::vector<double> feet, com0;
  std::vector<wg_morisawa_model_t> models;
  Fleet(int B_, int smax_, unsigned long long seed) : B(B_), smax(smax_), steps((size_t)B_ * smax_), n_steps(B_), feet(6 * (size_t)B_), com0(3 * (size_t)B_), models(B_) {
    Rng r{seed};
    static const int single[] = {100, 120, 140, 156, 160}, dbl[] = {4, 8, 12, 20};
    for (int b = 0; b < B; b++) {
      n_steps[b] = b == 0 ? smax : (b == 1 ? 2 : 2 + r.below(smax - 1));
      double side = b % 2 == 0 ? -1.0 : 1.0;
      for (int i = 0; i < smax; i++) {
        wg_rel_step_t &s = steps[(size_t)b * smax + i];
        memset(&s, 0, sizeof s);
        s.sx = i == 0 ? 0.0 : r.uni(0.0, 0.25);
        s.sy = side * (i == 0 ? 0.105 : r.uni(0.17, 0.21));
        s.theta = i == 0 ? 0.0 : r.uni(-10.0, 10.0);
        side = -side;
      }
      const double f[6] = {r.uni(-0.05, 0.05), r.uni(0.08, 0.1), b % 3 == 0 ? r.uni(-5, 5) : 0.0, r.uni(-0.05, 0.05), -r.uni(0.08, 0.1), b % 3 == 0 ? r.uni(-5, 5) : 0.0};
      memcpy(&feet[6 * (size_t)b], f, sizeof f);
      com0[3 * (size_t)b] = r.uni(0.0, 0.04); com0[3 * (size_t)b + 1] = r.uni(-0.01, 0.01); com0[3 * (size_t)b + 2] = r.uni(0.5, 1.0);
      wg_morisawa_defaults(&models[b]);
      models[b].t_single = single[r.below(5)] * models[b].T;
      models[b].t_double = dbl[r.below(4)] * models[b].T;
      models[b].step_height = r.uni(0.05, 0.1);
      models[b].omega = b % 2 ? 5.0 : 0.0;
    }
  }
};

const double CANARY = -7.25;

bool same_values(const double *a, const double *b, size_t n) {          // by value: +0 == -0
  for (size_t i = 0; i < n; i++)
    if (!(a[i] == b[i])) return false;
  return true;
}

struct Outs {
  int lcap, B;
  std::vector<double> zx, zy, com, left, right;
  std::vector<int> lt, rt, len;
  Outs(int lcap_, int B_) : lcap(lcap_), B(B_), zx((size_t)(lcap_ + 2) * B_, CANARY), zy(zx), com((size_t)(lcap_ + 2) * 4 * B_, CANARY), left((size_t)(lcap_ + 2) * 6 * B_, CANARY), right(left), lt((size_t)(lcap_ + 2) * B_, -77), rt(lt), len(B_ + 2, -77) {}
  // the arrays handed to the sampler start one row in: a row of canaries before and behind each
  bool rims_whole() const {
    bool ok = len[0] == -77 && len[B + 1] == -77;
    for (int b = 0; b < B; b++) {
      ok = ok && zx[b] == CANARY && zx[(size_t)(lcap + 1) * B + b] == CANARY && zy[b] == CANARY && zy[(size_t)(lcap + 1) * B + b] == CANARY;
      ok = ok && lt[b] == -77 && lt[(size_t)(lcap + 1) * B + b] == -77 && rt[b] == -77 && rt[(size_t)(lcap + 1) * B + b] == -77;
      for (int c = 0; c < 4; c++) ok = ok && com[(size_t)c * B + b] == CANARY && com[((size_t)(lcap + 1) * 4 + c) * B + b] == CANARY;
      for (int c = 0; c < 6; c++)
        ok = ok && left[(size_t)c * B + b] == CANARY && left[((size_t)(lcap + 1) * 6 + c) * B + b] == CANARY && right[(size_t)c * B + b] == CANARY &&
             right[((size_t)(lcap + 1) * 6 + c) * B + b] == CANARY;
    }
    return ok;
  }
};

int sample(bool lng, const Fleet &f, const std::vector<double> &blocks, size_t words, const std::vector<int> &status, double t0, double T, Outs &o) {
  auto fn = lng ? wg_morisawa_long_sample : wg_morisawa_sample;
  const size_t B = (size_t)f.B;
  return fn(f.B, f.smax, blocks.data() + words, status.data() + 1, t0, T, o.lcap, o.zx.data() + B, o.zy.data() + B, o.com.data() + 4 * B, o.left.data() + 6 * B,
            o.lt.data() + B, o.right.data() + 6 * B, o.rt.data() + B, o.len.data() + 1);
}

// the stored y from the stored w through the band alone, in dgbtrs's order
double band_solve_error(const wg_morisawa_view_t &v) {
  const int n = v.n;
  double worst = 0.0;
  for (int ax = 0; ax < 2; ax++) {
    std::vector<double> b(ax ? v.wy : v.wx, (ax ? v.wy : v.wx) + n);
    const double *y = ax ? v.yy : v.yx;
    auto lu = [&](int i, int c) { return v.lu[(size_t)i * v.lu_pitch + (c - i + 5)]; };
    for (int k = 0; k < n; k++) {
      const int p = v.piv[k];
      if (p < k || p > k + 5 || p >= n) return HUGE_VAL;
      const double t = b[k]; b[k] = b[p]; b[p] = t;
      for (int i = k + 1; i <= k + 5 && i < n; i++) b[i] = b[i] - lu(i, k) * b[k];
    }
    for (int c = n - 1; c >= 0; c--) {
      b[c] = b[c] / lu(c, c);
      for (int i = c - 1; i >= c - 9 && i >= 0; i--) b[i] = b[i] - lu(i, c) * b[c];
    }
    for (int i = 0; i < n; i++) worst = fmax(worst, fabs(b[i] - y[i]));
  }
  return worst;
}

void one_fleet(int smax, int B, unsigned long long seed) {
  Fleet f(B, smax, seed);
  const size_t words = wg_morisawa_long_block_bytes(smax) / 8;
  CHECK(words > 0 && words % 16 == 0, "smax %d: block of %zu words", smax, words);
  std::vector<double> blocks((size_t)(B + 2) * words, CANARY);
  std::vector<int> status(B + 2, -77);
  int rc = wg_morisawa_long_solve_fleet(f.models.data(), B, smax, f.steps.data(), f.n_steps.data(), f.feet.data(), f.com0.data(), blocks.data() + words, status.data() + 1);
  CHECK(rc == WG_OK, "smax %d: long solve %d", smax, rc);
  CHECK(status[0] == -77 && status[B + 1] == -77, "smax %d: status rims", smax);
  for (size_t e = 0; e < words; e++)
    if (blocks[e] != CANARY || blocks[(size_t)(B + 1) * words + e] != CANARY) { CHECK(false, "smax %d: block rims", smax); break; }
  const double T = f.models[0].T, t0 = 2.0 * 0.78;
  int lcap = 0;
  for (int b = 0; b < B; b++) {
    CHECK(status[1 + b] == WG_OK, "smax %d gait %d: status %d", smax, b, status[1 + b]);
    const int len = wg_morisawa_long_length(&f.models[b], f.n_steps[b], t0);
    CHECK(len > 100, "smax %d gait %d: length %d", smax, b, len);
    if (len > lcap) lcap = len;
    // the one-model call handed model b gives gait b's bytes
    std::vector<double> one((size_t)B * words, CANARY);
    std::vector<int> st1(B, -77);
    if (b < 3) {
      wg_morisawa_long_solve(&f.models[b], B, smax, f.steps.data(), f.n_steps.data(), f.feet.data(), f.com0.data(), one.data(), st1.data());
      CHECK(memcmp(&one[(size_t)b * words], &blocks[(size_t)(1 + b) * words], words * 8) == 0, "smax %d gait %d: fleet form differs from the one-model call", smax, b);
    }
    wg_morisawa_view_t v;
    rc = wg_morisawa_long_block_unpack(&blocks[(size_t)(1 + b) * words], smax, &v);
    CHECK(rc == WG_OK && v.lu_pitch == 16 && v.n == 4 * f.n_steps[b] + 8, "smax %d gait %d: unpack %d", smax, b, rc);
    if (rc != WG_OK) continue;
    double ymax = 0.0;
    for (int i = 0; i < v.n; i++) ymax = fmax(ymax, fmax(fabs(v.yx[i]), fabs(v.yy[i])));
    const double err = band_solve_error(v);
    CHECK(err <= 1e-9 * (1.0 + ymax), "smax %d gait %d: the band does not give y back: %g", smax, b, err);
  }
  lcap += 3;
  Outs lo(lcap, B);
  rc = sample(true, f, blocks, words, status, t0, T, lo);
  CHECK(rc == WG_OK && lo.rims_whole(), "smax %d: long sample %d, rims %d", smax, rc, (int)lo.rims_whole());
  for (int b = 0; b < B; b++) CHECK(lo.len[1 + b] == wg_morisawa_long_length(&f.models[b], f.n_steps[b], t0), "smax %d gait %d: length", smax, b);

  if (smax <= WG_MORISAWA_MAX_STEPS) {                        // the short twin: every section and every sample by value
    const size_t swords = wg_morisawa_block_bytes(smax) / 8;
    std::vector<double> sblocks((size_t)(B + 2) * swords, CANARY);
    std::vector<int> sstatus(B + 2, -77);
    rc = wg_morisawa_solve_fleet(f.models.data(), B, smax, f.steps.data(), f.n_steps.data(), f.feet.data(), f.com0.data(), sblocks.data() + swords, sstatus.data() + 1);
    CHECK(rc == WG_OK, "smax %d: short solve %d", smax, rc);
    for (int b = 0; b < B; b++) {
      wg_morisawa_view_t a, s;
      if (wg_morisawa_long_block_unpack(&blocks[(size_t)(1 + b) * words], smax, &a) != WG_OK || wg_morisawa_block_unpack(&sblocks[(size_t)(1 + b) * swords], smax, &s) != WG_OK) {
        CHECK(false, "smax %d gait %d: unpack", smax, b);
        continue;
      }
      const int I = a.n_int, n = a.n;
      bool ok = a.n_steps == s.n_steps && I == s.n_int && n == s.n && a.com_height == s.com_height && a.t_total == s.t_total;
      ok = ok && same_values(a.dT, s.dT, I) && same_values(a.omega, s.omega, I) && same_values(a.tref, s.tref, I);
      ok = ok && same_values(a.zmp_x, s.zmp_x, 5 * I) && same_values(a.cog_x, s.cog_x, 5 * I) && same_values(a.zmp_y, s.zmp_y, 5 * I) && same_values(a.cog_y, s.cog_y, 5 * I);
      ok = ok && same_values(a.Vx, s.Vx, I) && same_values(a.Wx, s.Wx, I) && same_values(a.Vy, s.Vy, I) && same_values(a.Wy, s.Wy, I);
      ok = ok && same_values(a.left, s.left, 36 * I) && same_values(a.right, s.right, 36 * I);
      ok = ok && memcmp(a.left_type, s.left_type, 4 * I) == 0 && memcmp(a.right_type, s.right_type, 4 * I) == 0;
      ok = ok && same_values(a.profile_x, s.profile_x, I) && same_values(a.profile_y, s.profile_y, I) && same_values(a.support, s.support, 3 * a.n_steps);
      ok = ok && same_values(a.wx, s.wx, n) && same_values(a.wy, s.wy, n) && same_values(a.yx, s.yx, n) && same_values(a.yy, s.yy, n);
      ok = ok && memcmp(a.piv, s.piv, 4 * n) == 0;
      CHECK(ok, "smax %d gait %d: the long block differs from the short one", smax, b);
    }
    Outs so(lcap, B);
    rc = sample(false, f, sblocks, swords, sstatus, t0, T, so);
    CHECK(rc == WG_OK, "smax %d: short sample %d", smax, rc);
    bool ok = lo.len == so.len && lo.lt == so.lt && lo.rt == so.rt;
    ok = ok && same_values(lo.zx.data(), so.zx.data(), lo.zx.size()) && same_values(lo.zy.data(), so.zy.data(), lo.zy.size());
    ok = ok && same_values(lo.com.data(), so.com.data(), lo.com.size()) && same_values(lo.left.data(), so.left.data(), lo.left.size()) &&
         same_values(lo.right.data(), so.right.data(), lo.right.size());
    CHECK(ok, "smax %d: the long samples differ from the short ones", smax);
  }
}

void refusals() {
  const int smax = 15, B = 6;
  Fleet f(B, smax, 99);
  const size_t words = wg_morisawa_long_block_bytes(smax) / 8;
  f.n_steps[0] = 1;
  f.n_steps[1] = smax + 1;
  f.models[2].t_double = 0.0;
  f.com0[3 * 3 + 2] = NAN;
  f.com0[3 * 4 + 2] = 0.01;                                   // omega dT > 40, far beyond WG_MORISAWA_WALK_ARG_MAX
  std::vector<double> blocks((size_t)(B + 2) * words, CANARY);
  std::vector<int> status(B + 2, -77);
  int rc = wg_morisawa_long_solve_fleet(f.models.data(), B, smax, f.steps.data(), f.n_steps.data(), f.feet.data(), f.com0.data(), blocks.data() + words, status.data() + 1);
  CHECK(rc == WG_OK, "refusals: solve %d", rc);
  for (int b = 0; b < 5; b++) {
    CHECK(status[1 + b] == WG_MORISAWA_BAD_INPUT, "refusals: gait %d status %d", b, status[1 + b]);
    bool whole = true;
    for (size_t e = 0; e < words; e++) whole = whole && blocks[(size_t)(1 + b) * words + e] == CANARY;
    CHECK(whole, "refusals: gait %d's block was written", b);
  }
  CHECK(status[6] == WG_OK, "refusals: the good gait %d", status[6]);
  Outs o(2000, B);
  rc = sample(true, f, blocks, words, status, 1.56, 0.005, o);
  CHECK(rc == WG_OK && o.rims_whole(), "refusals: sample %d", rc);
  for (int b = 0; b < 5; b++) {
    bool whole = o.len[1 + b] == WG_MORISAWA_BAD_INPUT;
    for (int k = 0; k < o.lcap + 2; k++) whole = whole && o.zx[(size_t)k * B + b] == CANARY && o.left[((size_t)k * 6 + 5) * B + b] == CANARY && o.lt[(size_t)k * B + b] == -77;
    CHECK(whole, "refusals: gait %d's outputs were written", b);
  }
  CHECK(o.len[6] == WG_MORISAWA_CAPACITY || o.len[6] > 0, "refusals: the good gait's length %d", o.len[6]);
  // blocks of the other family, of another smax, without statuses
  std::vector<int> none;
  Outs p(16, 1);
  std::vector<double> shortblk((size_t)3 * (wg_morisawa_block_bytes(14) / 8), 0.0);
  Fleet g(1, 14, 5);
  std::vector<int> st(3, 0);
  wg_morisawa_solve_fleet(g.models.data(), 1, 14, g.steps.data(), g.n_steps.data(), g.feet.data(), g.com0.data(), shortblk.data() + shortblk.size() / 3, st.data() + 1);
  std::vector<double> padded((size_t)3 * (wg_morisawa_long_block_bytes(14) / 8), 0.0);
  memcpy(padded.data() + padded.size() / 3, shortblk.data() + shortblk.size() / 3, wg_morisawa_long_block_bytes(14));
  rc = wg_morisawa_long_sample(1, 14, padded.data() + padded.size() / 3, nullptr, 1.56, 0.005, 16, p.zx.data() + 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, p.len.data() + 1);
  CHECK(rc == WG_OK && p.len[1] == WG_MORISAWA_BAD_INPUT && p.zx[1] == CANARY, "a short block passed the long sampler: %d %d", rc, p.len[1]);
  // host-side refusals
  CHECK(wg_morisawa_long_block_bytes(1) == 0 && wg_morisawa_long_block_bytes(65) == 0, "block bytes out of range");
  CHECK(wg_morisawa_long_length(&f.models[5], 65, 0.0) == WG_MORISAWA_BAD_INPUT && wg_morisawa_long_length(&f.models[5], 64, 0.0) > 0, "length's cap");
  CHECK(wg_morisawa_long_solve_fleet(f.models.data(), B, 65, f.steps.data(), f.n_steps.data(), f.feet.data(), f.com0.data(), blocks.data(), status.data()) == WG_ERR_BAD_ARG, "smax 65");
  CHECK(wg_morisawa_long_sample(1, 65, blocks.data(), nullptr, 0.0, 0.005, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == WG_ERR_BAD_ARG, "sample smax 65");
}

void system_band() {
  for (int S : {2, 15, 64}) {
    Fleet f(1, S, 7 + S);
    const int n = 4 * S + 8;
    std::vector<double> Zb((size_t)n * 16 + 16, CANARY), wx(n + 1, CANARY), wy(n + 1, CANARY);
    const int rc = wg_morisawa_long_system(&f.models[0], S, f.steps.data(), f.feet.data(), f.com0.data(), Zb.data(), wx.data(), wy.data());
    CHECK(rc == n, "system S = %d: %d", S, rc);
    CHECK(Zb[(size_t)n * 16] == CANARY && wx[n] == CANARY && wy[n] == CANARY, "system S = %d wrote past its arrays", S);
    int nz = 0;
    for (int i = 0; i < n; i++) {
      CHECK(Zb[(size_t)i * 16 + 15] == 0.0, "system S = %d row %d: word 15", S, i);
      for (int w = 10; w < 15; w++) CHECK(Zb[(size_t)i * 16 + w] == 0.0, "system S = %d row %d: Z beyond column i + 4", S, i);
      for (int w = 0; w < 15; w++) nz += Zb[(size_t)i * 16 + w] != 0.0;
    }
    CHECK(nz > 2 * n && nz <= 7 * n, "system S = %d: %d non-zeros", S, nz);
    if (S <= WG_MORISAWA_MAX_STEPS) {
      std::vector<double> Z((size_t)n * n), sx(n), sy(n);
      CHECK(wg_morisawa_system(&f.models[0], S, f.steps.data(), f.feet.data(), f.com0.data(), Z.data(), sx.data(), sy.data()) == n, "dense system");
      bool ok = same_values(sx.data(), wx.data(), n) && same_values(sy.data(), wy.data(), n);
      for (int i = 0; i < n; i++)
        for (int c = 0; c < n; c++) {
          const bool in = c >= i - 5 && c <= i + 9;
          ok = ok && (in ? Z[(size_t)i * n + c] == Zb[(size_t)i * 16 + c - i + 5] : Z[(size_t)i * n + c] == 0.0);
        }
      CHECK(ok, "system S = %d: the band differs from the dense Z", S);
    }
  }
}

}  // namespace

int main() {
  one_fleet(2, 5, 11);
  one_fleet(7, 12, 12);
  one_fleet(14, 12, 13);
  one_fleet(15, 6, 14);
  one_fleet(64, 4, 15);
  refusals();
  system_band();
  printf(failures ? "test_morisawa_long: %d FAILED\n" : "test_morisawa_long: ok\n", failures);
  return failures ? 1 : 0;
}
