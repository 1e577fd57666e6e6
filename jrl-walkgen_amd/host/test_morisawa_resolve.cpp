// test_morisawa_resolve -- the host twins of the Morisawa re-plan (wg_morisawa_resolve, _resolve_fleet and their wg_morisawa_long_
// forms: csrc/wg_morisawa.cpp), alone: no device, no Python.  Built with the host twin file only, so it can run under
// -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//         -o bin/test_morisawa_resolve host/test_morisawa_resolve.cpp csrc/wg_morisawa.cpp
// Plans of S steps on one model and two CoM heights are solved in full and re-planned from two of their blocks, one per height,
// between canaries, in arrays of exactly the sizes the calls are promised: the re-planned blocks are the solved ones byte for byte,
// one-model and fleet form; a zeroed factor block, a factor_of outside the blocks, a height moved by one ulp and a NaN step
// leave block and neighbours alone.  Exit status 0: all of it held.
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

struct Rng {
  unsigned long long s;
  double uni(double lo, double hi) {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return lo + (hi - lo) * (double)(s >> 11) / 9007199254740992.0;
  }
};

const double CANARY = -7.25;

struct Plans {                                   // B plans of smax steps each (S of them used), one model, heights per gait
  int B, smax;
  wg_morisawa_model_t model;
  std::vector<wg_morisawa_model_t> models;
  std::vector<wg_rel_step_t> steps;
  std::vector<int> n_steps;
  std::vector<double> feet, com0;
  Plans(int B_, int smax_, int S, double h, unsigned long long seed) : B(B_), smax(smax_), models(B_), steps((size_t)B_ * smax_), n_steps(B_, S), feet(6 * (size_t)B_), com0(3 * (size_t)B_) {
    Rng r{seed};
    wg_morisawa_defaults(&model);
    for (int b = 0; b < B; b++) {
      double side = b % 2 == 0 ? -1.0 : 1.0;
      for (int i = 0; i < smax; i++) {
        wg_rel_step_t &s = steps[(size_t)b * smax + i];
        memset(&s, 0, sizeof s);
        s.sx = i == 0 ? 0.0 : r.uni(0.0, 0.25);
        s.sy = side * (i == 0 ? 0.105 : r.uni(0.17, 0.21));
        s.theta = i == 0 ? 0.0 : r.uni(-10.0, 10.0);
        side = -side;
      }
      const double f[6] = {r.uni(-0.05, 0.05), r.uni(0.08, 0.1), r.uni(-5, 5), r.uni(-0.05, 0.05), -r.uni(0.08, 0.1), r.uni(-5, 5)};
      memcpy(&feet[6 * (size_t)b], f, sizeof f);
      com0[3 * (size_t)b] = r.uni(0.0, 0.04); com0[3 * (size_t)b + 1] = r.uni(-0.01, 0.01); com0[3 * (size_t)b + 2] = h;
      models[b] = model;
      models[b].step_height = r.uni(0.05, 0.1);
      models[b].omega = b % 2 ? 5.0 : 0.0;
    }
  }
};

struct Family {
  bool lng;
  size_t words(int smax) const { return (lng ? wg_morisawa_long_block_bytes : wg_morisawa_block_bytes)(smax) / 8; }
  int solve(bool fleet, const Plans &p, double *blocks, int *status) const {
    auto fn = lng ? (fleet ? wg_morisawa_long_solve_fleet : wg_morisawa_long_solve) : (fleet ? wg_morisawa_solve_fleet : wg_morisawa_solve);
    return fn(fleet ? p.models.data() : &p.model, p.B, p.smax, p.steps.data(), p.n_steps.data(), p.feet.data(), p.com0.data(), blocks, status);
  }
  int resolve(bool fleet, const Plans &p, const double *factors, int n_factors, const int *factor_of, double *blocks, int *status) const {
    auto fn = lng ? (fleet ? wg_morisawa_long_resolve_fleet : wg_morisawa_long_resolve) : (fleet ? wg_morisawa_resolve_fleet : wg_morisawa_resolve);
    return fn(fleet ? p.models.data() : &p.model, p.B, p.smax, factors, n_factors, factor_of, p.steps.data(), p.feet.data(), p.com0.data(), blocks, status);
  }
};

bool untouched(const double *blk, size_t words) {
  for (size_t e = 0; e < words; e++)
    if (blk[e] != CANARY) return false;
  return true;
}

void one_case(bool lng, int smax, int S, int B) {
  const Family fam{lng};
  const size_t words = fam.words(smax);
  const double heights[2] = {0.7116911, 0.62};
  for (int fleet = 0; fleet < 2; fleet++) {
    Plans p(B, smax, S, heights[0], 40 + smax);
    std::vector<int> factor_of(B);
    for (int b = 0; b < B; b++) { factor_of[b] = b % 3 == 1; p.com0[3 * (size_t)b + 2] = heights[factor_of[b]]; }
    std::vector<double> full((size_t)B * words), got((size_t)(B + 2) * words, CANARY), factors(2 * words);
    std::vector<int> st(B), st2(B + 2, -77);
    CHECK(fam.solve(fleet, p, full.data(), st.data()) == WG_OK, "solve");
    for (int b = 0; b < B; b++) CHECK(st[b] == WG_OK, "%s smax %d gait %d: solve status %d", lng ? "long" : "short", smax, b, st[b]);
    memcpy(factors.data(), &full[0], words * 8);                       // gait 0 is at height 0, gait 1 at height 1
    memcpy(factors.data() + words, &full[words], words * 8);
    CHECK(fam.resolve(fleet, p, factors.data(), 2, factor_of.data(), got.data() + words, st2.data() + 1) == WG_OK, "resolve");
    CHECK(untouched(got.data(), words) && untouched(&got[(size_t)(B + 1) * words], words) && st2[0] == -77 && st2[B + 1] == -77, "rims");
    for (int b = 0; b < B; b++)
      CHECK(st2[1 + b] == WG_OK && memcmp(&got[(size_t)(1 + b) * words], &full[(size_t)b * words], words * 8) == 0,
            "%s smax %d S %d gait %d%s: the re-planned block differs from the solved one (status %d)", lng ? "long" : "short", smax, S, b, fleet ? " (fleet)" : "", st2[1 + b]);
    // refusals: the gaits of factor 0 a zeroed factor, gait 1 a factor_of past the blocks, gait 2 below them, gait 4 a NaN step, gait 7 a
    // height one ulp up; gait 10 is left to be right
    std::vector<double> zeroed(factors);
    std::fill(zeroed.begin(), zeroed.begin() + words, 0.0);
    std::vector<int> fo(factor_of);
    fo[1] = 2; fo[2] = -1;
    p.com0[3 * 7 + 2] = nextafter(p.com0[3 * 7 + 2], 2.0);
    p.steps[(size_t)4 * smax + S - 1].theta = NAN;
    std::fill(got.begin(), got.end(), CANARY);
    std::fill(st2.begin(), st2.end(), -77);
    CHECK(fam.resolve(fleet, p, zeroed.data(), 2, fo.data(), got.data() + words, st2.data() + 1) == WG_OK, "resolve with refusals");
    for (int b = 0; b < B; b++) {
      const bool bad = b == 1 || b == 2 || b == 4 || b == 7 || factor_of[b] == 0;
      if (bad) CHECK(st2[1 + b] == WG_MORISAWA_BAD_INPUT && untouched(&got[(size_t)(1 + b) * words], words), "refused gait %d: status %d", b, st2[1 + b]);
      else CHECK(st2[1 + b] == WG_OK && memcmp(&got[(size_t)(1 + b) * words], &full[(size_t)b * words], words * 8) == 0, "gait %d next to refused ones", b);
    }
    // host-side errors touch nothing
    std::fill(st2.begin(), st2.end(), -77);
    CHECK(fam.resolve(fleet, p, nullptr, 2, fo.data(), got.data() + words, st2.data() + 1) == WG_ERR_BAD_ARG, "NULL factors");
    CHECK(fam.resolve(fleet, p, zeroed.data(), 0, fo.data(), got.data() + words, st2.data() + 1) == WG_ERR_BAD_ARG, "n_factors 0");
    CHECK(st2[1] == -77, "a host-side error wrote a status");
  }
}

}  // namespace

int main() {
  one_case(false, 2, 2, 11);
  one_case(false, 7, 5, 11);
  one_case(false, 14, 14, 11);
  one_case(true, 3, 3, 11);
  one_case(true, 15, 15, 11);
  one_case(true, 64, 64, 11);
  printf(failures ? "test_morisawa_resolve: %d FAILED\n" : "test_morisawa_resolve: ok\n", failures);
  return failures ? 1 : 0;
}
