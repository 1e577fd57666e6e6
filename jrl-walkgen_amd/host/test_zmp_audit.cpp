// test_zmp_audit -- the walk audit's host twin (wg_zmp_audit: csrc/wg_audit.cpp) alone: no device, no Python.  Built with the
// host files only, so it can run under -fsanitize=address,undefined:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//         -o bin/test_zmp_audit host/test_zmp_audit.cpp csrc/wg_audit.cpp csrc/wg_footcons.cpp
// A feet trajectory of five support phases goes through wg_foot_constraints; a ZMP track that wanders in and out of the
// polygons is audited against that queue, in heap arrays of exactly the sizes the call is promised (inputs) and between canaries
// (outputs): the twin is a serial restatement written here (linear first-match search), bit for bit; one call over [0, n) is the
// calls over pieces cut at 1, CH - 1, CH, CH + 1 and 2 CH; stride 2 reads an interleaved track; an empty queue, a queue cut by its
// capacity and non-finite samples are counted; refusals and argument errors leave the caller's bytes.  Exit status 0: all held.
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
const int CH = 64, N = 3 * CH + 5, CAP = 8;
const double INF = HUGE_VAL;

bool finite_(double v) { return std::fabs(v) <= 1.7976931348623157e308; }

// the rule of include/wg_mpc.h, serially, with the linear search for the first entry that holds the time
void restate(int n, const double *t, const double *x, const double *y, int stored, const wg_zmp_polytope_t *P, const double *ts,
             const double *te, wg_zmp_audit_t *A, double *margin) {
  *A = wg_zmp_audit_t{INF, -1, -1, 0, 0, 0, WG_OK};
  for (int k = 0; k < n; k++) {
    int q = -1;
    for (int e = 0; e < stored && q < 0; e++)
      if (ts[e] <= t[k] && t[k] <= te[e]) q = e;
    const bool nonfinite = !(finite_(x[k]) && finite_(y[k]));
    const bool uncovered = q < 0 || P[q].nrows < 1 || P[q].nrows > WG_POLY_MAX_ROWS;
    bool violated = nonfinite || uncovered;
    double m = -INF;
    int row = -1;
    if (!violated)
      for (int j = 0; j < P[q].nrows; j++) {
        const double v = (P[q].A[j][0] * x[k] + P[q].A[j][1] * y[k]) + P[q].B[j];
        double d = v / std::sqrt(P[q].A[j][0] * P[q].A[j][0] + P[q].A[j][1] * P[q].A[j][1]);
        if (!finite_(d)) d = -INF;
        if (j == 0 || d < m) { m = d; row = j; }
        if (v < -1e-8) violated = true;
      }
    margin[k] = m;
    if (m < A->margin) { A->margin = m; A->worst_sample = k; A->worst_row = row; }
    A->n_violated += violated; A->n_uncovered += uncovered; A->n_nonfinite += nonfinite;
  }
}

struct Out {                                     // a wg_zmp_audit_t between two of a pattern, margins between canaries
  std::vector<wg_zmp_audit_t> a;
  std::vector<double> m;
  explicit Out(int n) : a(3), m((size_t)n + 2, CANARY) { memset(a.data(), 0xA5, 3 * sizeof(wg_zmp_audit_t)); }
  wg_zmp_audit_t *audit() { return &a[1]; }
  double *margin() { return m.data() + 1; }
  bool canaries_hold() const {
    std::vector<unsigned char> pat(sizeof(wg_zmp_audit_t), 0xA5);
    return !memcmp(&a[0], pat.data(), pat.size()) && !memcmp(&a[2], pat.data(), pat.size()) && m.front() == CANARY && m.back() == CANARY;
  }
  bool untouched() const {
    std::vector<unsigned char> pat(sizeof(wg_zmp_audit_t), 0xA5);
    for (double v : m)
      if (v != CANARY) return false;
    return !memcmp(&a[1], pat.data(), pat.size());
  }
};

}  // namespace

int main() {
  // feet of five phases: aligned double support, a sole at +10 degrees, two crossed soles (8 corners on the hull), a sole at -10
  // degrees, a staggered aligned double support
  std::vector<double> time(N), left(6 * (size_t)N, 0.0), right(6 * (size_t)N, 0.0);
  std::vector<int> lt(N);
  const double T = 0.005;
  double tt = 0.0;
  for (int i = 0; i < N; i++) {
    time[i] = tt;
    tt += T;
    const int ph = i / 40 < 4 ? i / 40 : 4;
    double *L = &left[6 * (size_t)i], *R = &right[6 * (size_t)i];
    const double Ls[5][4] = {{0.0, 0.095, 0.0, 0.0}, {0.0, 0.095, 0.0, 10.0}, {0.1, 0.0, 0.0, 10.0}, {0.3, 0.095, 0.03, 0.0}, {0.35, 0.095, 0.0, 0.0}};
    const double Rs[5][4] = {{0.0, -0.095, 0.0, 0.0}, {0.1, -0.095, 0.03, 0.0}, {0.1, 0.0, 0.0, 100.0}, {0.2, -0.095, 0.0, -10.0}, {0.2, -0.095, 0.0, 0.0}};
    const int types[5] = {11, 1, 11, -1, 11};
    memcpy(L, Ls[ph], sizeof Ls[ph]);
    memcpy(R, Rs[ph], sizeof Rs[ph]);
    lt[i] = types[ph];
  }
  std::vector<wg_zmp_polytope_t> P(CAP);
  std::vector<double> ts(CAP, CANARY), te(CAP, CANARY);
  const int count = wg_foot_constraints(N, time.data(), left.data(), lt.data(), right.data(), 0.24, 0.138, 0.02, 0.02, CAP, P.data(), ts.data(), te.data());
  CHECK(count == 5, "wg_foot_constraints: %d polytopes", count);
  if (count != 5) return 1;
  CHECK(P[0].nrows == 4 && P[2].nrows == 8 && P[4].nrows == 6, "rows %d %d %d", P[0].nrows, P[2].nrows, P[4].nrows);

  Rng r{17};
  const double cx[5] = {0.0, 0.0, 0.1, 0.2, 0.275}, cy[5] = {0.0, 0.095, 0.0, -0.095, 0.0};
  std::vector<double> x(N), y(N), xy(2 * (size_t)N);
  for (int i = 0; i < N; i++) {
    const int ph = i / 40 < 4 ? i / 40 : 4;
    x[i] = cx[ph] + r.uni(-0.09, 0.09);
    y[i] = cy[ph] + r.uni(-0.09, 0.09);
  }
  x[CH] = NAN;
  y[100] = INF;
  for (int i = 0; i < N; i++) { xy[2 * (size_t)i] = x[i]; xy[2 * (size_t)i + 1] = y[i]; }

  // 1. the twin is the restatement, for the whole queue, a queue cut by its capacity, an empty one
  wg_zmp_audit_t want;
  std::vector<double> wm(N);
  Out whole(N);
  for (int variant = 0; variant < 3; variant++) {
    const int cnt = variant == 2 ? 0 : count, qcap = variant == 1 ? 2 : CAP;
    restate(N, time.data(), x.data(), y.data(), cnt < qcap ? cnt : qcap, P.data(), ts.data(), te.data(), &want, wm.data());
    Out o(N);
    const int rc = wg_zmp_audit(0, N, time.data(), x.data(), y.data(), 1, cnt, qcap, P.data(), ts.data(), te.data(), o.audit(), o.margin());
    CHECK(rc == WG_OK && o.canaries_hold(), "variant %d: rc %d", variant, rc);
    CHECK(!memcmp(o.audit(), &want, sizeof want), "variant %d: audit differs (margin %g vs %g, sample %d vs %d)", variant, o.audit()->margin, want.margin, o.audit()->worst_sample, want.worst_sample);
    CHECK(!memcmp(o.margin(), wm.data(), N * sizeof(double)), "variant %d: margins differ", variant);
    if (variant == 0) {
      CHECK(want.n_nonfinite == 2 && want.n_uncovered == 0 && want.n_violated > 10 && want.n_violated < N - 10 && want.margin == -INF && want.worst_sample == CH,
            "the track is not what the test is about");
      memcpy(whole.audit(), o.audit(), sizeof want);
      memcpy(whole.margin(), o.margin(), N * sizeof(double));
    }
    if (variant == 2) CHECK(want.n_uncovered == N && want.worst_sample == 0, "empty queue");
    // stride 2 reads the interleaved track
    Out s2(N);
    CHECK(wg_zmp_audit(0, N, time.data(), xy.data(), xy.data() + 1, 2, cnt, qcap, P.data(), ts.data(), te.data(), s2.audit(), s2.margin()) == WG_OK, "stride 2");
    CHECK(!memcmp(s2.audit(), o.audit(), sizeof want) && !memcmp(s2.margin(), o.margin(), N * sizeof(double)), "variant %d: stride 2 differs", variant);
    // no margins wanted
    Out nm(N);
    CHECK(wg_zmp_audit(0, N, time.data(), x.data(), y.data(), 1, cnt, qcap, P.data(), ts.data(), te.data(), nm.audit(), nullptr) == WG_OK, "no margins");
    CHECK(!memcmp(nm.audit(), o.audit(), sizeof want) && nm.canaries_hold(), "variant %d: without margins", variant);
  }

  // 2. cuts: inputs of exactly the length reached so far
  const int cuts[] = {1, CH - 1, CH, CH + 1, 2 * CH, N};
  Out pieces(N);
  int first = 0;
  for (int n : cuts) {
    std::vector<double> tn(time.begin(), time.begin() + n), xn(x.begin(), x.begin() + n), yn(y.begin(), y.begin() + n);
    const int rc = wg_zmp_audit(first, n, tn.data(), xn.data(), yn.data(), 1, count, CAP, P.data(), ts.data(), te.data(), pieces.audit(), pieces.margin());
    CHECK(rc == WG_OK, "cut at %d: rc %d", n, rc);
    restate(n, time.data(), x.data(), y.data(), count, P.data(), ts.data(), te.data(), &want, wm.data());
    CHECK(!memcmp(pieces.audit(), &want, sizeof want), "cut at %d: not the audit of the prefix", n);
    first = n;
  }
  CHECK(!memcmp(pieces.audit(), whole.audit(), sizeof want) && !memcmp(pieces.margin(), whole.margin(), N * sizeof(double)) && pieces.canaries_hold(),
        "the pieces are not the whole");
  CHECK(wg_zmp_audit(N, N, nullptr, nullptr, nullptr, 1, count, CAP, P.data(), ts.data(), te.data(), pieces.audit(), nullptr) == WG_OK &&
        !memcmp(pieces.audit(), whole.audit(), sizeof want), "a call that adds nothing");

  // 3. refusals keep the caller's bytes but the status; argument errors keep them all
  struct { int first, n, count; } refused[] = {{0, -1, count}, {0, N, -2}, {N + 1, N, count}, {1, N, count} /* the pattern's status is not WG_OK */};
  for (auto &c : refused) {
    Out o(N);
    const int rc = wg_zmp_audit(c.first, c.n, time.data(), x.data(), y.data(), 1, c.count, CAP, P.data(), ts.data(), te.data(), o.audit(), o.margin());
    CHECK(rc == WG_ERR_BAD_ARG && o.audit()->status == WG_ERR_BAD_ARG, "refusal (%d, %d, %d): rc %d", c.first, c.n, c.count, rc);
    o.audit()->status = (int)0xA5A5A5A5;
    CHECK(o.untouched(), "refusal (%d, %d, %d) wrote more than the status", c.first, c.n, c.count);
  }
  {
    Out o(N);
    const double *t = time.data(), *px = x.data(), *py = y.data(), *s = ts.data(), *e = te.data();
    const wg_zmp_polytope_t *p = P.data();
    CHECK(wg_zmp_audit(-1, N, t, px, py, 1, count, CAP, p, s, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "first_sample < 0");
    CHECK(wg_zmp_audit(0, N, nullptr, px, py, 1, count, CAP, p, s, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "null time");
    CHECK(wg_zmp_audit(0, N, t, nullptr, py, 1, count, CAP, p, s, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "null px");
    CHECK(wg_zmp_audit(0, N, t, px, nullptr, 1, count, CAP, p, s, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "null py");
    CHECK(wg_zmp_audit(0, N, t, px, py, 0, count, CAP, p, s, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "stride 0");
    CHECK(wg_zmp_audit(0, N, t, px, py, 1, count, 0, p, s, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "qcap 0");
    CHECK(wg_zmp_audit(0, N, t, px, py, 1, count, CAP, nullptr, s, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "null polys");
    CHECK(wg_zmp_audit(0, N, t, px, py, 1, count, CAP, p, nullptr, e, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "null t_start");
    CHECK(wg_zmp_audit(0, N, t, px, py, 1, count, CAP, p, s, nullptr, o.audit(), o.margin()) == WG_ERR_BAD_ARG, "null t_end");
    CHECK(wg_zmp_audit(0, N, t, px, py, 1, count, CAP, p, s, e, nullptr, o.margin()) == WG_ERR_BAD_ARG, "null audit");
    CHECK(o.untouched(), "an argument error wrote something");
    CHECK(wg_zmp_audit(0, 0, nullptr, nullptr, nullptr, 1, count, CAP, p, s, e, o.audit(), nullptr) == WG_OK && o.audit()->margin == INF &&
          o.audit()->worst_sample == -1 && o.audit()->worst_row == -1 && o.audit()->status == WG_OK, "no sample: the empty audit");
  }
  printf("test_zmp_audit: %s (%d samples, %d entries)\n", failures ? "FAILED" : "ok", N, count);
  return failures ? 1 : 0;
}
