// ref_parts_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// C entry points over the reference's dependency-free classes, for oracle/_ref/libwalkgen_parts_ref.so (oracle/Makefile, target
// `ref`): ComputeConvexHull (src/Mathematics/ConvexHull.cpp) and Polynome3 / Polynome4 / Polynome5 (src/Mathematics/Polynome.cpp,
// PolynomeFoot.cpp).  This file is the project's own text: it constructs the reference's objects and calls their methods, and
// holds no arithmetic.  The reference's headers are found through -I at build time; nothing built from them is committed.
//
// Array shapes are those of the oracle's probes (oracle/wg_oracle.h), so a test can hand both the same buffers.
#include <cstddef>
#include <vector>

#include <Mathematics/ConvexHull.hh>
#include <Mathematics/PolynomeFoot.hh>

namespace ref = PatternGeneratorJRL;

namespace {
// Compute / ComputeDerivative / ComputeSecDerivative of one polynomial at nt times; d1 and d2 may be null
void evaluate(ref::Polynome &p, int nt, const double *t, double *val, double *d1, double *d2) {
  for (int k = 0; k < nt; k++) {
    val[k] = p.Compute(t[k]);
    if (d1) d1[k] = p.ComputeDerivative(t[k]);
    if (d2) d2[k] = p.ComputeSecDerivative(t[k]);
  }
}
double *at(double *a, std::size_t i) { return a ? a + i : nullptr; }
}  // namespace

extern "C" {

// DoComputeConvexHull on n_sets point sets of n_pts points, xy [n_sets][n_pts][2] (x = col, y = row) -> hull [n_sets][n_pts + 1][2]
// (zero past the count) and count [n_sets].  The caller keeps away sets that span fewer than two directions about their lowest
// point: the reference reads past the end of its candidate list there.  Returns the number of hulls that did not fit n_pts + 1.
int wgr_convex_hull(int n_sets, int n_pts, const double *xy, double *hull, int *count) {
  int overflow = 0;
  ref::ComputeConvexHull ch;
  for (int s = 0; s < n_sets; s++) {
    std::vector<ref::CH_Point> pts((std::size_t)n_pts), out;
    for (int i = 0; i < n_pts; i++) {
      pts[i].col = xy[2 * ((std::size_t)s * n_pts + i)];
      pts[i].row = xy[2 * ((std::size_t)s * n_pts + i) + 1];
    }
    ch.DoComputeConvexHull(pts, out);
    count[s] = (int)out.size();
    if ((int)out.size() > n_pts + 1) overflow++;
    for (int i = 0; i <= n_pts; i++) {
      const bool have = i < (int)out.size();
      hull[2 * ((std::size_t)s * (n_pts + 1) + i)] = have ? out[i].col : 0.0;
      hull[2 * ((std::size_t)s * (n_pts + 1) + i) + 1] = have ? out[i].row : 0.0;
    }
  }
  return overflow;
}

// the plain forms, as the feet queue sets them: Polynome<degree>(FT[i], FP[i]) (degree 4: FP is the middle position), Compute at
// t[i][0 .. nt) -> val [n][nt]; d1 / d2 (may be null) the two derivatives.  Returns 0, or -2 on an unknown degree.
int wgr_poly_plain(int degree, int n, const double *FT, const double *FP, int nt, const double *t, double *val, double *d1,
                   double *d2) {
  if (degree < 3 || degree > 5) return -2;
  for (int i = 0; i < n; i++) {
    const std::size_t o = (std::size_t)i * nt;
    if (degree == 3) {
      ref::Polynome3 p(FT[i], FP[i]);
      evaluate(p, nt, t + o, val + o, at(d1, o), at(d2, o));
    } else if (degree == 4) {
      ref::Polynome4 p(FT[i], FP[i]);
      evaluate(p, nt, t + o, val + o, at(d1, o), at(d2, o));
    } else {
      ref::Polynome5 p(FT[i], FP[i]);
      evaluate(p, nt, t + o, val + o, at(d1, o), at(d2, o));
    }
  }
  return 0;
}

// the forms of the tick: 3: Polynome3::SetParametersWithInitPosInitSpeed(FT, FP, p0, v0); 4: Polynome4::SetParameters(FT, MP = FP);
// 5: Polynome5::SetParameters(FT, FP, p0, v0, a0) -- each on an object constructed with (0, 0) first, as the reference's foot
// trajectory generator holds them -- then value and both derivatives at t[i][0 .. nt).  Returns 0, or -2 on an unknown degree.
int wgr_poly_init(int degree, int n, const double *FT, const double *FP, const double *p0, const double *v0, const double *a0,
                  int nt, const double *t, double *val, double *d1, double *d2) {
  if (degree < 3 || degree > 5) return -2;
  for (int i = 0; i < n; i++) {
    const std::size_t o = (std::size_t)i * nt;
    double ft = FT[i], fp = FP[i], ip = p0[i], iv = v0[i];
    if (degree == 3) {
      ref::Polynome3 p(0.0, 0.0);
      p.SetParametersWithInitPosInitSpeed(ft, fp, ip, iv);
      evaluate(p, nt, t + o, val + o, at(d1, o), at(d2, o));
    } else if (degree == 4) {
      ref::Polynome4 p(0.0, 0.0);
      p.SetParameters(ft, fp);
      evaluate(p, nt, t + o, val + o, at(d1, o), at(d2, o));
    } else {
      ref::Polynome5 p(0.0, 0.0);
      p.SetParameters(ft, fp, ip, iv, a0[i]);
      evaluate(p, nt, t + o, val + o, at(d1, o), at(d2, o));
    }
  }
  return 0;
}

}  // extern "C"
