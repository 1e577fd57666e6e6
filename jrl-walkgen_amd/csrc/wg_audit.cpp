// wg_audit.cpp -- the walk audit of one gait on the host (host part of libwg_mpc.so): how far a ZMP track stays inside the
// polytopes of its gait's queue, the check ZMPConstrainedQPFastFormulation::ValidationConstraints makes of the previewed
// instants (ZMPConstrainedQPFastFormulation.cpp:248-381, switched off at :1403-1414) for every sample of the walk.  The
// arithmetic is wg_audit_math.hpp, shared with the kernels of wg_zmp_audit_dev / _append_dev: the same bytes.
//
// Plain host C++, sample after sample: the twin the fleet programs and the tests hold the kernels to.
#include "wg_audit_math.hpp"

extern "C" int wg_zmp_audit(int first_sample, int n, const double *time, const double *px, const double *py, int stride, int count,
                            int qcap, const wg_zmp_polytope_t *polys, const double *t_start, const double *t_end,
                            wg_zmp_audit_t *audit, double *margin) {
  if (!audit || first_sample < 0 || stride < 1 || qcap < 1 || !polys || !t_start || !t_end) return WG_ERR_BAD_ARG;
  if (n > first_sample && (!time || !px || !py)) return WG_ERR_BAD_ARG;
  // a refused gait: the verdicts of wg_zmp_audit_append_dev
  if (n < 0 || count < 0 || first_sample > n || (first_sample > 0 && audit->status != WG_OK)) {
    audit->status = WG_ERR_BAD_ARG;
    return WG_ERR_BAD_ARG;
  }
  wg_zmp_audit_t A = first_sample == 0 ? wg::au_empty() : *audit;
  const int K = count < qcap ? count : qcap;
  if (first_sample < n) {
    wg::AuCursor c;
    wg::au_place(t_start, t_end, K, wg::au_lower_bound(t_end, K, time[first_sample]), c);
    wg::AuRows R;
    R.nrows = 0;
    int loaded = -1;
    for (int k = first_sample; k < n; k++) {
      const bool covered = wg::au_seek(t_start, t_end, K, time[k], c);
      if (covered && c.q != loaded) {
        wg::au_load(polys + c.q, R);
        loaded = c.q;
      }
      const double m = wg::au_sample(R, covered, px[(size_t)k * stride], py[(size_t)k * stride], k, A);
      if (margin) margin[k] = m;
    }
  }
  A.status = WG_OK;
  *audit = A;
  return WG_OK;
}
