// Kajita preview-control gains (host side of the C ABI, include/wg_mpc.h: wg_riccati_solve / wg_riccati_gains).
//
// Replaces OptimalControllerSolver::ComputeWeights (src/PreviewControl/OptimalControllerSolver.cpp:200-352) and the
// system set-up of PreviewControl::ComputeOptimalWeights (src/PreviewControl/PreviewControl.cpp:198-322).
//
// The arithmetic is wg_riccati_math.hpp, the one text this file and the fleet kernel (wg_riccati_gains_batch_dev, one lane per
// CoM height) compile: LAPACK is not part of this image and the system is 3x3 / 4x4, so P comes from the structure-preserving
// doubling algorithm there.  One model takes microseconds here; a fleet with a height per gait has its gains made on the device.
#include "wg_riccati_math.hpp"

extern "C" int wg_riccati_solve(int n, const double *A_rm, const double *b, const double *c, double Q, double R,
                                int Nl, int mode, double *K, double *F) {
  switch (n) {
    case 1: return wg::rc_solve_order<1>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    case 2: return wg::rc_solve_order<2>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    case 3: return wg::rc_solve_order<3>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    case 4: return wg::rc_solve_order<4>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    case 5: return wg::rc_solve_order<5>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    case 6: return wg::rc_solve_order<6>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    case 7: return wg::rc_solve_order<7>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    case 8: return wg::rc_solve_order<8>(A_rm, b, c, Q, R, Nl, mode, K, 1, F, 1);
    default: return WG_ERR_BAD_ARG;                        // 1 <= n <= wg::kRcMaxN
  }
}

extern "C" int wg_riccati_gains(double T, double zc, double Q, double R, int Nl, int mode, double *K, double *F) {
  return wg::rc_gains(T, zc, Q, R, Nl, mode, K, 1, F, 1);
}
