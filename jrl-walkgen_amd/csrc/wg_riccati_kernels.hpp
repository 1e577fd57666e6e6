// wg_riccati_kernels.hpp -- the preview-control gains of a fleet whose gaits differ in CoM height (wg_riccati_gains_batch_dev).
//
// One lane per model: lane b runs wg_riccati_gains(T, zc[b], Q, R, Nl, mode) from wg_riccati_math.hpp, the text the host call
// compiles, so K, F and the status are the host's bits.  The doubling loop leaves when its own iterate has converged: the lanes
// of a wave diverge there and meet again behind it.  The matrices are 3x3 / 4x4 with constant indices (registers); what a lane
// stores goes time-major -- entry i of gait b at i*B + b -- so that a wave's stores are whole 512-byte rows and the F the preview
// kernels read (wg_preview_device.hpp, FLEET) is the array this kernel leaves.
#pragma once
#include <hip/hip_runtime.h>

#include "wg_riccati_math.hpp"

namespace wg {

// zc [B];  K_tm [4][B];  F_tm [Nl][B] (not read or written when Nl == 0);  status [B]
// A gait whose solve fails (a height that is not finite, no convergence) gets the host's code and zeros in its columns.
__global__ void __launch_bounds__(64)
wg_riccati_gains_kernel(int B, double T, const double *__restrict__ zc, double Q, double R, int Nl, int mode,
                        double *__restrict__ K_tm, double *__restrict__ F_tm, int *__restrict__ status) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const size_t sB = (size_t)B;
  double *K = K_tm + b, *F = Nl > 0 ? F_tm + b : nullptr;
  const int rc = rc_gains(T, zc[b], Q, R, Nl, mode, K, sB, F, sB);
  if (rc != WG_OK) {
    for (int i = 0; i < 4; ++i) K[(size_t)i * sB] = 0.0;
    for (int i = 0; i < Nl; ++i) F[(size_t)i * sB] = 0.0;
  }
  status[b] = rc;
}

}  // namespace wg
