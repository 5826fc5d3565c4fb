// phnn_ukf.h -- the two kernels of the batched unscented Kalman filter (phnn_ukf_sigma, phnn_ukf_moments,
// phnn_ukf_step) as the host side (phnn_mpc.hip) sees them: the sigma points of (xhat, P) with their control rows, and
// the weighted mean and covariance of their images.  Between the two runs K1 with H = 1 on the B * S sigma points, after
// them k_ekf_update (phnn_ekf.hip) with the identity as its Jacobian.  Kernels in phnn_ukf.hip.  DESIGN.md section 24;
// tests/ukf_model.py states the operation order of both kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

struct UkfSigmaParams {
  const float* xhat;  // (B,N)
  const double* P;    // (B,N,N): only the lower triangle is read
  const float* u;     // problem b's applied control: u + b * u_stride, m floats; read only when ctrl is given
  long long u_stride;
  float* chi;         // (B,S,N), S = 2 N + 1: xhat, xhat + gamma L[:,c], xhat - gamma L[:,c]; all NaN on a failure
  float* ctrl;        // (B,S,1,m) or NULL: the control of problem b for each of its sigma points
  long long B;
  int m;
  double gamma;       // sqrt(n + lambda)
};

struct UkfMomentsParams {
  const float* Y;     // image k of problem b: Y + (b * S + k) * Y_stride, N floats
  long long Y_stride;
  float* xm;          // (B,N): the weighted mean, rounded once
  double* Pm;         // (B,N,N): the weighted covariance about the float64 mean, symmetric
  float* eye;         // (B,N,N) or NULL: the identity k_ekf_update takes as its Jacobian
  long long B;
  double wm0, wc0, wi;
};

// hipErrorInvalidValue: no kernel for n
hipError_t ukf_sigma_launch(int n, const UkfSigmaParams& p, hipStream_t st);
hipError_t ukf_moments_launch(int n, const UkfMomentsParams& p, hipStream_t st);
