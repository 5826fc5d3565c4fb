// phnn_ekf.h -- the two kernels of the batched extended Kalman filter (phnn_ekf_update, phnn_ekf_step) as the host side
// (phnn_mpc.hip) sees them: the covariance propagation with the measurement update, and the copy of the applied
// control into the one-step control row K1 reads.  Kernels in phnn_ekf.hip.  DESIGN.md section 20; tests/ekf_model.py
// states the operation order of the update.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

struct EkfUpdateParams {
  const float* xpred;      // problem b's predicted state: xpred + b * xpred_stride, N floats
  long long xpred_stride;
  const float* A;          // (B,N,N): d x+ / d x of the prediction step
  const float* y;          // problem b's measurement row: y + b * y_stride; only the measured components are read
  long long y_stride;
  double* P;               // (B,N,N) in/out
  float* xhat;             // (B,N)
  double* nis;             // (B) or NULL
  double* innov;           // (B,N) or NULL: 0 at unmeasured components
  int* status;             // (B): 0 updated (or nothing measured), 1 dropped measurement, 2 failure (outputs NaN)
  float* log_xhat;         // (T+1,B,N) or NULL: row step + 1
  double* log_nis;         // (T,B) or NULL: row step
  const int* step_dev;     // the step index of the log rows: *step_dev, else step_host
  int step_host;
  long long B;
  unsigned mask;           // bit i: component i is measured
  double Qn[16];           // (N,N) row-major
  double Rn[4];            // variances; read for measured components only
};

struct EkfControlsParams {
  const float* u;   // problem b's applied control: u + b * u_stride, m floats
  long long u_stride;
  float* row;       // (B,1,m)
  long long B;
  int m;
};

// hipErrorInvalidValue: no kernel for n
hipError_t ekf_update_launch(int n, const EkfUpdateParams& p, hipStream_t st);
hipError_t ekf_controls_launch(const EkfControlsParams& p, hipStream_t st);
