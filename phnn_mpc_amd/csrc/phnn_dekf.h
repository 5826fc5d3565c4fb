// phnn_dekf.h -- the three kernels of the disturbance-augmented extended Kalman filter (phnn_dekf_update,
// phnn_dekf_step, phnn_dist_compensate) as the host side (phnn_mpc.hip) sees them: the update of the augmented state
// z = (x, d), the control row c(u) + dhat of the prediction, and the compensation of a command by dhat.  Kernels in
// phnn_dekf.hip.  DESIGN.md section 23; tests/dekf_model.py states the operation order of the update.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

struct DekfUpdateParams {
  const float* xpred;      // problem b's predicted state: xpred + b * xpred_stride, N floats
  long long xpred_stride;
  const float* A;          // (B,N,N): d x+ / d x of the prediction step
  const float* Bm;         // (B,N,MD): d x+ / d d of the prediction step (no clamp mask)
  const float* y;          // problem b's measurement row: y + b * y_stride; only the measured components are read
  long long y_stride;
  double* Pz;              // (B,N+MD,N+MD) in/out
  float* xhat;             // (B,N)
  float* dhat;             // (B,MD) in/out: the predicted disturbance is the one held
  double* nis;             // (B) or NULL
  double* innov;           // (B,N) or NULL: 0 at unmeasured components
  int* status;             // (B): 0 updated (or nothing measured), 1 dropped measurement, 2 failure (outputs NaN)
  float* log_xhat;         // (T+1,B,N) or NULL: row step + 1
  float* log_dhat;         // (T+1,B,MD) or NULL: row step + 1
  double* log_nis;         // (T,B) or NULL: row step
  const int* step_dev;     // the step index of the log rows: *step_dev, else step_host
  int step_host;
  long long B;
  unsigned mask;           // bit i < N: state component i is measured
  double Qz[36];           // (N+MD,N+MD) row-major
  double Rn[4];            // variances; read for measured components only
};

struct DekfControlsParams {
  const float* u;   // problem b's applied command: u + b * u_stride, m floats
  long long u_stride;
  const float* dhat;  // (B,m)
  float* row;         // (B,1,m) = c(u) + dhat
  long long B;
  int m;
  int has_bounds;
  float u_min, u_max;
};

struct DistCompensateParams {
  const float* v;   // problem b's command: v + b * v_stride, m floats
  long long v_stride;
  const float* dhat;  // (B,m)
  float* u_cmd;       // (B,m) = c(c(v) - dhat), c(v) where dhat is not finite
  int* status;        // (B) or NULL: 1 where a component of dhat is not finite, else 0
  long long B;
  int m;
  int has_bounds;
  float u_min, u_max;
};

// is there a k_dekf_update<n, m>?
bool dekf_has_kernel(int n, int m);
// hipErrorInvalidValue: no kernel for (n, m)
hipError_t dekf_update_launch(int n, int m, const DekfUpdateParams& p, hipStream_t st);
hipError_t dekf_controls_launch(const DekfControlsParams& p, hipStream_t st);
hipError_t dist_compensate_launch(const DistCompensateParams& p, hipStream_t st);
