// phnn_feedback.h -- the kernel of the tracking law between two solves (phnn_feedback_control) and the workspace of the
// plan that feeds it (phnn_feedback_plan) as the host side (phnn_mpc.hip) sees them.  Kernel in phnn_feedback.hip.
// DESIGN.md section 21; tests/feedback_model.py states the operation order of the control.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

struct FeedbackControlParams {
  const float* x;      // (B,N): the current measurement or estimate
  const float* u;      // (B,H,MI): the plan's controls
  const float* traj;   // (B,H+1,N): the plan's nominal states
  const double* K;     // (B,H,MI,N): the gains around the plan
  float* u_out;        // (B,MI)
  int* status;         // (B) or NULL: 0 feedback applied, 1 gains not finite, 2 deviation not finite (1, 2: open loop)
  double* dev;         // (B) or NULL: max_i |dx_i|, NaN for status 2
  int* log_status;     // (T,B) or NULL: row step
  double* log_dev;     // (T,B) or NULL: row step
  const int* step_dev; // the step index: *step_dev, else step_host; the plan row is step % solve_every
  int step_host;
  int solve_every;
  int H;
  long long B;
  float u_min, u_max;
  int has_u_bounds;
};

// Byte offsets of the caller-owned workspace of phnn_feedback_plan, every region 256-byte aligned.
struct FeedbackLayout {
  size_t A, Bm, cost, P0, total;
};
FeedbackLayout feedback_layout(long long B, int H, int n, int m);

// hipErrorInvalidValue: no kernel for (n, m)
hipError_t feedback_control_launch(int n, int m, const FeedbackControlParams& p, hipStream_t st);
