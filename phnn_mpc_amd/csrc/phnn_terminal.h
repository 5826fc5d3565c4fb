// phnn_terminal.h -- the two kernels of the terminal cost as the host side (phnn_mpc.hip) sees
// them: k_terminal_cost adds e_H^T W e_H to the cost K1 wrote (and writes row H of the cotangent K2 reads), k_dare
// iterates the Riccati step of phnn_tvlqr on one (A, B) to the infinite-horizon cost-to-go and hands back the terminal
// weight W.  Kernels in phnn_terminal.hip; tests/terminal_model.py states the operation order of both.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

struct TerminalCostParams {
  const float* traj;  // (B,H+1,N): row H is read
  float* cost;        // (B): cost[b] = cost[b] + c
  float* traj_bar;    // (B,H+1,N) or NULL: row H is written, the rows before it are never touched
  const float* W;     // row b uses W + (b / group) * w_bs, (N,N) row-major
  long long w_bs;
  int group;
  long long B;
  int H;
  float x_target[4];
  // reference tracking (phnn_reference): r = x_ref + b * ref_bs + min(off + H, ref_rows - 1) * ref_ts, or x_target
  const float* x_ref;
  long long ref_bs, ref_ts;
  int ref_rows;
  const int* ref_off_dev;
  int ref_off_host;
};

struct DareParams {
  const float* A;   // (B,N,N)
  const float* Bm;  // (B,N,MI)
  double* P;        // (B,N,N)
  double* K;        // (B,MI,N)
  float* W;         // (B,N,N): (float)(0.5 (P - Lxx))
  int* iters;       // (B): Riccati steps taken
  int* status;      // (B): 0 converged, 1 failure (outputs quiet NaN), 2 max_iters reached (outputs: the last iterate)
  long long B;
  int max_iters;
  double tol, mu;
  double Lxx[16], Luu[16];  // Q + Q^T (N x N), R + R^T (MI x MI), row-major, formed on the host in float64
};

// hipErrorInvalidValue: no kernel for n / (n, m)
hipError_t terminal_cost_launch(int n, const TerminalCostParams& p, hipStream_t st);
hipError_t dare_launch(int n, int m, const DareParams& p, hipStream_t st);
