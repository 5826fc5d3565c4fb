// phnn_lbfgs.h -- the batched L-BFGS slot kernel (phnn_lbfgs.hip) as the host side (phnn_mpc.hip) sees it.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

// Per-problem scalars of one torch.optim.LBFGS instance (torch/optim/lbfgs.py, step()).  48 bytes, zeroed by the
// state reset of phnn_solve_lbfgs (n_iter = 0: the next iteration is the first one ever).
struct LbfgsState {
  int32_t n_iter;      // state['n_iter'], over the whole solve
  int32_t func_evals;  // state['func_evals']
  int32_t it;          // n_iter of the current step() call
  int32_t evals;       // current_evals of the current step() call
  int32_t status;      // 1: moved, waiting on the evaluation of the next slot; 0: idle until the next step()
  int32_t count;       // history pairs held (len(old_dirs))
  int32_t head;        // ring position the next pair is written to
  int32_t pad;
  float t;             // step length of the last iteration
  float hdiag;         // H_diag
  double prev_loss;    // prev_loss (a Python float)
};

struct LbfgsParams {
  float* u;                 // (B, N) iterates, updated in place
  const float* cost;        // (B) K1 cost of this slot's evaluation
  const float* grad;        // (B, N) K2 gradient of this slot's evaluation
  float* costs_out;         // (B) row of the orig_loss history (slot 0 only), or NULL
  int32_t* n_iter_out;      // (B) or NULL
  int32_t* func_evals_out;  // (B) or NULL
  LbfgsState* st;           // (B)
  float* ro;                // (B, hs) ring of 1 / ys
  float* al;                // (B, hs) two-loop scratch
  float* d;                 // (B, Np) direction
  float* pg;                // (B, Np) prev_flat_grad
  float* hist;              // (B, hs, 2, Np) ring of (s, y) pairs
  long long B;
  int N;   // H * m
  int Np;  // N rounded up to a multiple of 4 (16-byte rows)
  int hs;  // history_size
  int max_iter, max_eval, slot;
  float lr, tol_grad, tol_change, ys_min;  // float32 thresholds (a float32 tensor compared with a Python scalar)
  double tol_change_d;                     // |loss - prev_loss| < tolerance_change is taken in double
};

// Largest H * m the slot kernel holds in registers (16 lanes x 4 float4 per problem).
constexpr int kLbfgsMaxN = 256;

// Byte layout of the caller-owned L-BFGS workspace; every region 256-byte aligned.
struct LbfgsLayout {
  size_t st, ro, al, d, pg, hist, total;
};
LbfgsLayout lbfgs_layout(long long B, int N, int hs);

// Enqueues one k_lbfgs launch on `st` (B > 0, N <= kLbfgsMaxN).
hipError_t lbfgs_launch(const LbfgsParams& p, hipStream_t st);
