// phnn_gn.h -- the three kernels of the batched Gauss-Newton solve (phnn_solve_gn) as the host side (phnn_mpc.hip) sees
// them: the LQ direction, the line-search candidates and the selection.  Kernels in phnn_gn.hip.  DESIGN.md section 18;
// tests/gn_model.py states the operation order of all three.  The box-constrained direction of phnn_solve_gn_ex
// (PHNN_GN_BOX) is DESIGN.md section 19 and tests/gn_box_model.py.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

constexpr int kGnMaxLineSteps = 32;  // L: alpha_j = 2^-j, j < L

struct GnDirectionParams {
  const float* A;     // (B,H,N,N)
  const float* Bm;    // (B,H,N,MI)
  const float* traj;  // (B,H+1,N)
  const float* u;     // (B,H,MI)
  const double* mu;   // (B)
  float* du;          // (B,H,MI): the float64 step rounded once; zeros on failure
  double* dV;         // (B): sum_t qu_t . d_t; quiet NaN on failure
  int* status;        // (B): k_tvlqr's rule
  double* scratch;    // H * (MI*N + MI) * B float64: K_t and k_t between the sweeps, element-major ([t][e][b])
  long long B;
  int H;
  double Lxx[16], Luu[16];  // Q + Q^T (N x N), R + R^T (MI x MI), row-major, formed on the host in float64
  float x_target[4], x_min[4], x_max[4];
  int has_x_min, has_x_max;
  double w2;  // 2 * (double)barrier_weight
  // reference tracking (phnn_reference): r_t = x_ref + b * ref_bs + min(off + t, ref_rows - 1) * ref_ts, or x_target
  const float* x_ref;
  long long ref_bs, ref_ts;
  int ref_rows;
  const int* ref_off_dev;
  int ref_off_host;
  // terminal weight (phnn_terminal), read only where the backward sweep starts: with
  // W = term_W + (b / term_group) * term_bs, Tf[i][j] = (double)W[i][j] + (double)W[j][i], P_H = Lxx_H + Tf and
  // p_H = lx_H + Tf e_H (k ascending from 0.0, each product rounded, then added).  NULL: none of this is executed.
  const float* term_W;
  long long term_bs;
  int term_group;
};

// k_gn_direction_box (tests/gn_box_model.py): the plain step's arguments and the control bounds
struct GnDirectionBoxParams {
  GnDirectionParams d;
  double u_min, u_max;  // (double) of the cost's float bounds, read when has_u_bounds
  int has_u_bounds;     // 0: the step's bounds are -inf / +inf
  int* nclamp;          // (B) or NULL: (t, component) pairs held on a bound in the backward sweep; 0 on failure
};

struct GnCandidatesParams {
  const float* u;   // (B,N)
  const float* du;  // (B,N)
  const float* x0;  // (B,n), read when x0_rep is set
  float* cand;      // (B*L,N): row b*L + j = clamp(u_b + 2^-j du_b)
  float* x0_rep;    // (B*L,n) or NULL
  long long B;
  int L, N, n;
  float u_min, u_max;
  int has_u_bounds;
};

struct GnSelectParams {
  float* u;                // (B,N) in/out
  float* traj;             // (B,T) in/out, T = (H+1)*n
  float* cost;             // (B) in/out
  double* mu;              // (B) in/out
  int* accepts;            // (B) in/out
  const float* cand;       // (B*L,N)
  const float* cand_cost;  // (B*L)
  const float* cand_traj;  // (B*L,T)
  const int* status;       // (B)
  float* costs_row;        // (B) or NULL: cost_b before the update
  float* alpha_row;        // (B) or NULL: alpha_{j*}, 0 on reject
  long long B;
  int L, N, T;
  double mu_min, mu_max, mu_up, mu_down;
};

// Byte offsets of the caller-owned workspace of phnn_solve_gn, every region 256-byte aligned.
struct GnLayout {
  size_t A, Bm, traj, du, dV, status, scratch, cand, x0_rep, cand_cost, cand_traj, total;
};
GnLayout gn_layout(long long B, int H, int n, int m, int L);

// hipErrorInvalidValue: no kernel for (n, m)
hipError_t gn_direction_launch(int n, int m, const GnDirectionParams& p, hipStream_t st);
hipError_t gn_direction_box_launch(int n, int m, const GnDirectionBoxParams& p, hipStream_t st);
hipError_t gn_candidates_launch(const GnCandidatesParams& p, hipStream_t st);
hipError_t gn_select_launch(const GnSelectParams& p, hipStream_t st);
// mu[b] = mu_init, accepts[b] = 0: the entry state of phnn_solve_gn
hipError_t gn_state_launch(double* mu, int* accepts, long long B, double mu_init, hipStream_t st);
