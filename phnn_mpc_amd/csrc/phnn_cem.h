// phnn_cem.h -- the kernels of the batched cross-entropy (CEM) solve (phnn_cem.hip) as the host side (phnn_mpc.hip)
// sees them.  DESIGN.md section 13.  The noise counter, its ranges and the H * m <= 256 limit are MPPI's (phnn_mppi.h).
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

struct CemSampleParams {
  const float* u;    // (B, N) means
  const float* sig;  // (B, N) standard deviations, per problem and element
  const float* x0;   // (B, n)
  float* v;          // (B*K, N) samples: row b*K + k = clamp(u_b + sig_b o z_{b,k}); z_{b,0} = 0
  float* x0_rep;     // (B*K, n) x0_b replicated, or NULL
  long long B;
  int K, N, n;
  float u_min, u_max;
  int has_u_bounds;
  unsigned key0, key1;       // seed
  long long problem_offset;  // gid = problem_offset + b
  const int* epoch_dev;      // read by the launch when not NULL, else epoch_host
  int epoch_host;
  int iteration;
};

struct CemUpdateParams {
  float* u;          // (B, N) mean, refitted in place (kept where every cost is non-finite)
  float* sig;        // (B, N) standard deviation, refitted in place (kept likewise)
  const float* v;    // (B*K, N) samples
  const float* s;    // (B*K) their costs
  float* costs_out;  // (B) S_{b,0}, or NULL
  float* best_cost;  // (B) lowest sample cost seen so far (strict '<'), or NULL
  float* best_u;     // (B, N) its sample row
  long long B;
  int K, N;
  int elites;        // E: the E lowest finite costs (cost, then k ascending) are refitted to
  float alpha;       // smoothing: new = alpha * old + (1 - alpha) * elite statistic
  float sigma_min;   // floor of the refitted standard deviation
  float u_min, u_max;
  int has_u_bounds;
};

struct CemLayout {  // byte offsets of the caller-owned workspace: MPPI's regions, then the sigma state (B, N)
  size_t v, x0_rep, s, sig, total;
};
CemLayout cem_layout(long long B, int N, int n, int K);

hipError_t cem_sample_launch(const CemSampleParams& p, hipStream_t st);
hipError_t cem_update_launch(const CemUpdateParams& p, hipStream_t st);
// sig[b, t, c] = sigma_init[c] (count = B * N floats, m components): the entry of phnn_solve_cem
hipError_t cem_sigma_init_launch(float* sig, long long count, int m, const float* sigma_init, hipStream_t st);
