// phnn_sampling.h -- the kernels of the two batched sampling solves, MPPI (phnn_solve_mppi) and cross-entropy
// (phnn_solve_cem), as the host side (phnn_mpc.hip) sees them: one sample kernel for both, one update kernel each.
// Kernels in phnn_sampling.hip.  DESIGN.md sections 12 and 13.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

// Noise counter (Philox4x32-10).  The four normals of float4 j of sample k of problem gid at (epoch, iteration) come
// from ONE Philox call with
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (gid & 0xffffffff, (gid >> 32) | (iteration << 16), epoch, (k << 6) | j)
// so the supported ranges are gid < 2^48, iteration < 2^16, epoch any 32-bit pattern, k < 2^26, j < 64 (H*m <= 256);
// distinct tuples inside them never share a counter.
constexpr int kSamplingMaxN = 256;  // H * m (16 lanes x 4 float4 per problem in the update kernels)
constexpr int kSamplingMaxIters = 1 << 16;
constexpr int kSamplingMaxSamples = 1 << 26;
constexpr long long kSamplingMaxProblem = 1LL << 48;

struct SampleParams {
  const float* u;    // (B, N) nominal controls (MPPI) / means (CEM)
  const float* sig;  // (B, N) standard deviations per problem and element (CEM), or NULL: the table `sigma` (MPPI)
  const float* x0;   // (B, n)
  float* v;          // (B*K, N) samples: row b*K + k = clamp(u_b + sigma o z_{b,k}); z_{b,0} = 0
  float* x0_rep;     // (B*K, n) x0_b replicated, or NULL
  long long B;
  int K, N, n, m;
  float sigma[4];    // per control component; read when sig is NULL
  float u_min, u_max;
  int has_u_bounds;
  unsigned key0, key1;       // seed
  long long problem_offset;  // gid = problem_offset + b
  const int* epoch_dev;      // read by the launch when not NULL, else epoch_host
  int epoch_host;
  int iteration;
};

struct MppiUpdateParams {
  float* u;               // (B, N) nominal, replaced by the weighted mean (kept where every cost is non-finite)
  const float* v;         // (B*K, N) samples
  const float* s;         // (B*K) their costs
  float* costs_out;       // (B) S_{b,0}, or NULL
  float* best_cost;       // (B) lowest sample cost seen so far (strict '<'), or NULL
  float* best_u;          // (B, N) its sample row
  long long B;
  int K, N;
  float lambda;
  float u_min, u_max;  // the mean is clamped: rounding can carry a combination of in-bound rows one ulp past a bound
  int has_u_bounds;
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

// Byte offsets of the caller-owned workspace, every region 256-byte aligned: samples, replicated x0, K1's costs, and
// with sigma_state (CEM) the standard deviations (B, N) after them; without it sig == total.
struct SamplingLayout {
  size_t v, x0_rep, s, sig, total;
};
SamplingLayout sampling_layout(long long B, int N, int n, int K, bool sigma_state);

hipError_t sample_launch(const SampleParams& p, hipStream_t st);
// k_shaped_sample: sample_launch with a noise shape L (H = N / m rows, P columns, row-major, device, read-only):
// z[t, c] = sum_{s < P} L[t, s] * eps[s, c], eps the white normals of a row of length P * m.
hipError_t sample_shaped_launch(const SampleParams& p, const float* L, int P, hipStream_t st);
// Bytes of LDS k_shaped_sample stages an (H, P) shape in (row stride P | 1 floats), or 0: too large, L is read from
// global memory.  Introspection for tests and tools.
size_t sample_shaped_lds_bytes(int H, int P);
hipError_t mppi_update_launch(const MppiUpdateParams& p, hipStream_t st);
hipError_t cem_update_launch(const CemUpdateParams& p, hipStream_t st);
// u <- clamp(u) in place (count floats): the entry of both solves
hipError_t clamp_launch(float* u, long long count, float u_min, float u_max, hipStream_t st);
// sig[b, t, c] = sigma_init[c] (count = B * N floats, m components): the entry of phnn_solve_cem
hipError_t sigma_init_launch(float* sig, long long count, int m, const float* sigma_init, hipStream_t st);

// k_plant_step_ex (phnn_plant_step_ex): k_plant_step with per-plant parameters, a force
// disturbance, measurement noise, a freeze at termination and running metrics.  It lives in this unit because the noise
// is the sampler's: z0 and the four measurement normals of plant gid at step s are the normals of float4 0 and float4 1
// of sample 1 of problem gid at (seed, epoch = s, iteration = 0), i.e. counter words (gid, gid >> 32, s, 1 << 6 | 0 / 1).
struct PlantExParams {
  double gravity, masscart, masspole, length, dt, x_limit, theta_limit;  // the phnn_plant
  double* state;        // (B,4) in/out
  const float* action;  // action[b * stride]
  long long stride, B;
  int has_u_bounds;
  float u_min, u_max;
  float* state_f32;
  int* done_step;
  const int* step_dev;
  int step_host;
  double* log_states;    // (T+1,B,4)
  float* log_controls;   // (T,B)
  const double* params;  // (B,4) gravity, masscart, masspole, length per plant, or NULL: the shared ones above
  const float* force_bias;  // (B) or NULL
  float force_sigma;
  float meas_sigma[4];
  unsigned key0, key1;     // seed
  long long plant_offset;  // gid = plant_offset + b
  int freeze_done;
  float* disturbance_log;  // (T,B) or NULL
  int has_metrics;
  double Q[16], R, target[4], tol[4];
  double* cost_acc;  // (B)
  int* run;          // (B)
  int* best_run;     // (B)
};
hipError_t plant_step_ex_launch(const PlantExParams& p, hipStream_t st);
