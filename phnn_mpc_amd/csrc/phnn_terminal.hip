// phnn_terminal.hip -- the kernels of the terminal cost: k_terminal_cost, the quadratic form
// e_H^T W e_H behind a K1 launch with row H of the cotangent that K2 reads, and k_dare, the fixed point of k_tvlqr's
// Riccati step on one (A, B).  tests/terminal_model.py states every operation in its order; the kernels equal it bit for
// bit.  The unit is built with -ffp-contract=off: the only fused multiply-adds are the ones written out below.
#include "phnn_terminal.h"

#include "phnn_riccati.hip.h"

namespace {

constexpr int kTermThreads = 256;
constexpr int kDareThreads = 64;

// ------------------------------------------------------------------------------------------------ k_terminal_cost
// One thread per rollout, float32.  With e = x_H - r (formed as state_cost forms it, r the reference row
// min(off + H, rows - 1) of K1's rule or the cost's x_target):
//   s_j = fma(e_i, W[i][j], s_j), i ascending from 0;  c = fma(s_j, e_j, c), j ascending from 0;  cost[b] = cost[b] + c
//   traj_bar[b,H,i] = g_i,  g_i = fma(W[i][j] + W[j][i], e_j, g_i), j ascending from 0, the sum of the two weights
//   rounded once in float32.
template <int N>
__global__ __launch_bounds__(kTermThreads) void k_terminal_cost(TerminalCostParams p) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const float* x = p.traj + (b * (p.H + 1) + p.H) * N;
  const float* W = p.W + (b / p.group) * p.w_bs;
  float e[N];
  if (p.x_ref) {
    const int last = p.ref_rows - 1;
    const int o = p.ref_off_dev ? *p.ref_off_dev : p.ref_off_host;
    const int off = o < 0 ? 0 : (o > last ? last : o);
    const int r = p.H < last - off ? off + p.H : last;
    const float* q = p.x_ref + b * p.ref_bs + r * p.ref_ts;
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = x[i] - q[i];
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = x[i] - p.x_target[i];
  }
  float w[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) w[i][j] = W[i * N + j];
  float c = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) s = __builtin_fmaf(e[i], w[i][j], s);
    c = __builtin_fmaf(s, e[j], c);
  }
  p.cost[b] = p.cost[b] + c;
  if (p.traj_bar) {
    float* g = p.traj_bar + (b * (p.H + 1) + p.H) * N;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      float a = 0.f;
#pragma unroll
      for (int j = 0; j < N; ++j) a = __builtin_fmaf(w[i][j] + w[j][i], e[j], a);
      g[i] = a;
    }
  }
}

// ------------------------------------------------------------------------------------------------ k_dare
// One thread per problem, float64 in registers.  P_0 = Lxx; step k = 1, 2, ...: riccati_step (k_tvlqr's) on the same
// (A, B) gives P_k and X_k; then d = max |P_k - P_{k-1}|, s = max |P_k| over the entries (row-major order).  A failed
// pivot, or an s that is NaN or +inf: status 1.  d <= tol * s: status 0.  k == max_iters: status 2.  On status 0 and 2:
// P = P_k, K = -X_k, W = (float)(0.5 * (P_k - Lxx)) entry by entry (the stage cost already charges Q at t = H); a W
// entry that is not finite turns the problem into status 1.  Status 1 leaves P, K and W quiet NaN.  iters = k.
template <int N, int MI>
__global__ __launch_bounds__(kDareThreads) void k_dare(DareParams p) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  double A[N][N], Bt[N][MI], P[N][N], X[MI][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      A[i][j] = (double)p.A[b * (N * N) + i * N + j];
      P[i][j] = p.Lxx[i * N + j];
    }
#pragma unroll
    for (int j = 0; j < MI; ++j) Bt[i][j] = (double)p.Bm[b * (N * MI) + i * MI + j];
  }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) X[i][j] = 0.0;
  int status = 2, k = 0;
  while (k < p.max_iters) {
    double Pp[N][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) Pp[i][j] = P[i][j];
    k = k + 1;
    if (!riccati_step<N, MI>(P, A, Bt, p.Lxx, p.Luu, p.mu, X)) {
      status = 1;
      break;
    }
    double d = 0.0, s = 0.0;
    bool nan = false;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const double a = fabs(P[i][j]), c = fabs(P[i][j] - Pp[i][j]);
        if (a != a) nan = true;
        if (a > s) s = a;
        if (c > d) d = c;
      }
    if (nan || s == __builtin_inf()) {
      status = 1;
      break;
    }
    if (d <= p.tol * s) {
      status = 0;
      break;
    }
  }
  float Wf[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      Wf[i][j] = (float)(0.5 * (P[i][j] - p.Lxx[i * N + j]));
      if (!(fabsf(Wf[i][j]) < __builtin_inff())) status = 1;
    }
  const bool ok = status != 1;
  const double qnan = __builtin_nan("");
  const float qnanf = __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      p.P[b * (N * N) + i * N + j] = ok ? P[i][j] : qnan;
      p.W[b * (N * N) + i * N + j] = ok ? Wf[i][j] : qnanf;
    }
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) p.K[b * (MI * N) + i * N + j] = ok ? -X[i][j] : qnan;
  p.iters[b] = k;
  p.status[b] = status;
}

template <int N>
hipError_t terminal_launch(const TerminalCostParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kTermThreads - 1) / kTermThreads);
  hipLaunchKernelGGL((k_terminal_cost<N>), dim3(grid), dim3(kTermThreads), 0, st, p);
  return hipGetLastError();
}

template <int N, int MI>
hipError_t dare_launch_nm(const DareParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kDareThreads - 1) / kDareThreads);
  hipLaunchKernelGGL((k_dare<N, MI>), dim3(grid), dim3(kDareThreads), 0, st, p);
  return hipGetLastError();
}

}  // namespace

hipError_t terminal_cost_launch(int n, const TerminalCostParams& p, hipStream_t st) {
  switch (n) {
    case 2: return terminal_launch<2>(p, st);
    case 3: return terminal_launch<3>(p, st);
    case 4: return terminal_launch<4>(p, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t dare_launch(int n, int m, const DareParams& p, hipStream_t st) {
  switch (n * 8 + m) {
#define PHNN_DARE_CASE(N, MI) \
  case N * 8 + MI: return dare_launch_nm<N, MI>(p, st);
#define PHNN_DARE_ROW(N) PHNN_DARE_CASE(N, 1) PHNN_DARE_CASE(N, 2) PHNN_DARE_CASE(N, 3) PHNN_DARE_CASE(N, 4)
    PHNN_DARE_ROW(2)
    PHNN_DARE_ROW(3)
    PHNN_DARE_ROW(4)
#undef PHNN_DARE_ROW
#undef PHNN_DARE_CASE
    default: return hipErrorInvalidValue;
  }
}
