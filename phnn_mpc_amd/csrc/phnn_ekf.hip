// phnn_ekf.hip -- the kernels of the batched extended Kalman filter (phnn_ekf_update / phnn_ekf_step, DESIGN.md section
// 20): per problem the covariance propagation P- = A P A^T + Qn through the Jacobian of the prediction step and the
// measurement update for a selection of state components (k_ekf_update), and the copy of the applied control into the
// one-step control row of the prediction (k_ekf_controls).  tests/ekf_model.py states every operation of the update in
// its order; the kernel equals it bit for bit.  The unit is built with -ffp-contract=off: every product is rounded
// before it is added.
#include "phnn_ekf.h"

namespace {

constexpr int kUpdThreads = 64;
constexpr int kFlat = 256;

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ------------------------------------------------------------------------------------------------ k_ekf_update
// One thread per problem, float64 in registers; no array is indexed by a run-time value.  The measured components are
// a bit mask shared by the batch, so the branches on it are uniform.  The innovation covariance is held at its full
// size N with the rows and columns of the unmeasured components replaced by the identity (their innovation is 0): the
// L D L^T routine of k_tvlqr then runs at a compile-time size, every entry it forms for an unmeasured component is an
// exact 0 or 1, and the entries of the measured ones see the operations of the factorisation of S = P-[idx, idx] +
// diag(Rn[idx]) in their order.  Everything is computed for every problem and the outcome (update, no update, failure)
// selects what is written, as tests/ekf_model.py does it.
template <int N>
__global__ __launch_bounds__(kUpdThreads) void k_ekf_update(EkfUpdateParams p) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const float* xp = p.xpred + b * p.xpred_stride;
  const float* Ab = p.A + b * (N * N);
  const float* yb = p.y + b * p.y_stride;
  double* Pb = p.P + b * (N * N);

  double x[N], A[N][N], P[N][N];
  bool bad_in = false;  // a prediction or a Jacobian that is not finite
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float xf = xp[i];
    if (!finite32(xf)) bad_in = true;
    x[i] = (double)xf;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float af = Ab[i * N + j];
      if (!finite32(af)) bad_in = true;
      A[i][j] = (double)af;
      P[i][j] = Pb[i * N + j];
    }
  }
  // predict: M = A P, P- = M A^T + Qn, symmetrised
  double M[N][N], Pm[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + A[i][k] * P[k][j];
      M[i][j] = a;
    }
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + M[i][k] * A[j][k];
      P[i][j] = a + p.Qn[i * N + j];
    }
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) {
      const double s = 0.5 * (P[i][j] + P[j][i]);
      Pm[i][j] = s;
      Pm[j][i] = s;
    }
  // innovation of the measured components; a measurement that is not finite is a dropped one
  double nu[N], Rv[N];
  bool meas[N];
  bool dropout = false, any = false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    meas[i] = (p.mask >> i) & 1u;
    nu[i] = 0.0;
    Rv[i] = 0.0;
    if (meas[i]) {
      any = true;
      const float yf = yb[i];
      if (!finite32(yf)) dropout = true;
      nu[i] = (double)yf - x[i];
      Rv[i] = p.Rn[i];
    }
  }
  // S (lower triangle) = L D L^T, no square roots, k_tvlqr's pivot rule
  double Lf[N][N], D[N];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double w[N];
    double d = meas[j] ? Pm[j][j] + Rv[j] : 1.0;
#pragma unroll
    for (int k = 0; k < j; ++k) {
      w[k] = Lf[j][k] * D[k];
      d = d - Lf[j][k] * w[k];
    }
    D[j] = d;
    if (!(d > 0.0) || d == __builtin_inf()) bad = true;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double s = meas[i] && meas[j] ? Pm[i][j] : 0.0;
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - Lf[i][k] * w[k];
      Lf[i][j] = s / d;
    }
  }
  // column c < N: K[c][.] = S^-1 P-[idx, c] (S is symmetric), column N: z = S^-1 nu, from the same factors
  double X[N][N + 1];
#pragma unroll
  for (int c = 0; c <= N; ++c) {
    double yv[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      // the inner c < N keeps the index of the unrolled c == N column inside Pm; that column's value is nu[i]
      double s = c < N ? (meas[i] ? Pm[c < N ? c : 0][i] : 0.0) : nu[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - Lf[i][k] * yv[k];
      yv[i] = s;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) yv[i] = yv[i] / D[i];
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
      double s = yv[i];
#pragma unroll
      for (int k = i + 1; k < N; ++k) s = s - Lf[k][i] * X[k][c];
      X[i][c] = s;
    }
  }
  // state: xhat_i = x_i + sum_a K[i][a] nu_a, rounded once;  G = I - K C
  float xh[N];
  double G[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) a = a + X[k][i] * nu[k];
    xh[i] = (float)(x[i] + a);
#pragma unroll
    for (int j = 0; j < N; ++j) G[i][j] = (i == j ? 1.0 : 0.0) - X[j][i];
  }
  // Joseph form: P = G P- G^T + K diag(Rn) K^T, symmetrised
  double W[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + G[i][k] * Pm[k][j];
      W[i][j] = a;
    }
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0, c = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + W[i][k] * G[j][k];
#pragma unroll
      for (int k = 0; k < N; ++k) c = c + (X[k][i] * Rv[k]) * X[k][j];
      M[i][j] = a + c;
    }
  double nis = 0.0;
#pragma unroll
  for (int k = 0; k < N; ++k) nis = nis + nu[k] * X[k][N];

  // the outcome selects what is written
  const bool update = any && !dropout;
  const bool fail = bad_in || (update && bad);
  const double qnan = __builtin_nan("");
  if (fail || !update) nis = qnan;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (fail) xh[i] = __builtin_nanf("");
    else if (!update) xh[i] = xp[i];
#pragma unroll
    for (int j = i; j < N; ++j) {
      double s = 0.5 * (M[i][j] + M[j][i]);
      if (fail) s = qnan;
      else if (!update) s = Pm[i][j];
      Pb[i * N + j] = s;
      Pb[j * N + i] = s;
    }
  }
  p.status[b] = fail ? 2 : (update || !any ? 0 : 1);
#pragma unroll
  for (int i = 0; i < N; ++i) p.xhat[b * N + i] = xh[i];
  if (p.nis) p.nis[b] = nis;
  if (p.innov) {
#pragma unroll
    for (int i = 0; i < N; ++i) p.innov[b * N + i] = nu[i];
  }
  if (p.log_xhat || p.log_nis) {
    const long long step = p.step_dev ? *p.step_dev : p.step_host;
    if (p.log_xhat) {
#pragma unroll
      for (int i = 0; i < N; ++i) p.log_xhat[((step + 1) * p.B + b) * N + i] = xh[i];
    }
    if (p.log_nis) p.log_nis[step * p.B + b] = nis;
  }
}

// ------------------------------------------------------------------------------------------------ k_ekf_controls
// One thread per element of the (B,1,m) control row of the one-step prediction.
__global__ __launch_bounds__(kFlat) void k_ekf_controls(EkfControlsParams p) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.B * p.m) return;
  const long long b = idx / p.m;
  const int k = (int)(idx - b * p.m);
  p.row[idx] = p.u[b * p.u_stride + k];
}

template <int N>
hipError_t update_launch(const EkfUpdateParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kUpdThreads - 1) / kUpdThreads);
  hipLaunchKernelGGL((k_ekf_update<N>), dim3(grid), dim3(kUpdThreads), 0, st, p);
  return hipGetLastError();
}

}  // namespace

hipError_t ekf_update_launch(int n, const EkfUpdateParams& p, hipStream_t st) {
  switch (n) {
    case 2: return update_launch<2>(p, st);
    case 3: return update_launch<3>(p, st);
    case 4: return update_launch<4>(p, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t ekf_controls_launch(const EkfControlsParams& p, hipStream_t st) {
  hipLaunchKernelGGL(k_ekf_controls, dim3((unsigned)((p.B * p.m + kFlat - 1) / kFlat)), dim3(kFlat), 0, st, p);
  return hipGetLastError();
}
