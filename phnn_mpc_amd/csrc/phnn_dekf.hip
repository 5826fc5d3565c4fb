// phnn_dekf.hip -- the kernels of the disturbance-augmented extended Kalman filter (phnn_dekf_update / phnn_dekf_step /
// phnn_dist_compensate).  The model is x+ = F(x, c(u) + d), d+ = d: an input disturbance d that
// enters where the control enters, estimated together with the state.  k_dekf_update is k_ekf_update's algebra
// (phnn_ekf.hip) on the augmented system z = (x, d) of size NZ = N + MD, whose Jacobian [[A, Bm], [0, I]] is never
// assembled in memory; k_dekf_controls writes the control row c(u) + dhat of the prediction, k_dist_compensate takes
// dhat off a command.  tests/dekf_model.py states every operation of the update in its order (tests/ekf_model.py's
// update at size NZ); the kernel equals it bit for bit.  The unit is built with -ffp-contract=off: every product is
// rounded before it is added.
#include "phnn_dekf.h"

namespace {

constexpr int kUpdThreads = 64;
constexpr int kFlat = 256;

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the library's clamp: a NaN stays NaN, as in torch.clamp (fminf / fmaxf alone would turn it into lo)
__device__ __forceinline__ float clampf(float v, float lo, float hi, int on) { return on && v == v ? fminf(fmaxf(v, lo), hi) : v; }

// A float input of k_dekf_update, kept a scalar value of its own: without the empty asm the compiler gathers the loaded
// floats into pairs and reorders them with v_pk_mov_b32, a packed instruction this library is built without
// (tests/test_static_isa.py).
__device__ __forceinline__ float own(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ----------------------------------------------------------------------------------------------- k_dekf_update
// One thread per problem, float64 in registers; no array is indexed by a run-time value.  The rows of the augmented
// Jacobian that belong to d are the compile-time constants 0 and 1, the measurement mask has no bit at or above N, so
// the d rows and columns of S are the identity at compile time.  The products with those constants are kept (0 * inf
// is a NaN the stated order has, too); what the constants save is the registers of a fifth and sixth Jacobian row.
// One wave per SIMD (__launch_bounds__(64)): the kernel may use the unified 512-register file, which the six live
// NZ x NZ float64 matrices of the Joseph form need at NZ = 5 and 6.
template <int N, int MD>
__global__ __launch_bounds__(kUpdThreads) void k_dekf_update(DekfUpdateParams p) {
  constexpr int NZ = N + MD;
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const float* xp = p.xpred + b * p.xpred_stride;
  const float* Ab = p.A + b * (N * N);
  const float* Bb = p.Bm + b * (N * MD);
  const float* yb = p.y + b * p.y_stride;
  float* db = p.dhat + b * MD;
  double* Pb = p.Pz + b * (NZ * NZ);

  float zf[NZ];  // the prediction as floats: (x-, dhat)
  double x[NZ], A[NZ][NZ], P[NZ][NZ];
  bool bad_in = false;  // a prediction or a Jacobian that is not finite
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    zf[i] = own(i < N ? xp[i < N ? i : 0] : db[i < N ? 0 : i - N]);
    if (!finite32(zf[i])) bad_in = true;
    x[i] = (double)zf[i];
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      if (i < N) {
        const float af = own(j < N ? Ab[i * N + (j < N ? j : 0)] : Bb[i * MD + (j < N ? 0 : j - N)]);
        if (!finite32(af)) bad_in = true;
        A[i][j] = (double)af;
      } else {
        A[i][j] = i == j ? 1.0 : 0.0;
      }
      P[i][j] = Pb[i * NZ + j];
    }
  }
  // predict: M = A_z P, P- = M A_z^T + Qz, symmetrised
  double M[NZ][NZ], Pm[NZ][NZ];
#pragma unroll
  for (int i = 0; i < NZ; ++i)
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < NZ; ++k) a = a + A[i][k] * P[k][j];
      M[i][j] = a;
    }
#pragma unroll
  for (int i = 0; i < NZ; ++i)
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < NZ; ++k) a = a + M[i][k] * A[j][k];
      P[i][j] = a + p.Qz[i * NZ + j];
    }
#pragma unroll
  for (int i = 0; i < NZ; ++i)
#pragma unroll
    for (int j = i; j < NZ; ++j) {
      const double s = 0.5 * (P[i][j] + P[j][i]);
      Pm[i][j] = s;
      Pm[j][i] = s;
    }
  // innovation of the measured state components; a measurement that is not finite is a dropped one
  double nu[NZ], Rv[NZ];
  bool meas[NZ];
  bool dropout = false, any = false;
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    meas[i] = i < N && ((p.mask >> i) & 1u);
    nu[i] = 0.0;
    Rv[i] = 0.0;
    if (meas[i]) {
      any = true;
      const float yf = own(yb[i < N ? i : 0]);
      if (!finite32(yf)) dropout = true;
      nu[i] = (double)yf - x[i];
      Rv[i] = p.Rn[i < N ? i : 0];
    }
  }
  // S (lower triangle) = L D L^T, no square roots, k_tvlqr's pivot rule
  double Lf[NZ][NZ], D[NZ];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NZ; ++j) {
    double w[NZ];
    double d = meas[j] ? Pm[j][j] + Rv[j] : 1.0;
#pragma unroll
    for (int k = 0; k < j; ++k) {
      w[k] = Lf[j][k] * D[k];
      d = d - Lf[j][k] * w[k];
    }
    D[j] = d;
    if (!(d > 0.0) || d == __builtin_inf()) bad = true;
#pragma unroll
    for (int i = j + 1; i < NZ; ++i) {
      double s = meas[i] && meas[j] ? Pm[i][j] : 0.0;
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - Lf[i][k] * w[k];
      Lf[i][j] = s / d;
    }
  }
  // column c < NZ: K[c][.] = S^-1 P-[idx, c] (S is symmetric), column NZ: z = S^-1 nu, from the same factors
  double X[NZ][NZ + 1];
#pragma unroll
  for (int c = 0; c <= NZ; ++c) {
    double yv[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      // the inner c < NZ keeps the index of the unrolled c == NZ column inside Pm; that column's value is nu[i]
      double s = c < NZ ? (meas[i] ? Pm[c < NZ ? c : 0][i] : 0.0) : nu[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - Lf[i][k] * yv[k];
      yv[i] = s;
    }
#pragma unroll
    for (int i = 0; i < NZ; ++i) yv[i] = yv[i] / D[i];
#pragma unroll
    for (int i = NZ - 1; i >= 0; --i) {
      double s = yv[i];
#pragma unroll
      for (int k = i + 1; k < NZ; ++k) s = s - Lf[k][i] * X[k][c];
      X[i][c] = s;
    }
  }
  // state: zhat_i = z_i + sum_a K[i][a] nu_a, rounded once;  G = I - K C
  float xh[NZ];
  double G[NZ][NZ];
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < NZ; ++k) a = a + X[k][i] * nu[k];
    xh[i] = (float)(x[i] + a);
#pragma unroll
    for (int j = 0; j < NZ; ++j) G[i][j] = (i == j ? 1.0 : 0.0) - X[j][i];
  }
  // Joseph form: P = G P- G^T + K diag(Rn) K^T, symmetrised
  double W[NZ][NZ];
#pragma unroll
  for (int i = 0; i < NZ; ++i)
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < NZ; ++k) a = a + G[i][k] * Pm[k][j];
      W[i][j] = a;
    }
#pragma unroll
  for (int i = 0; i < NZ; ++i)
#pragma unroll
    for (int j = 0; j < NZ; ++j) {
      double a = 0.0, c = 0.0;
#pragma unroll
      for (int k = 0; k < NZ; ++k) a = a + W[i][k] * G[j][k];
#pragma unroll
      for (int k = 0; k < NZ; ++k) c = c + (X[k][i] * Rv[k]) * X[k][j];
      M[i][j] = a + c;
    }
  double nis = 0.0;
#pragma unroll
  for (int k = 0; k < NZ; ++k) nis = nis + nu[k] * X[k][NZ];

  // the outcome selects what is written
  const bool update = any && !dropout;
  const bool fail = bad_in || (update && bad);
  const double qnan = __builtin_nan("");
  if (fail || !update) nis = qnan;
#pragma unroll
  for (int i = 0; i < NZ; ++i) {
    if (fail) xh[i] = __builtin_nanf("");
    else if (!update) xh[i] = zf[i];
#pragma unroll
    for (int j = i; j < NZ; ++j) {
      double s = 0.5 * (M[i][j] + M[j][i]);
      if (fail) s = qnan;
      else if (!update) s = Pm[i][j];
      Pb[i * NZ + j] = s;
      Pb[j * NZ + i] = s;
    }
  }
  p.status[b] = fail ? 2 : (update || !any ? 0 : 1);
#pragma unroll
  for (int i = 0; i < N; ++i) p.xhat[b * N + i] = xh[i];
#pragma unroll
  for (int i = 0; i < MD; ++i) db[i] = xh[N + i];
  if (p.nis) p.nis[b] = nis;
  if (p.innov) {
#pragma unroll
    for (int i = 0; i < N; ++i) p.innov[b * N + i] = nu[i];
  }
  if (p.log_xhat || p.log_dhat || p.log_nis) {
    const long long step = p.step_dev ? *p.step_dev : p.step_host;
    if (p.log_xhat) {
#pragma unroll
      for (int i = 0; i < N; ++i) p.log_xhat[((step + 1) * p.B + b) * N + i] = xh[i];
    }
    if (p.log_dhat) {
#pragma unroll
      for (int i = 0; i < MD; ++i) p.log_dhat[((step + 1) * p.B + b) * MD + i] = xh[N + i];
    }
    if (p.log_nis) p.log_nis[step * p.B + b] = nis;
  }
}

// ----------------------------------------------------------------------------------------------- k_dekf_controls
// One thread per element of the (B,1,m) control row of the one-step prediction: the clamped command plus the
// disturbance estimate, the sum rounded once.
__global__ __launch_bounds__(kFlat) void k_dekf_controls(DekfControlsParams p) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p.B * p.m) return;
  const long long b = idx / p.m;
  const int k = (int)(idx - b * p.m);
  p.row[idx] = clampf(p.u[b * p.u_stride + k], p.u_min, p.u_max, p.has_bounds) + p.dhat[idx];
}

// ----------------------------------------------------------------------------------------------- k_dist_compensate
// One thread per problem (its status is one value): u_cmd = c(c(v) - dhat), the difference rounded once; a component
// whose estimate is not finite keeps c(v) and raises the status.
__global__ __launch_bounds__(kFlat) void k_dist_compensate(DistCompensateParams p) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  int st = 0;
  for (int k = 0; k < p.m; ++k) {
    const float cv = clampf(p.v[b * p.v_stride + k], p.u_min, p.u_max, p.has_bounds);
    const float d = p.dhat[b * p.m + k];
    float u = cv;
    if (finite32(d)) u = clampf(cv - d, p.u_min, p.u_max, p.has_bounds);
    else st = 1;
    p.u_cmd[b * p.m + k] = u;
  }
  if (p.status) p.status[b] = st;
}

template <int N, int MD>
hipError_t update_launch(const DekfUpdateParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kUpdThreads - 1) / kUpdThreads);
  hipLaunchKernelGGL((k_dekf_update<N, MD>), dim3(grid), dim3(kUpdThreads), 0, st, p);
  return hipGetLastError();
}

}  // namespace

bool dekf_has_kernel(int n, int m) { return (m == 1 && n >= 2 && n <= 4) || (m == 2 && n == 4); }

hipError_t dekf_update_launch(int n, int m, const DekfUpdateParams& p, hipStream_t st) {
  if (m == 1 && n == 2) return update_launch<2, 1>(p, st);
  if (m == 1 && n == 3) return update_launch<3, 1>(p, st);
  if (m == 1 && n == 4) return update_launch<4, 1>(p, st);
  if (m == 2 && n == 4) return update_launch<4, 2>(p, st);
  return hipErrorInvalidValue;
}

hipError_t dekf_controls_launch(const DekfControlsParams& p, hipStream_t st) {
  hipLaunchKernelGGL(k_dekf_controls, dim3((unsigned)((p.B * p.m + kFlat - 1) / kFlat)), dim3(kFlat), 0, st, p);
  return hipGetLastError();
}

hipError_t dist_compensate_launch(const DistCompensateParams& p, hipStream_t st) {
  hipLaunchKernelGGL(k_dist_compensate, dim3((unsigned)((p.B + kFlat - 1) / kFlat)), dim3(kFlat), 0, st, p);
  return hipGetLastError();
}
