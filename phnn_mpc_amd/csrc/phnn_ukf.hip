// phnn_ukf.hip -- the kernels of the batched unscented Kalman filter (phnn_ukf_sigma / phnn_ukf_moments /
// phnn_ukf_step).  Per problem, k_ukf_sigma factors P = L L^T and writes the S = 2 N + 1 sigma
// points xhat, xhat +- gamma L[:,c] as float32 rollouts for K1, with the applied control copied to each of them;
// k_ukf_moments forms the weighted mean and covariance of their images and the identity that k_ekf_update
// (phnn_ekf.hip) then takes as its Jacobian.  The kernels see the weights gamma, wm0, wc0, wi only, never alpha, beta
// or kappa.  tests/ukf_model.py states every operation of both in its order; the kernels equal it bit for bit.  The
// unit is built with -ffp-contract=off: every product is rounded before it is added.
#include "phnn_ukf.h"

namespace {

constexpr int kThreads = 64;

__device__ __forceinline__ bool finite32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// A float that goes in or out of a kernel here, kept a scalar value of its own: without the empty asm the compiler
// gathers neighbouring floats into pairs and moves them with v_pk_mov_b32, a packed instruction this library is built
// without (tests/test_static_isa.py; phnn_dekf.hip has the same remedy).
__device__ __forceinline__ float own(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// ------------------------------------------------------------------------------------------------- k_ukf_sigma
// One thread per problem, float64 in registers; no array is indexed by a run-time value.  Cholesky by columns with the
// sums in ascending k; a pivot with !(d > 0) or d = +inf, or an xhat that is not finite, is a failure: every sigma point
// of the problem is then a quiet NaN, which K1 keeps NaN, so that k_ekf_update ends the step in status 2.  The control
// rows are copied in every case.
template <int N>
__global__ __launch_bounds__(kThreads) void k_ukf_sigma(UkfSigmaParams p) {
  constexpr int S = 2 * N + 1;
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const float* xb = p.xhat + b * N;
  const double* Pb = p.P + b * (N * N);
  float* cb = p.chi + b * (S * N);

  float xf[N];
  double x[N];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    xf[i] = own(xb[i]);
    if (!finite32(xf[i])) bad = true;
    x[i] = (double)xf[i];
  }
  double L[N][N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = Pb[j * N + j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (!(d > 0.0) || d == __builtin_inf()) bad = true;
    const double r = __builtin_sqrt(d);
    L[j][j] = r;
#pragma unroll
    for (int i = 0; i < j; ++i) L[i][j] = 0.0;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double s = Pb[i * N + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / r;
    }
  }
  const float qnan = __builtin_nanf("");
#pragma unroll
  for (int i = 0; i < N; ++i) cb[i] = own(bad ? qnan : xf[i]);
#pragma unroll
  for (int c = 0; c < N; ++c)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double g = p.gamma * L[i][c];  // the product first, then the sum, one rounding to float32
      const float plus = (float)(x[i] + g), minus = (float)(x[i] - g);
      cb[(1 + c) * N + i] = own(bad ? qnan : plus);
      cb[(1 + N + c) * N + i] = own(bad ? qnan : minus);
    }
  if (p.ctrl) {
    const float* ub = p.u + b * p.u_stride;
    float* rb = p.ctrl + b * (S * p.m);
    for (int k = 0; k < p.m; ++k) {
      const float v = own(ub[k]);
#pragma unroll
      for (int s = 0; s < S; ++s) rb[s * p.m + k] = v;
    }
  }
}

// ------------------------------------------------------------------------------------------------- k_ukf_moments
// One thread per problem.  The mean is wm0 Y_0 + wi Y_1 + ... from an accumulator 0.0 in ascending k, the deviations are
// taken from that float64 mean, and an entry of the covariance is wc0 (e_0i e_0j) + wi (e_1i e_1j) + ...: the product of
// the deviations rounded first, then the weight times it, then the sum.
template <int N>
__global__ __launch_bounds__(kThreads) void k_ukf_moments(UkfMomentsParams p) {
  constexpr int S = 2 * N + 1;
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  const float* Yb = p.Y + b * S * p.Y_stride;
  double* Pb = p.Pm + b * (N * N);

  double e[S][N], xm[N];
#pragma unroll
  for (int k = 0; k < S; ++k)
#pragma unroll
    for (int i = 0; i < N; ++i) e[k][i] = (double)own(Yb[k * p.Y_stride + i]);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double a = 0.0;
    a = a + p.wm0 * e[0][i];
#pragma unroll
    for (int k = 1; k < S; ++k) a = a + p.wi * e[k][i];
    xm[i] = a;
  }
#pragma unroll
  for (int k = 0; k < S; ++k)
#pragma unroll
    for (int i = 0; i < N; ++i) e[k][i] = e[k][i] - xm[i];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) {
      double a = 0.0;
      a = a + p.wc0 * (e[0][i] * e[0][j]);
#pragma unroll
      for (int k = 1; k < S; ++k) a = a + p.wi * (e[k][i] * e[k][j]);
      Pb[i * N + j] = a;
      Pb[j * N + i] = a;
    }
#pragma unroll
  for (int i = 0; i < N; ++i) p.xm[b * N + i] = own((float)xm[i]);
  if (p.eye) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = 0; j < N; ++j) p.eye[b * (N * N) + i * N + j] = own(i == j ? 1.f : 0.f);
  }
}

template <int N>
hipError_t sigma_launch(const UkfSigmaParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kThreads - 1) / kThreads);
  hipLaunchKernelGGL((k_ukf_sigma<N>), dim3(grid), dim3(kThreads), 0, st, p);
  return hipGetLastError();
}

template <int N>
hipError_t moments_launch(const UkfMomentsParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kThreads - 1) / kThreads);
  hipLaunchKernelGGL((k_ukf_moments<N>), dim3(grid), dim3(kThreads), 0, st, p);
  return hipGetLastError();
}

}  // namespace

hipError_t ukf_sigma_launch(int n, const UkfSigmaParams& p, hipStream_t st) {
  switch (n) {
    case 2: return sigma_launch<2>(p, st);
    case 3: return sigma_launch<3>(p, st);
    case 4: return sigma_launch<4>(p, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t ukf_moments_launch(int n, const UkfMomentsParams& p, hipStream_t st) {
  switch (n) {
    case 2: return moments_launch<2>(p, st);
    case 3: return moments_launch<3>(p, st);
    case 4: return moments_launch<4>(p, st);
    default: return hipErrorInvalidValue;
  }
}
