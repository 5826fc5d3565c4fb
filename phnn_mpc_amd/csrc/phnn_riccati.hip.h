// phnn_riccati.hip.h -- ONE Riccati step of the LQ backward pass, shared by k_tvlqr (phnn_kernels.hip.h, a new (A, B)
// at every step) and k_dare (phnn_terminal.hip, the same (A, B) until the cost-to-go stands still).  float64 in
// registers, every product rounded before it is added (the units are built with -ffp-contract=off), every inner product
// with its index ascending from an accumulator 0.0; tests/tvlqr_model.py states the order:
//   S = P A,  T = P B,  Qxx = Lxx + A^T S,  Qux = B^T S,  Quu = Luu + B^T T (+ mu on the diagonal, added last), lower
//   triangle only;  Quu = L D L^T without square roots, a pivot d with !(d > 0) or d = +inf is a failure;
//   X = Quu^-1 Qux column by column (forward, divide by D, backward);  P <- Qxx - Qux^T X, symmetrised as
//   P[i][j] = P[j][i] = 0.5 (P[i][j] + P[j][i]).   The gain of the step is K = -X.
#pragma once
#include <hip/hip_runtime.h>

// -> false on a pivot failure (P and X are left as they were), else true with P replaced and X filled.
template <int N, int MI>
__device__ __forceinline__ bool riccati_step(double (&P)[N][N], const double (&A)[N][N], const double (&Bt)[N][MI],
                                             const double* Lxx, const double* Luu, double mu, double (&X)[MI][N]) {
  double S[N][N], T[N][MI];
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + P[i][k] * A[k][j];
      S[i][j] = a;
    }
#pragma unroll
    for (int j = 0; j < MI; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + P[i][k] * Bt[k][j];
      T[i][j] = a;
    }
  }
  double Qxx[N][N], Qux[MI][N], Quu[MI][MI];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + A[k][i] * S[k][j];
      Qxx[i][j] = Lxx[i * N + j] + a;
    }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + Bt[k][i] * S[k][j];
      Qux[i][j] = a;
    }
#pragma unroll
    for (int j = 0; j <= i; ++j) {  // lower triangle only
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + Bt[k][i] * T[k][j];
      double q = Luu[i * MI + j] + a;
      if (i == j) q = q + mu;
      Quu[i][j] = q;
    }
  }
  // Quu = L D L^T, no square roots
  double Lf[MI][MI], D[MI];
  bool bad = false;
#pragma unroll
  for (int j = 0; j < MI; ++j) {
    double w[MI];
    double d = Quu[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) {
      w[k] = Lf[j][k] * D[k];
      d = d - Lf[j][k] * w[k];
    }
    D[j] = d;
    if (!(d > 0.0) || d == __builtin_inf()) bad = true;
#pragma unroll
    for (int i = j + 1; i < MI; ++i) {
      double s = Quu[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - Lf[i][k] * w[k];
      Lf[i][j] = s / d;
    }
  }
  if (bad) return false;
#pragma unroll
  for (int c = 0; c < N; ++c) {
    double y[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      double s = Qux[i][c];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - Lf[i][k] * y[k];
      y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) y[i] = y[i] / D[i];
#pragma unroll
    for (int i = MI - 1; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < MI; ++k) s = s - Lf[k][i] * X[k][c];
      X[i][c] = s;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < MI; ++k) a = a + Qux[k][i] * X[k][j];
      S[i][j] = Qxx[i][j] - a;
    }
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = i; j < N; ++j) {
      const double s = 0.5 * (S[i][j] + S[j][i]);
      P[i][j] = s;
      P[j][i] = s;
    }
  return true;
}
