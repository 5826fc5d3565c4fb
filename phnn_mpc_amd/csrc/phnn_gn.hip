// phnn_gn.hip -- the kernels of the batched Gauss-Newton solve (phnn_solve_gn, DESIGN.md sections 18 and 19): per problem the
// LQ step on the local model (A_t, B_t) of phnn_rollout_linearize with the gradients of the stage cost
// (k_gn_direction), the L candidates u + 2^-j du of the backtracking line search (k_gn_candidates) and, after ONE K1
// launch over all B * L of them, the choice among them with the Levenberg-Marquardt update of mu (k_gn_select).
// tests/gn_model.py states every operation in its order; the kernels equal it bit for bit.  The unit is built with
// -ffp-contract=off: every product is rounded before it is added.
#include "phnn_gn.h"

#include "phnn_rows.hip.h"

using phnn_rows::clampf;
using phnn_rows::finite;

namespace {

constexpr int kDirThreads = 64;
constexpr int kFlat = 256;

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The terminal weight in the initialisation of both backward sweeps (tests/terminal_model.py):
// Tf[i][j] = (double)W[i][j] + (double)W[j][i], P_H = Lxx_H + Tf, p_H = lx_H + Tf e_H with k ascending from 0.0, each
// product rounded, then added.  Called only with a terminal weight, so a solve without one executes none of it.
template <int N>
__device__ __forceinline__ void terminal_init(const GnDirectionParams& p, long long b, const double (&e)[N],
                                              const double (&lx)[N], double (&P)[N][N], double (&pv)[N]) {
  const float* W = p.term_W + (b / p.term_group) * p.term_bs;
  double Tf[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) Tf[i][j] = (double)W[i * N + j] + (double)W[j * N + i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j < N; ++j) P[i][j] = P[i][j] + Tf[i][j];
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) a = a + Tf[i][k] * e[k];
    pv[i] = lx[i] + a;
  }
}

// ------------------------------------------------------------------------------------------------ k_gn_direction
// One thread per problem, float64 in registers.  The backward step is the TWIN of k_tvlqr's (phnn_kernels.hip.h) with the
// affine terms added: S, T, Qxx, Qux, Quu, the LDL^T factorisation, X, K_t and the symmetrised P_t are formed exactly
// as there (tests/tvlqr_model.py); a change to one of the two belongs in the other.  Added here: Lxx_t with the active
// barrier rows, qx, qu, the solve d = Quu^-1 qu from the same factors, k_t, p_t and dV, then the forward sweep on the
// linear model.  K_t and k_t wait in `scratch` between the sweeps, element-major so that the 64 threads of a
// workgroup touch neighbouring doubles.
template <int N, int MI>
__global__ __launch_bounds__(kDirThreads) void k_gn_direction(GnDirectionParams p) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  constexpr int E = MI * N + MI;
  const float* Ab = p.A + b * p.H * (N * N);
  const float* Bb = p.Bm + b * p.H * (N * MI);
  const float* xb = p.traj + b * (p.H + 1) * N;
  const float* ub = p.u + b * p.H * MI;
  float* dub = p.du + b * p.H * MI;
  double* scr = p.scratch + b;
  const double mu = p.mu[b];
  // the reference rows of this problem (phnn_reference), or the cost's target
  const float* rbase = p.x_ref ? p.x_ref + b * p.ref_bs : nullptr;
  int roff = 0;
  const int rlast = p.ref_rows - 1;
  if (rbase) {
    const int o = p.ref_off_dev ? *p.ref_off_dev : p.ref_off_host;
    roff = o < 0 ? 0 : (o > rlast ? rlast : o);
  }

  double P[N][N], pv[N];
  double dV = 0.0;
  int t = p.H;
  for (; t >= 0; --t) {
    // the stage cost's gradient and curvature at x_t: e = x - r, Lxx_t = Lxx + diag(2 w act), lx = Lxx e + barrier
    double e[N], lx[N], ldiag[N];
    {
      const long long row = (long long)roff + t < rlast ? (long long)roff + t : rlast;
      const float* r = rbase ? rbase + (long long)row * p.ref_ts : nullptr;
#pragma unroll
      for (int i = 0; i < N; ++i) e[i] = (double)xb[(long long)t * N + i] - (double)(r ? r[i] : p.x_target[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + p.Lxx[i * N + k] * e[k];
      const double x = (double)xb[(long long)t * N + i];
      bool act = false;
      if (p.has_x_min) {
        const double v = (double)p.x_min[i] - x;
        if (v > 0.0) {
          act = true;
          a = a - p.w2 * v;
        }
      }
      if (p.has_x_max) {
        const double v = x - (double)p.x_max[i];
        if (v > 0.0) {
          act = true;
          a = a + p.w2 * v;
        }
      }
      lx[i] = a;
      ldiag[i] = act ? p.Lxx[i * N + i] + p.w2 : p.Lxx[i * N + i];
    }
    if (t == p.H) {  // P_H = Lxx_H, p_H = lx_H
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) P[i][j] = i == j ? ldiag[i] : p.Lxx[i * N + j];
        pv[i] = lx[i];
      }
      if (p.term_W) terminal_init<N>(p, b, e, lx, P, pv);
      continue;
    }
    double A[N][N], Bt[N][MI];
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < N; ++j) A[i][j] = (double)Ab[(long long)t * (N * N) + i * N + j];
#pragma unroll
      for (int j = 0; j < MI; ++j) Bt[i][j] = (double)Bb[(long long)t * (N * MI) + i * MI + j];
    }
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
    double Qxx[N][N], Qux[MI][N], Quu[MI][MI], qx[N], qu[MI];
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) a = a + A[k][i] * S[k][j];
        Qxx[i][j] = (i == j ? ldiag[i] : p.Lxx[i * N + j]) + a;
      }
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + A[k][i] * pv[k];
      qx[i] = lx[i] + a;
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
        double q = p.Luu[i * MI + j] + a;
        if (i == j) q = q + mu;
        Quu[i][j] = q;
      }
      double lu = 0.0;  // lu_t = (R + R^T) u_t
#pragma unroll
      for (int k = 0; k < MI; ++k) lu = lu + p.Luu[i * MI + k] * (double)ub[(long long)t * MI + k];
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + Bt[k][i] * pv[k];
      qu[i] = lu + a;
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
    if (bad) break;
    // X = Quu^-1 Qux (columns 0 .. N-1) and d = Quu^-1 qu (column N) from the same factors
    double X[MI][N + 1];
#pragma unroll
    for (int c = 0; c <= N; ++c) {
      double y[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        double s = c < N ? Qux[i][c < N ? c : 0] : qu[i];
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
    // K_t = -X, k_t = -d
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int j = 0; j < N; ++j) scr[((long long)t * E + i * N + j) * p.B] = -X[i][j];
      scr[((long long)t * E + MI * N + i) * p.B] = -X[i][N];
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
    // p_t = qx - Qux^T d,  dV += qu . d
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < MI; ++k) a = a + Qux[k][i] * X[k][N];
      pv[i] = qx[i] - a;
    }
    {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < MI; ++k) a = a + qu[k] * X[k][N];
      dV = dV + a;
    }
  }
  // the first failure, going backwards, at step t: status = t + 1 (0: none), as k_tvlqr reports it
  p.status[b] = t + 1;
  bool ok = t < 0 && fabs(dV) < __builtin_inf();
  if (t < 0) {
    // forward on the linear model: dx_0 = 0, du_t = k_t + K_t dx_t, dx_{t+1} = A_t dx_t + B_t du_t
    double dx[N];
#pragma unroll
    for (int i = 0; i < N; ++i) dx[i] = 0.0;
    for (int s = 0; s < p.H; ++s) {
      double du[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) a = a + scr[((long long)s * E + i * N + j) * p.B] * dx[j];
        du[i] = scr[((long long)s * E + MI * N + i) * p.B] + a;
        const float f = (float)du[i];
        if (!finite(f)) ok = false;
        dub[(long long)s * MI + i] = f;
      }
      double nx[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) a = a + (double)Ab[(long long)s * (N * N) + i * N + j] * dx[j];
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < MI; ++k) c = c + (double)Bb[(long long)s * (N * MI) + i * MI + k] * du[k];
        nx[i] = a + c;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) dx[i] = nx[i];
    }
  }
  // a failed pivot, or a step or dV that is not finite: no step at all, never a finite wrong one
  if (!ok)
    for (int s = 0; s < p.H * MI; ++s) dub[s] = 0.f;
  p.dV[b] = ok ? dV : __builtin_nan("");
}

// ------------------------------------------------------------------------------------------------ k_gn_direction_box
// The box-constrained step (tests/gn_box_model.py): the TWIN of k_gn_direction -- everything up
// to d = Quu^-1 qu is formed exactly as there, and a step whose -d violates no bound continues exactly as there; a
// change to one of the two belongs in the other.  A step that violates a bound solves the box-QP by enumerating the
// 3^MI - 1 active sets in code order (digit i of the code: 0 free, 1 at lo, 2 at hi), each with the same L D L^T routine
// on Quu with the fixed rows and columns replaced by the identity, takes the first one that satisfies the bounds and
// the sign conditions of the multipliers, and updates the value function in its general form.  The code loop is a
// run-time loop (neighbouring problems diverge only on such steps); no array is indexed by a run-time value.
constexpr int pow3(int m) { return m <= 0 ? 1 : 3 * pow3(m - 1); }

template <int N, int MI>
__global__ __launch_bounds__(kDirThreads) void k_gn_direction_box(GnDirectionBoxParams q) {
  const GnDirectionParams& p = q.d;
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.B) return;
  constexpr int E = MI * N + MI;
  const float* Ab = p.A + b * p.H * (N * N);
  const float* Bb = p.Bm + b * p.H * (N * MI);
  const float* xb = p.traj + b * (p.H + 1) * N;
  const float* ub = p.u + b * p.H * MI;
  float* dub = p.du + b * p.H * MI;
  double* scr = p.scratch + b;
  const double mu = p.mu[b];
  const float* rbase = p.x_ref ? p.x_ref + b * p.ref_bs : nullptr;
  int roff = 0;
  const int rlast = p.ref_rows - 1;
  if (rbase) {
    const int o = p.ref_off_dev ? *p.ref_off_dev : p.ref_off_host;
    roff = o < 0 ? 0 : (o > rlast ? rlast : o);
  }

  double P[N][N], pv[N];
  double dV = 0.0;
  int nclamp = 0;
  int t = p.H;
  for (; t >= 0; --t) {
    double e[N], lx[N], ldiag[N];
    {
      const long long row = (long long)roff + t < rlast ? (long long)roff + t : rlast;
      const float* r = rbase ? rbase + (long long)row * p.ref_ts : nullptr;
#pragma unroll
      for (int i = 0; i < N; ++i) e[i] = (double)xb[(long long)t * N + i] - (double)(r ? r[i] : p.x_target[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + p.Lxx[i * N + k] * e[k];
      const double x = (double)xb[(long long)t * N + i];
      bool act = false;
      if (p.has_x_min) {
        const double v = (double)p.x_min[i] - x;
        if (v > 0.0) {
          act = true;
          a = a - p.w2 * v;
        }
      }
      if (p.has_x_max) {
        const double v = x - (double)p.x_max[i];
        if (v > 0.0) {
          act = true;
          a = a + p.w2 * v;
        }
      }
      lx[i] = a;
      ldiag[i] = act ? p.Lxx[i * N + i] + p.w2 : p.Lxx[i * N + i];
    }
    if (t == p.H) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) P[i][j] = i == j ? ldiag[i] : p.Lxx[i * N + j];
        pv[i] = lx[i];
      }
      if (p.term_W) terminal_init<N>(p, b, e, lx, P, pv);
      continue;
    }
    double A[N][N], Bt[N][MI];
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < N; ++j) A[i][j] = (double)Ab[(long long)t * (N * N) + i * N + j];
#pragma unroll
      for (int j = 0; j < MI; ++j) Bt[i][j] = (double)Bb[(long long)t * (N * MI) + i * MI + j];
    }
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
    double Qxx[N][N], Qux[MI][N], Quu[MI][MI], qx[N], qu[MI];
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
      for (int j = 0; j < N; ++j) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) a = a + A[k][i] * S[k][j];
        Qxx[i][j] = (i == j ? ldiag[i] : p.Lxx[i * N + j]) + a;
      }
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + A[k][i] * pv[k];
      qx[i] = lx[i] + a;
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
      for (int j = 0; j <= i; ++j) {  // lower triangle, mirrored so that Quu[i][j] reads either half
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) a = a + Bt[k][i] * T[k][j];
        double v = p.Luu[i * MI + j] + a;
        if (i == j) v = v + mu;
        Quu[i][j] = v;
        Quu[j][i] = v;
      }
      double lu = 0.0;
#pragma unroll
      for (int k = 0; k < MI; ++k) lu = lu + p.Luu[i * MI + k] * (double)ub[(long long)t * MI + k];
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) a = a + Bt[k][i] * pv[k];
      qu[i] = lu + a;
    }
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
    // the bounds of the step; a nominal outside them (a NaN control included) fails like a pivot
    double lo[MI], hi[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      if (q.has_u_bounds) {
        const double uu = (double)ub[(long long)t * MI + i];
        lo[i] = q.u_min - uu;
        hi[i] = q.u_max - uu;
      } else {
        lo[i] = -__builtin_inf();
        hi[i] = __builtin_inf();
      }
      if (!(lo[i] <= 0.0 && 0.0 <= hi[i])) bad = true;
    }
    if (bad) break;
    double X[MI][N + 1];
#pragma unroll
    for (int c = 0; c <= N; ++c) {
      double y[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        double s = c < N ? Qux[i][c < N ? c : 0] : qu[i];
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
    bool all_free = true;
#pragma unroll
    for (int i = 0; i < MI; ++i)
      if (-X[i][N] < lo[i] || -X[i][N] > hi[i]) all_free = false;
    if (all_free) {
      // k_gn_direction's step: K_t = -X, k_t = -d, P_t = Qxx - Qux^T X, p_t = qx - Qux^T d, dV += qu . d
#pragma unroll
      for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) scr[((long long)t * E + i * N + j) * p.B] = -X[i][j];
        scr[((long long)t * E + MI * N + i) * p.B] = -X[i][N];
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
      for (int i = 0; i < N; ++i) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < MI; ++k) a = a + Qux[k][i] * X[k][N];
        pv[i] = qx[i] - a;
      }
      {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < MI; ++k) a = a + qu[k] * X[k][N];
        dV = dV + a;
      }
    } else {
      // the box-QP: the first active set, in code order, that passes
      double x[MI];
      int dg[MI];
      bool found = false;
#pragma nounroll
      for (int c = 1; c < pow3(MI) && !found; ++c) {
        int cc = c;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          dg[i] = cc % 3;
          cc /= 3;
          x[i] = dg[i] == 1 ? lo[i] : (dg[i] == 2 ? hi[i] : 0.0);
        }
        double r[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          double s = qu[i];
#pragma unroll
          for (int j = 0; j < MI; ++j)
            if (dg[j] != 0) s = s + Quu[i][j] * x[j];
          r[i] = dg[i] == 0 ? s : 0.0;
        }
        bool badm = false;
#pragma unroll
        for (int j = 0; j < MI; ++j) {
          double w[MI];
          double d = dg[j] == 0 ? Quu[j][j] : 1.0;
#pragma unroll
          for (int k = 0; k < j; ++k) {
            w[k] = Lf[j][k] * D[k];
            d = d - Lf[j][k] * w[k];
          }
          D[j] = d;
          if (!(d > 0.0) || d == __builtin_inf()) badm = true;
#pragma unroll
          for (int i = j + 1; i < MI; ++i) {
            double s = dg[i] == 0 && dg[j] == 0 ? Quu[i][j] : 0.0;
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - Lf[i][k] * w[k];
            Lf[i][j] = s / d;
          }
        }
        if (badm) continue;
        {
          double y[MI], z[MI];
#pragma unroll
          for (int i = 0; i < MI; ++i) {
            double s = r[i];
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
            for (int k = i + 1; k < MI; ++k) s = s - Lf[k][i] * z[k];
            z[i] = s;
          }
#pragma unroll
          for (int i = 0; i < MI; ++i)
            if (dg[i] == 0) x[i] = -z[i];
        }
        bool ok = true;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          double g = qu[i];
#pragma unroll
          for (int j = 0; j < MI; ++j) g = g + Quu[i][j] * x[j];
          if (dg[i] == 0) {
            if (!(lo[i] <= x[i] && x[i] <= hi[i])) ok = false;
          } else if (dg[i] == 1) {
            if (!(g >= 0.0)) ok = false;
          } else {
            if (!(g <= 0.0)) ok = false;
          }
        }
        found = ok;
      }
      if (!found) break;
      // K_t: rows of the free components from the factors of the accepted set, zero rows for the fixed ones; k_t = x
      double Kt[MI][N];
#pragma unroll
      for (int c = 0; c < N; ++c) {
        double y[MI], z[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          double s = dg[i] == 0 ? Qux[i][c] : 0.0;
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
          for (int k = i + 1; k < MI; ++k) s = s - Lf[k][i] * z[k];
          z[i] = s;
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) Kt[i][c] = dg[i] == 0 ? -z[i] : 0.0;
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) scr[((long long)t * E + i * N + j) * p.B] = Kt[i][j];
        scr[((long long)t * E + MI * N + i) * p.B] = x[i];
        if (dg[i] != 0) nclamp = nclamp + 1;
      }
      // W = Quu K, w = Quu k; P_t = Qxx + K^T W + K^T Qux + Qux^T K; p_t = qx + K^T w + K^T qu + Qux^T k;
      // dV += -(2 qu . k + k . w)
      double W[MI][N], w[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          double a = 0.0;
#pragma unroll
          for (int k = 0; k < MI; ++k) a = a + Quu[i][k] * Kt[k][j];
          W[i][j] = a;
        }
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < MI; ++k) a = a + Quu[i][k] * x[k];
        w[i] = a;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
          double a = 0.0, c = 0.0, d = 0.0;
#pragma unroll
          for (int k = 0; k < MI; ++k) a = a + Kt[k][i] * W[k][j];
#pragma unroll
          for (int k = 0; k < MI; ++k) c = c + Kt[k][i] * Qux[k][j];
#pragma unroll
          for (int k = 0; k < MI; ++k) d = d + Qux[k][i] * Kt[k][j];
          S[i][j] = ((Qxx[i][j] + a) + c) + d;
        }
        double a = 0.0, c = 0.0, d = 0.0;
#pragma unroll
        for (int k = 0; k < MI; ++k) a = a + Kt[k][i] * w[k];
#pragma unroll
        for (int k = 0; k < MI; ++k) c = c + Kt[k][i] * qu[k];
#pragma unroll
        for (int k = 0; k < MI; ++k) d = d + Qux[k][i] * x[k];
        pv[i] = ((qx[i] + a) + c) + d;
      }
      {
        double a = 0.0, c = 0.0;
#pragma unroll
        for (int k = 0; k < MI; ++k) a = a + qu[k] * x[k];
#pragma unroll
        for (int k = 0; k < MI; ++k) c = c + x[k] * w[k];
        dV = dV + (-(2.0 * a + c));
      }
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i; j < N; ++j) {
        const double s = 0.5 * (S[i][j] + S[j][i]);
        P[i][j] = s;
        P[j][i] = s;
      }
  }
  p.status[b] = t + 1;
  bool ok = t < 0 && fabs(dV) < __builtin_inf();
  if (t < 0) {
    // forward on the linear model, every step clipped to the bounds of the step
    double dx[N];
#pragma unroll
    for (int i = 0; i < N; ++i) dx[i] = 0.0;
    for (int s = 0; s < p.H; ++s) {
      double du[MI];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) a = a + scr[((long long)s * E + i * N + j) * p.B] * dx[j];
        double v = scr[((long long)s * E + MI * N + i) * p.B] + a;
        if (q.has_u_bounds) {
          const double uu = (double)ub[(long long)s * MI + i];
          const double lo = q.u_min - uu, hi = q.u_max - uu;
          if (v < lo) v = lo;
          if (v > hi) v = hi;
        }
        du[i] = v;
        const float f = (float)v;
        if (!finite(f)) ok = false;
        dub[(long long)s * MI + i] = f;
      }
      double nx[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        double a = 0.0;
#pragma unroll
        for (int j = 0; j < N; ++j) a = a + (double)Ab[(long long)s * (N * N) + i * N + j] * dx[j];
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < MI; ++k) c = c + (double)Bb[(long long)s * (N * MI) + i * MI + k] * du[k];
        nx[i] = a + c;
      }
#pragma unroll
      for (int i = 0; i < N; ++i) dx[i] = nx[i];
    }
  }
  if (!ok)
    for (int s = 0; s < p.H * MI; ++s) dub[s] = 0.f;
  p.dV[b] = ok ? dV : __builtin_nan("");
  if (q.nclamp) q.nclamp[b] = ok ? nclamp : 0;
}

// ------------------------------------------------------------------------------------------------ k_gn_candidates
// One thread per element of the candidate tensor (consecutive threads, consecutive floats of a row); the first
// B * L * n threads also write the replicated x0, as k_sample does.
__global__ __launch_bounds__(kFlat) void k_gn_candidates(GnCandidatesParams p) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long rows = p.B * p.L;
  if (idx < rows * p.N) {
    const long long r = idx / p.N;
    const int e = (int)(idx - r * p.N);
    const long long b = r / p.L;
    const int j = (int)(r - b * p.L);
    const float alpha = __uint_as_float((unsigned)(127 - j) << 23);  // 2^-j, j < 32
    const float step = alpha * p.du[b * p.N + e];
    p.cand[idx] = clampf(p.u[b * p.N + e] + step, p.u_min, p.u_max, p.has_u_bounds);
  }
  if (p.x0_rep && idx < rows * p.n) {
    const long long r = idx / p.n;
    const int i = (int)(idx - r * p.n);
    p.x0_rep[idx] = p.x0[(r / p.L) * p.n + i];
  }
}

// ------------------------------------------------------------------------------------------------ k_gn_select
// One 64-thread workgroup per problem: every thread finds j* from the L costs (the same loads in every lane), the
// decision is taken before anything is written (barrier), then the threads copy the accepted rows side by side.
__global__ __launch_bounds__(64) void k_gn_select(GnSelectParams p) {
  const long long b = blockIdx.x;
  const float* s = p.cand_cost + b * p.L;
  int js = -1;
  float best = 0.f;
  for (int j = 0; j < p.L; ++j) {
    const float sj = s[j];
    if (finite(sj) && (js < 0 || sj < best)) {
      js = j;
      best = sj;
    }
  }
  const float cost = p.cost[b];
  const bool accept = p.status[b] == 0 && js >= 0 && best < cost;
  __syncthreads();  // every lane has read cost[b] before lane 0 replaces it
  if (threadIdx.x == 0) {
    if (p.costs_row) p.costs_row[b] = cost;
    if (p.alpha_row) p.alpha_row[b] = accept ? __uint_as_float((unsigned)(127 - js) << 23) : 0.f;
    const double mu = p.mu[b];
    if (accept) {
      const double v = mu * p.mu_down;
      p.mu[b] = v > p.mu_min ? v : p.mu_min;
      p.cost[b] = best;
      p.accepts[b] = p.accepts[b] + 1;
    } else {
      const double v = mu * p.mu_up;
      p.mu[b] = v < p.mu_max ? v : p.mu_max;
    }
  }
  if (!accept) return;
  const long long r = b * p.L + js;
  for (int e = threadIdx.x; e < p.N; e += blockDim.x) p.u[b * p.N + e] = p.cand[r * p.N + e];
  for (int e = threadIdx.x; e < p.T; e += blockDim.x) p.traj[b * p.T + e] = p.cand_traj[r * p.T + e];
}

__global__ __launch_bounds__(kFlat) void k_gn_state(double* mu, int* accepts, long long B, double mu_init) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    mu[b] = mu_init;
    accepts[b] = 0;
  }
}

template <int N, int MI>
hipError_t direction_launch(const GnDirectionParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.B + kDirThreads - 1) / kDirThreads);
  hipLaunchKernelGGL((k_gn_direction<N, MI>), dim3(grid), dim3(kDirThreads), 0, st, p);
  return hipGetLastError();
}

template <int N, int MI>
hipError_t direction_box_launch(const GnDirectionBoxParams& p, hipStream_t st) {
  const unsigned grid = (unsigned)((p.d.B + kDirThreads - 1) / kDirThreads);
  hipLaunchKernelGGL((k_gn_direction_box<N, MI>), dim3(grid), dim3(kDirThreads), 0, st, p);
  return hipGetLastError();
}

dim3 flat_grid(long long count) { return dim3((unsigned)((count + kFlat - 1) / kFlat)); }

}  // namespace

GnLayout gn_layout(long long B, int H, int n, int m, int L) {
  GnLayout l{};
  const size_t b = (size_t)B, h = (size_t)H, rows = b * (size_t)L, f = sizeof(float), d = sizeof(double);
  size_t off = 0;
  const auto region = [&off](size_t bytes) {
    const size_t at = off;
    off = align256(off + bytes);
    return at;
  };
  l.A = region(b * h * n * n * f);
  l.Bm = region(b * h * n * m * f);
  l.traj = region(b * (h + 1) * n * f);
  l.du = region(b * h * m * f);
  l.dV = region(b * d);
  l.status = region(b * sizeof(int));
  l.scratch = region(b * h * (size_t)(m * n + m) * d);
  l.cand = region(rows * h * m * f);
  l.x0_rep = region(rows * n * f);
  l.cand_cost = region(rows * f);
  l.cand_traj = region(rows * (h + 1) * n * f);
  l.total = off;
  return l;
}

hipError_t gn_direction_launch(int n, int m, const GnDirectionParams& p, hipStream_t st) {
  switch (n * 8 + m) {
#define PHNN_GN_CASE(N, MI) \
  case N * 8 + MI: return direction_launch<N, MI>(p, st);
#define PHNN_GN_ROW(N) PHNN_GN_CASE(N, 1) PHNN_GN_CASE(N, 2) PHNN_GN_CASE(N, 3) PHNN_GN_CASE(N, 4)
    PHNN_GN_ROW(2)
    PHNN_GN_ROW(3)
    PHNN_GN_ROW(4)
#undef PHNN_GN_ROW
#undef PHNN_GN_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t gn_direction_box_launch(int n, int m, const GnDirectionBoxParams& p, hipStream_t st) {
  switch (n * 8 + m) {
#define PHNN_GN_CASE(N, MI) \
  case N * 8 + MI: return direction_box_launch<N, MI>(p, st);
#define PHNN_GN_ROW(N) PHNN_GN_CASE(N, 1) PHNN_GN_CASE(N, 2) PHNN_GN_CASE(N, 3) PHNN_GN_CASE(N, 4)
    PHNN_GN_ROW(2)
    PHNN_GN_ROW(3)
    PHNN_GN_ROW(4)
#undef PHNN_GN_ROW
#undef PHNN_GN_CASE
    default: return hipErrorInvalidValue;
  }
}

hipError_t gn_candidates_launch(const GnCandidatesParams& p, hipStream_t st) {
  const long long rows = p.B * p.L;
  const long long count = rows * (p.N > p.n ? p.N : p.n);
  hipLaunchKernelGGL(k_gn_candidates, flat_grid(count), dim3(kFlat), 0, st, p);
  return hipGetLastError();
}

hipError_t gn_select_launch(const GnSelectParams& p, hipStream_t st) {
  hipLaunchKernelGGL(k_gn_select, dim3((unsigned)p.B), dim3(64), 0, st, p);
  return hipGetLastError();
}

hipError_t gn_state_launch(double* mu, int* accepts, long long B, double mu_init, hipStream_t st) {
  hipLaunchKernelGGL(k_gn_state, flat_grid(B), dim3(kFlat), 0, st, mu, accepts, B, mu_init);
  return hipGetLastError();
}
