"""The measurement update of the batched extended Kalman filter (phnn_ekf_update), stated operation
for operation (TEST INFRASTRUCTURE, in the style of tvlqr_model.py, whose `_dot` this file uses): float64, no fused
multiply-adds, every inner product with its index ascending from an accumulator 0.0, each product rounded, then added.
k_ekf_update (phnn_ekf.hip) follows this file and is pinned against it bit for bit (tests/test_gpu_ekf.py); `textbook` is
a second formulation (numpy.linalg, compact S, the standard covariance form) the stated order is checked against
(tests/test_ekf_model.py).

Vectorised over the batch only: every operation below acts on float64 arrays of shape (B,) element-wise, so each problem
sees exactly the scalar sequence written here.  n = N state components, `mask` bit i set = component i is measured.

  x_i = (double)xpred_i,  A = (double)A,  bad_in = any of them not finite
  M[i][j]  = sum_k A[i][k] P[k][j];   W[i][j] = (sum_k M[i][k] A[j][k]) + Qn[i][j];
  P-[i][j] = P-[j][i] = 0.5 (W[i][j] + W[j][i])                                  (i <= j)
  nu_i = (double)y_i - x_i where measured, else 0;  Rv_i = Rn_i where measured, else 0;  dropout = a measured y_i not finite
  S at its full size n with the rows and columns of the unmeasured components replaced by the identity, lower triangle:
      S[j][j] = P-[j][j] + Rv_j  (measured)  |  1;      S[i][j] = P-[i][j]  (both measured)  |  0        (i > j)
  S = L D L^T exactly as tvlqr_model factors Quu (w_k = L[j][k] D[k], d_j = S[j][j] - L[j][0] w_0 - ...,
      L[i][j] = (S[i][j] - L[i][0] w_0 - ...) / d_j); a pivot with not (d_j > 0), or d_j = +inf: bad
      -- every entry formed for an unmeasured component is an exact 0 or 1, the measured ones see the factorisation of the
      compact S = P-[idx, idx] + diag(Rn[idx]) in its order
  column c < n: rhs_i = P-[c][i] where i is measured, else 0;  column n: rhs = nu;  each solved as tvlqr_model solves a column
      (forward y_i = rhs_i - L[i][0] y_0 - ..., y_i = y_i / d_i, backward x_i = y_i - L[i+1][i] x_{i+1} - ...) -> X[.][c];
      K[i][a] = X[a][i],  z = X[.][n]
  xhat_i = (float)(x_i + sum_a K[i][a] nu_a)                                     (a = 0 .. n-1)
  G[i][j] = (i == j ? 1 : 0) - K[i][j];   V[i][j] = sum_k G[i][k] P-[k][j];
  Pn[i][j] = (sum_k V[i][k] G[j][k]) + (sum_a (K[i][a] Rv_a) K[j][a]);   P[i][j] = P[j][i] = 0.5 (Pn[i][j] + Pn[j][i])
  nis = sum_a nu_a z_a
  update = something is measured and not dropout;  fail = bad_in or (update and bad)
  fail:        xhat, P, nis = NaN, status 2
  not update:  xhat = xpred (the float), P = P-, nis = NaN, status 1 for a dropout, 0 when nothing is measured
  innov = nu in every case.
"""
import numpy as np
import torch

from linearize_model import LinOracleEngine
from tvlqr_model import _dot, same_floats  # noqa: F401  (same_floats: re-exported for the tests)


def mask_of(measured):
    return sum(1 << int(i) for i in measured)


def measured_of(mask, n):
    return [i for i in range(n) if (mask >> i) & 1]


def update(xpred, A, P, y, mask, Qn, Rn):
    """xpred (B,n) float32, A (B,n,n) float32, P (B,n,n) float64, y (B,n) float32 (unmeasured entries are not read),
    mask int, Qn (n,n) float64, Rn (n,) float64 (read where measured) ->
    dict(xhat (B,n) float32, P (B,n,n), nis (B), innov (B,n), status (B) int32, xhat64 (B,n))."""
    xpred = np.asarray(xpred, np.float32)
    nb, n = xpred.shape
    A = np.asarray(A, np.float32).reshape(nb, n, n).astype(np.float64)
    P = np.asarray(P, np.float64).reshape(nb, n, n)
    y = np.asarray(y, np.float32).reshape(nb, n)
    Qn = np.asarray(Qn, np.float64).reshape(n, n)
    Rn = np.asarray(Rn, np.float64).reshape(-1)
    meas = [bool((mask >> i) & 1) for i in range(n)]
    x = [xpred[:, i].astype(np.float64) for i in range(n)]
    At = [[A[:, i, j] for j in range(n)] for i in range(n)]
    Pi = [[P[:, i, j] for j in range(n)] for i in range(n)]
    zero = np.zeros(nb)
    bad_in = np.zeros(nb, bool)
    for i in range(n):
        bad_in |= ~np.isfinite(x[i])
        for j in range(n):
            bad_in |= ~np.isfinite(At[i][j])
    with np.errstate(all="ignore"):
        M = [[_dot((At[i][k], Pi[k][j]) for k in range(n)) for j in range(n)] for i in range(n)]
        W = [[_dot((M[i][k], At[j][k]) for k in range(n)) + Qn[i][j] for j in range(n)] for i in range(n)]
        Pm = [[None] * n for _ in range(n)]
        for i in range(n):
            for j in range(i, n):
                s = 0.5 * (W[i][j] + W[j][i])
                Pm[i][j] = s
                Pm[j][i] = s
        nu, Rv = [zero.copy() for _ in range(n)], [0.0] * n
        dropout = np.zeros(nb, bool)
        for i in range(n):
            if meas[i]:
                yi = y[:, i].astype(np.float64)
                dropout |= ~np.isfinite(yi)
                nu[i] = yi - x[i]
                Rv[i] = float(Rn[i])
        L = [[None] * n for _ in range(n)]
        D = [None] * n
        bad = np.zeros(nb, bool)
        for j in range(n):
            w = [None] * n
            d = (Pm[j][j] + Rv[j]) if meas[j] else np.ones(nb)
            for k in range(j):
                w[k] = L[j][k] * D[k]
                d = d - L[j][k] * w[k]
            D[j] = d
            bad |= ~(d > 0.0) | (d == np.inf)
            for i in range(j + 1, n):
                s = Pm[i][j] if (meas[i] and meas[j]) else zero.copy()
                for k in range(j):
                    s = s - L[i][k] * w[k]
                L[i][j] = s / d
        X = [[None] * (n + 1) for _ in range(n)]
        for c in range(n + 1):
            yv = [None] * n
            for i in range(n):
                s = nu[i] if c == n else (Pm[c][i] if meas[i] else zero.copy())
                for k in range(i):
                    s = s - L[i][k] * yv[k]
                yv[i] = s
            for i in range(n):
                yv[i] = yv[i] / D[i]
            for i in range(n - 1, -1, -1):
                s = yv[i]
                for k in range(i + 1, n):
                    s = s - L[k][i] * X[k][c]
                X[i][c] = s
        xh64 = [x[i] + _dot((X[k][i], nu[k]) for k in range(n)) for i in range(n)]
        xh = [v.astype(np.float32) for v in xh64]
        G = [[(1.0 if i == j else 0.0) - X[j][i] for j in range(n)] for i in range(n)]
        V = [[_dot((G[i][k], Pm[k][j]) for k in range(n)) for j in range(n)] for i in range(n)]
        Pn = [[_dot((V[i][k], G[j][k]) for k in range(n)) + _dot((X[k][i] * Rv[k], X[k][j]) for k in range(n))
               for j in range(n)] for i in range(n)]
        nis = _dot((nu[k], X[k][n]) for k in range(n))
    any_meas = any(meas)
    upd = np.full(nb, any_meas) & ~dropout
    fail = bad_in | (upd & bad)
    keep = ~fail & ~upd  # the prediction passes through
    out_x = np.empty((nb, n), np.float32)
    out_P = np.empty((nb, n, n))
    for i in range(n):
        out_x[:, i] = np.where(fail, np.float32(np.nan), np.where(keep, xpred[:, i], xh[i]))
        for j in range(i, n):
            s = 0.5 * (Pn[i][j] + Pn[j][i])
            s = np.where(fail, np.nan, np.where(keep, Pm[i][j], s))
            out_P[:, i, j] = s
            out_P[:, j, i] = s
    status = np.where(fail, 2, np.where(upd | (not any_meas), 0, 1)).astype(np.int32)
    return dict(xhat=out_x, P=out_P, nis=np.where(fail | keep, np.nan, nis), innov=np.stack(nu, axis=1), status=status,
                xhat64=np.stack(xh64, axis=1))  # xhat64: the updated state before its one rounding (of the update branch)


def textbook(xpred, A, P, y, mask, Qn, Rn):
    """The same step in its textbook form with numpy.linalg: compact S, inv, P = (I - K C) P- (another operation order,
    no failure handling) -> (xhat (B,n) float64, P (B,n,n), nis (B))."""
    xpred = np.asarray(xpred, np.float64)
    nb, n = xpred.shape
    A = np.asarray(A, np.float64).reshape(nb, n, n)
    idx = measured_of(mask, n)
    Cm = np.eye(n)[idx]
    R = np.diag(np.asarray(Rn, np.float64)[idx])
    Pm = A @ np.asarray(P, np.float64).reshape(nb, n, n) @ np.swapaxes(A, 1, 2) + np.asarray(Qn, np.float64)
    Si = np.linalg.inv(Cm @ Pm @ Cm.T + R)
    K = Pm @ Cm.T @ Si
    nu = (np.asarray(y, np.float64).reshape(nb, n) - xpred)[:, idx]
    xh = xpred + np.einsum("bia,ba->bi", K, nu)
    Pn = (np.eye(n) - K @ Cm) @ Pm
    nis = np.einsum("ba,bac,bc->b", nu, Si, nu)
    return xh, Pn, nis


def seeded_problem(seed, nb, n, mask):
    """Well-conditioned seeded inputs: A = I + 0.05 N(0,1) (float32), P = F F^T + 0.05 I with F = 0.2 N(0,1), Qn = a
    full SPD matrix of size ~1e-3, Rn in [0.01, 0.1], xpred = 0.5 N(0,1) and y = xpred + 0.2 N(0,1) (float32); the
    unmeasured entries of y are NaN (they are not read) -> dict(xpred, A, P, y, mask, Qn, Rn)."""
    rng = np.random.default_rng(seed)
    A = (np.eye(n) + 0.05 * rng.normal(size=(nb, n, n))).astype(np.float32)
    F = 0.2 * rng.normal(size=(nb, n, n))
    P = F @ np.swapaxes(F, 1, 2) + 0.05 * np.eye(n)
    P = 0.5 * (P + np.swapaxes(P, 1, 2))
    Fq = 0.03 * rng.normal(size=(n, n))
    Qn = Fq @ Fq.T + 1e-4 * np.eye(n)
    Qn = 0.5 * (Qn + Qn.T)
    Rn = rng.uniform(0.01, 0.1, size=n)
    xpred = (0.5 * rng.normal(size=(nb, n))).astype(np.float32)
    y = (xpred + 0.2 * rng.normal(size=(nb, n))).astype(np.float32)
    for i in range(n):
        if not (mask >> i) & 1:
            y[:, i] = np.nan
    return dict(xpred=xpred, A=A, P=np.ascontiguousarray(P), y=y, mask=mask, Qn=Qn, Rn=Rn)


def plant_cases(p, rng):
    """Mixes per-problem special cases into a seeded problem IN PLACE (where the batch is large enough): a dropped
    measurement, an indefinite S (a large negative P diagonal), a NaN prediction, an infinite Jacobian entry.  ->
    dict(case name -> problem index)."""
    nb, n = p["xpred"].shape
    idx = measured_of(p["mask"], n)
    where = {}
    slots = list(rng.permutation(nb))
    if idx and nb >= 5:
        b = where["dropout"] = int(slots.pop())
        p["y"][b, idx[-1]] = np.inf
        b = where["indefinite"] = int(slots.pop())
        p["P"][b] = np.diag(np.full(n, -50.0))
    if nb >= 5:
        b = where["nan_xpred"] = int(slots.pop())
        p["xpred"][b, n - 1] = np.nan
        b = where["inf_A"] = int(slots.pop())
        p["A"][b, 0, n - 1] = np.inf
    return where


MASKS = {2: {"single": 0b01, "all": 0b11, "empty": 0}, 3: {"single": 0b010, "all": 0b111, "pair02": 0b101, "empty": 0},
         4: {"single": 0b0100, "all": 0b1111, "pair02": 0b0101, "empty": 0}}


class EkfOracleEngine(LinOracleEngine):
    """LinOracleEngine with ekf_update served by this file (CPU tensors), so that estimation.EKF.step and the closed loop
    with an estimator run without a GPU."""

    def ekf_update(self, xpred, A, y, P, opt, xhat=None, nis=True, innov=True, status=None, log=None):
        self.calls.append("ekf_update")
        n = self.n
        Qn = np.array(opt.Qn[: n * n], np.float64).reshape(n, n)
        Rn = np.array(opt.Rn[:n], np.float64)
        r = update(np.asarray(xpred), np.asarray(A), np.asarray(P), np.asarray(y), int(opt.meas_mask), Qn, Rn)
        P.copy_(torch.from_numpy(r["P"]))
        return dict(xhat=torch.from_numpy(r["xhat"]), P=P, nis=torch.from_numpy(r["nis"]), innov=torch.from_numpy(r["innov"]),
                    status=torch.from_numpy(r["status"]))


# ----------------------------------------------------------------------------- filter consistency
def consistency_system(seed, n, mask, nb=64, T=200, rho=0.98):
    """A seeded linear-Gaussian system x+ = F x + w, y = x[idx] + v with spectral radius rho, w ~ N(0, Qn), v ~ N(0,
    diag(Rn)), x0 = 0, and the filter's start xhat0 ~ N(x0, P0) -> dict(F float32-exact (n,n), Qn, Rn, P0, xs (T+1,nb,n)
    true states, ys (T,nb,n) float32 measurements (NaN where unmeasured), xhat0 (nb,n) float32)."""
    rng = np.random.default_rng(seed)
    F = rng.normal(size=(n, n))
    F = (F * (rho / np.max(np.abs(np.linalg.eigvals(F))))).astype(np.float32).astype(np.float64)
    Fq = 0.1 * rng.normal(size=(n, n))
    Qn = Fq @ Fq.T + 0.01 * np.eye(n)
    Qn = 0.5 * (Qn + Qn.T)
    Rn = rng.uniform(0.02, 0.2, size=n)
    P0 = 0.5 * np.eye(n)
    idx = measured_of(mask, n)
    Lq = np.linalg.cholesky(Qn)
    xs = np.zeros((T + 1, nb, n))
    ys = np.full((T, nb, n), np.nan, np.float32)
    for t in range(T):
        xs[t + 1] = xs[t] @ F.T + rng.normal(size=(nb, n)) @ Lq.T
        v = rng.normal(size=(nb, n)) * np.sqrt(Rn)
        ys[t][:, idx] = (xs[t + 1] + v)[:, idx].astype(np.float32)
    xhat0 = (xs[0] + rng.normal(size=(nb, n)) * np.sqrt(0.5)).astype(np.float32)
    return dict(F=F, Qn=Qn, Rn=Rn, P0=P0, xs=xs, ys=ys, xhat0=xhat0, mask=mask, idx=idx)


def consistency_z(nis_sum, count, p):
    """The z score of the mean normalised innovation: sum of count chi-square(p) draws -> (mean / p - 1) / sqrt(2 / (p count))."""
    return (nis_sum / count / p - 1.0) / np.sqrt(2.0 / (p * count))
