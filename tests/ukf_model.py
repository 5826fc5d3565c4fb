"""The two kernels of the batched unscented Kalman filter (phnn_ukf_sigma, phnn_ukf_moments), stated
operation for operation (TEST INFRASTRUCTURE, in the style of ekf_model.py): float64, no fused multiply-adds, every sum in
ascending index order, each product rounded, then added.  k_ukf_sigma and k_ukf_moments (phnn_ukf.hip) follow this file
and are pinned against it bit for bit (tests/test_gpu_ukf.py); `textbook_*` is a second formulation (numpy.linalg.cholesky,
matrix products) the stated order is checked against (tests/test_ukf_model.py).  The measurement update is
ekf_model.update with the identity as its Jacobian, imported unchanged.

Vectorised over the batch only: every operation acts on float64 arrays of shape (B,) element-wise, so each problem sees
exactly the scalar sequence written here.  n state components, S = 2 n + 1 sigma points.

  weights (host, float64): lambda = alpha^2 (n + kappa) - n, gamma = sqrt(n + lambda), wm0 = lambda / (n + lambda),
      wc0 = wm0 + (1 - alpha^2 + beta), wi = 1 / (2 (n + lambda))
  sigma:  x_i = (double)xhat_i;  P = L L^T by columns from the lower triangle of P:
      d_j = P[j][j] - L[j][0] L[j][0] - ... (ascending k),  L[j][j] = sqrt(d_j)  (numpy's sqrt is correctly rounded),
      L[i][j] = (P[i][j] - L[i][0] L[j][0] - ...) / L[j][j]  (i > j),  L[i][j] = 0  (i < j)
      fail = an xhat_i not finite, or a pivot with not (d_j > 0), or d_j = +inf
      chi_0 = xhat (its own bits),  g = gamma L[i][c],  chi_{1+c,i} = (float)(x_i + g),  chi_{1+n+c,i} = (float)(x_i - g)
      fail: every chi of the problem is NaN.   ctrl[b,k,0,:] = u[b,:] for every k, in every case.
  moments:  Y = (double)Y;  x-_i = ((0.0 + wm0 Y_0i) + wi Y_1i) + ... + wi Y_{S-1,i};  e_ki = Y_ki - x-_i
      Pm[i][j] = Pm[j][i] = ((0.0 + wc0 (e_0i e_0j)) + wi (e_1i e_1j)) + ...   (i <= j)
      xm_i = (float)x-_i;  eye = the float32 identity
"""
import numpy as np
import torch

import ekf_model as em


def weights(n, alpha=1.0, beta=0.0, kappa=1.0):
    """-> (gamma, wm0, wc0, wi), float64."""
    a2 = float(alpha) * float(alpha)
    lam = a2 * (n + float(kappa)) - n
    c = n + lam
    wm0 = lam / c
    return float(np.sqrt(c)), wm0, wm0 + (1.0 - a2 + float(beta)), 1.0 / (2.0 * c)


def sigma(xhat, P, gamma, u=None):
    """xhat (B,n) float32, P (B,n,n) float64 (lower triangle read), gamma float, u (B,m) float32 or None ->
    dict(chi (B,S,n) float32, ctrl (B,S,1,m) float32 or None, L (B,n,n) float64, fail (B) bool)."""
    xhat = np.asarray(xhat, np.float32)
    nb, n = xhat.shape
    S = 2 * n + 1
    P = np.asarray(P, np.float64).reshape(nb, n, n)
    x = [xhat[:, i].astype(np.float64) for i in range(n)]
    fail = np.zeros(nb, bool)
    for i in range(n):
        fail |= ~np.isfinite(x[i])
    L = [[np.zeros(nb) for _ in range(n)] for _ in range(n)]
    with np.errstate(all="ignore"):
        for j in range(n):
            d = P[:, j, j].copy()
            for k in range(j):
                d = d - L[j][k] * L[j][k]
            fail |= ~(d > 0.0) | (d == np.inf)
            r = np.sqrt(d)
            L[j][j] = r
            for i in range(j + 1, n):
                s = P[:, i, j].copy()
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                L[i][j] = s / r
        chi = np.empty((nb, S, n), np.float32)
        for i in range(n):
            chi[:, 0, i] = xhat[:, i]
            for c in range(n):
                g = gamma * L[i][c]
                chi[:, 1 + c, i] = (x[i] + g).astype(np.float32)
                chi[:, 1 + n + c, i] = (x[i] - g).astype(np.float32)
    chi[fail] = np.float32(np.nan)
    ctrl = None
    if u is not None:
        u = np.asarray(u, np.float32).reshape(nb, -1)
        ctrl = np.ascontiguousarray(np.broadcast_to(u[:, None, None, :], (nb, S, 1, u.shape[1])))
    Lm = np.stack([np.stack(row, axis=1) for row in L], axis=1)
    return dict(chi=chi, ctrl=ctrl, L=Lm, fail=fail)


def moments(Y, wm0, wc0, wi):
    """Y (B,S,n) float32 -> dict(xm (B,n) float32, xm64 (B,n), Pm (B,n,n) float64, eye (B,n,n) float32)."""
    Y = np.asarray(Y, np.float32)
    nb, S, n = Y.shape
    assert S == 2 * n + 1
    Yd = [[Y[:, k, i].astype(np.float64) for i in range(n)] for k in range(S)]
    with np.errstate(all="ignore"):
        xm = []
        for i in range(n):
            a = 0.0 + wm0 * Yd[0][i]
            for k in range(1, S):
                a = a + wi * Yd[k][i]
            xm.append(a)
        e = [[Yd[k][i] - xm[i] for i in range(n)] for k in range(S)]
        Pm = np.empty((nb, n, n))
        for i in range(n):
            for j in range(i, n):
                a = 0.0 + wc0 * (e[0][i] * e[0][j])
                for k in range(1, S):
                    a = a + wi * (e[k][i] * e[k][j])
                Pm[:, i, j] = a
                Pm[:, j, i] = a
    xm64 = np.stack(xm, axis=1)
    eye = np.ascontiguousarray(np.broadcast_to(np.eye(n, dtype=np.float32), (nb, n, n)))
    return dict(xm=xm64.astype(np.float32), xm64=xm64, Pm=Pm, eye=eye)


def step(xhat, P, propagate, y, mask, Qn, Rn, w):
    """One filter step: sigma, `propagate` ((B*S,n) float32 sigma points -> (B*S,n) float32 images), moments,
    ekf_model.update with the identity.  w = (gamma, wm0, wc0, wi).  -> ekf_model.update's dict plus chi, xm, Pm."""
    nb, n = np.asarray(xhat).shape
    sg = sigma(xhat, P, w[0])
    Y = np.asarray(propagate(sg["chi"].reshape(-1, n)), np.float32).reshape(nb, 2 * n + 1, n)
    mo = moments(Y, w[1], w[2], w[3])
    r = em.update(mo["xm"], mo["eye"], mo["Pm"], y, mask, Qn, Rn)
    r.update(chi=sg["chi"], xm=mo["xm"], Pm=mo["Pm"])
    return r


# ----------------------------------------------------------------------------- the textbook twin
def textbook_sigma(xhat, P, gamma):
    """numpy.linalg.cholesky and whole-matrix arithmetic -> (chi (B,S,n) float64, L (B,n,n))."""
    x = np.asarray(xhat, np.float64)
    L = np.linalg.cholesky(np.asarray(P, np.float64))
    cols = np.swapaxes(L, 1, 2)  # row c = column c of L
    return np.concatenate([x[:, None, :], x[:, None, :] + gamma * cols, x[:, None, :] - gamma * cols], axis=1), L


def textbook_moments(Y, wm0, wc0, wi):
    """Weighted mean and covariance as matrix products -> (xm (B,n) float64, Pm (B,n,n))."""
    Y = np.asarray(Y, np.float64)
    S = Y.shape[1]
    wm = np.full(S, wi)
    wc = wm.copy()
    wm[0], wc[0] = wm0, wc0
    xm = np.einsum("k,bki->bi", wm, Y)
    e = Y - xm[:, None, :]
    return xm, np.einsum("k,bki,bkj->bij", wc, e, e)


# ----------------------------------------------------------------------------- CPU stand-in of the engine
class UkfOracleEngine(em.EkfOracleEngine):
    """EkfOracleEngine with ukf_sigma and ukf_moments served by this file (CPU tensors), so that estimation.UKF.step and
    the closed loop with an unscented estimator run without a GPU."""

    def ukf_sigma(self, xhat, P, opt, u=None, u_stride=None, chi=None, ctrl=None):
        self.calls.append("ukf_sigma")
        r = sigma(np.asarray(xhat), np.asarray(P), float(opt.gamma), None if u is None else np.asarray(u))
        return torch.from_numpy(r["chi"]), (None if r["ctrl"] is None else torch.from_numpy(r["ctrl"]))

    def ukf_moments(self, Y, B, opt, Y_stride=None, xm=None, Pm=None, eye=True):
        self.calls.append("ukf_moments")
        n = self.n
        r = moments(np.asarray(Y).reshape(B, 2 * n + 1, n), float(opt.wm0), float(opt.wc0), float(opt.wi))
        return dict(xm=torch.from_numpy(r["xm"]), Pm=torch.from_numpy(r["Pm"]), eye=torch.from_numpy(r["eye"]))
