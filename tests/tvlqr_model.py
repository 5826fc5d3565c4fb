"""The LQ backward pass of phnn_tvlqr, stated operation for operation (TEST INFRASTRUCTURE, in the style of
cem_model.py): float64, no fused multiply-adds, every inner product with its index ascending from an accumulator 0.0,
each product rounded, then added.  k_tvlqr (phnn_kernels.hip.h) follows this file and is pinned against it bit for bit
(tests/test_gpu_tvlqr.py); `riccati_reference` is a second formulation (numpy.linalg) the stated order is checked
against (tests/test_tvlqr_model.py).

The recursion is vectorised over the batch only: every arithmetic operation below acts on float64 arrays of shape (B,)
element-wise, so each problem sees exactly the scalar sequence written here (numpy fuses nothing).

  Lxx[i][j] = (double)Q[i][j] + (double)Q[j][i],  Luu likewise from R,  P_H = Lxx
  t = H-1 .. 0:   S = P A,  T = P B,  Qxx = Lxx + A^T S,  Qux = B^T S,  Quu = Luu + B^T T (+ mu on the diagonal, added
                  last), lower triangle only
                  Quu = L D L^T:  for j: w_k = L[j][k] D[k], d_j = Quu[j][j] - L[j][0] w_0 - L[j][1] w_1 ...,
                                  L[i][j] = (Quu[i][j] - L[i][0] w_0 - ...) / d_j      (i > j)
                  a pivot with not (d_j > 0), or d_j = +inf: failure at step t
                  per column c of Qux: forward  y_i = Qux[i][c] - L[i][0] y_0 - ...;  y_i = y_i / d_i;
                                       backward x_i = y_i - L[i+1][i] x_{i+1} - L[i+2][i] x_{i+2} ... (k ascending)
                  K_t = -X,  P_t = Qxx - Qux^T X,  then P[i][j] = P[j][i] = 0.5 (P[i][j] + P[j][i])
On the first failure, going backwards, at step t: K_s and P_s for s <= t (P0 included) are NaN, status = t + 1, later
steps keep their values; else status = 0.
"""
import numpy as np


def _dot(terms):
    """acc = 0.0; acc = acc + a * b for the (a, b) pairs in order (each product rounded, then added)."""
    acc = None
    for a, b in terms:
        p = a * b
        acc = (0.0 + p) if acc is None else (acc + p)
    return acc


def cost_matrices(Q, R, n, m):
    """(Lxx (n,n), Luu (m,m)) in float64 from float32 row-major Q (n x n leading entries) and R (m x m)."""
    Q = np.asarray(Q, np.float32).reshape(-1)[: n * n].reshape(n, n).astype(np.float64)
    R = np.asarray(R, np.float32).reshape(-1)[: m * m].reshape(m, m).astype(np.float64)
    return Q + Q.T, R + R.T


def cost_matrices_of(cost, n, m):
    """The same from a _capi.Cost."""
    return cost_matrices(np.ctypeslib.as_array(cost.Q), np.ctypeslib.as_array(cost.R), n, m)


def tvlqr(A, Bm, Lxx, Luu, mu=0.0):
    """A (B,H,n,n), Bm (B,H,n,m) float32; Lxx (n,n), Luu (m,m) float64 -> dict(K (B,H,m,n), P0 (B,n,n), P (B,H+1,n,n),
    status (B) int32), float64."""
    A = np.asarray(A, np.float32).astype(np.float64)
    Bm = np.asarray(Bm, np.float32).astype(np.float64)
    nb, H, n, _ = A.shape
    m = Bm.shape[3]
    mu = float(mu)
    K = np.full((nb, H, m, n), np.nan)
    Pall = np.full((nb, H + 1, n, n), np.nan)
    status = np.zeros(nb, np.int32)
    alive = np.ones(nb, bool)
    P = [[np.full(nb, Lxx[i][j]) for j in range(n)] for i in range(n)]
    for i in range(n):
        for j in range(n):
            Pall[:, H, i, j] = P[i][j]
    with np.errstate(all="ignore"):
        for t in range(H - 1, -1, -1):
            At = [[A[:, t, i, j] for j in range(n)] for i in range(n)]
            Bt = [[Bm[:, t, i, j] for j in range(m)] for i in range(n)]
            S = [[_dot((P[i][k], At[k][j]) for k in range(n)) for j in range(n)] for i in range(n)]
            T = [[_dot((P[i][k], Bt[k][j]) for k in range(n)) for j in range(m)] for i in range(n)]
            Qxx = [[Lxx[i][j] + _dot((At[k][i], S[k][j]) for k in range(n)) for j in range(n)] for i in range(n)]
            Qux = [[_dot((Bt[k][i], S[k][j]) for k in range(n)) for j in range(n)] for i in range(m)]
            Quu = [[None] * m for _ in range(m)]
            for i in range(m):
                for j in range(i + 1):
                    q = Luu[i][j] + _dot((Bt[k][i], T[k][j]) for k in range(n))
                    if i == j:
                        q = q + mu
                    Quu[i][j] = q
            L = [[None] * m for _ in range(m)]
            D = [None] * m
            bad = np.zeros(nb, bool)
            for j in range(m):
                w = [None] * m
                d = Quu[j][j]
                for k in range(j):
                    w[k] = L[j][k] * D[k]
                    d = d - L[j][k] * w[k]
                D[j] = d
                bad |= ~(d > 0.0) | (d == np.inf)
                for i in range(j + 1, m):
                    s = Quu[i][j]
                    for k in range(j):
                        s = s - L[i][k] * w[k]
                    L[i][j] = s / d
            failed = alive & bad
            status[failed] = t + 1
            alive &= ~bad
            X = [[None] * n for _ in range(m)]
            for c in range(n):
                y = [None] * m
                for i in range(m):
                    s = Qux[i][c]
                    for k in range(i):
                        s = s - L[i][k] * y[k]
                    y[i] = s
                for i in range(m):
                    y[i] = y[i] / D[i]
                for i in range(m - 1, -1, -1):
                    s = y[i]
                    for k in range(i + 1, m):
                        s = s - L[k][i] * X[k][c]
                    X[i][c] = s
            Pn = [[Qxx[i][j] - _dot((Qux[k][i], X[k][j]) for k in range(m)) for j in range(n)] for i in range(n)]
            for i in range(n):
                for j in range(i, n):
                    s = 0.5 * (Pn[i][j] + Pn[j][i])
                    P[i][j] = s
                    P[j][i] = s
            for i in range(m):
                for j in range(n):
                    K[alive, t, i, j] = (-X[i][j])[alive]
            for i in range(n):
                for j in range(n):
                    Pall[alive, t, i, j] = P[i][j][alive]
    return dict(K=K, P0=Pall[:, 0].copy(), P=Pall, status=status)


def riccati_reference(A, Bm, Lxx, Luu, mu=0.0):
    """The same recursion in its textbook form with numpy.linalg (another operation order, LU instead of LDL^T, no
    failure handling): -> (K (B,H,m,n), P0 (B,n,n))."""
    A = np.asarray(A, np.float64)
    Bm = np.asarray(Bm, np.float64)
    nb, H, n, _ = A.shape
    m = Bm.shape[3]
    K = np.empty((nb, H, m, n))
    P0 = np.empty((nb, n, n))
    for b in range(nb):
        P = np.array(Lxx, np.float64)
        for t in range(H - 1, -1, -1):
            At, Bt = A[b, t], Bm[b, t]
            Quu = Luu + Bt.T @ P @ Bt + mu * np.eye(m)
            Qux = Bt.T @ P @ At
            X = np.linalg.solve(Quu, Qux)
            K[b, t] = -X
            P = Lxx + At.T @ P @ At - Qux.T @ X
            P = 0.5 * (P + P.T)
        P0[b] = P
    return K, P0


def seeded_problem(seed, nb, H, n, m):
    """The well-conditioned seeded inputs of the CPU and GPU tests: A = I + 0.02 N(0,1), B = 0.02 N(0,1) (float32),
    Q = diag in [0.1, 10], R = diag in [0.01, 1] (float32) -> (A, Bm, Q, R)."""
    rng = np.random.default_rng(seed)
    A = (np.eye(n) + 0.02 * rng.normal(size=(nb, H, n, n))).astype(np.float32)
    Bm = (0.02 * rng.normal(size=(nb, H, n, m))).astype(np.float32)
    Q = np.diag(rng.uniform(0.1, 10.0, size=n)).astype(np.float32)
    R = np.diag(rng.uniform(0.01, 1.0, size=m)).astype(np.float32)
    return A, Bm, Q, R


def same_floats(a, b):
    """a == b as floats: -0 == +0, NaN at the same positions."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
