"""The box-constrained LQ step of the Gauss-Newton solve (phnn_gn_direction_box), stated operation
for operation (TEST INFRASTRUCTURE, as gn_model.py is for the plain step): control-limited DDP (Tassa, Mansard, Todorov
2014) on the Gauss-Newton model.  k_gn_direction_box follows this file and is pinned against it bit for bit.  Float64,
no fused multiply-adds, every inner product with its index ascending from an accumulator 0.0, each product rounded, then
added.  One problem at a time in scalar float64 (the active sets differ between problems).

Step t of the backward sweep (t = H-1 .. 0), per problem:
  lx, lu, Lxx_t, S, T, Qxx, Qux, Quu = Luu + B^T T + mu I (lower triangle), its L D L^T, qx and qu: gn_model.direction_core's,
  operation for operation; a pivot with not (d > 0), or +inf: status = t + 1.
  bounds of the step: lo_i = (double)u_min - (double)u_t,i, hi_i = (double)u_max - (double)u_t,i; without has_u_bounds
  -inf / +inf (not computed from u).  not (lo_i <= 0 and 0 <= hi_i) in a component -- an infeasible nominal, a NaN control
  with bounds -- fails like a bad pivot: status = t + 1.
  d = Quu^-1 qu by the column solve (column n of X).  ALL-FREE: no component with -d_i < lo_i or -d_i > hi_i (a NaN d
  violates nothing: it takes this path and fails as in gn_model, status 0).  Then the step is gn_model's: K = -X, k = -d,
  P = Qxx - Qux^T X, p = qx - Qux^T d, dV += qu^T d.
  Otherwise the box-QP  min 1/2 x^T Quu x + qu^T x,  lo <= x <= hi  by enumeration of the active sets: codes
  c = 1 .. 3^m - 1, digit_i = (c // 3^i) % 3: 0 free, 1 at lo_i, 2 at hi_i (c = 0, all free, is the d above).  For a code:
    x_i = lo_i | hi_i for the fixed components;
    r_i = qu_i, then for j ascending over the FIXED j: r_i = r_i + Quu(i,j) x_j   (free i; r_i = 0.0 for a fixed i;
          Quu(i,j) reads the lower triangle);
    M = Quu on the free block, and for a fixed i: M_ii = 1.0, M_ij = M_ji = 0.0 -- the same L D L^T routine on M (the
          exact zeros and ones make the free block's factors those of the sub-matrix); a bad pivot rejects the code;
    y = M^-1 r by the column solve, x_i = -y_i for the free components;
    the code passes when lo_i <= x_i <= hi_i for every free i and, with g_i = qu_i then for j ascending over ALL j:
          g_i = g_i + Quu(i,j) x_j,  g_i >= 0 for every i at lo and g_i <= 0 for every i at hi.
  The first code that passes is taken; if none passes (borderline rounding) the step fails like a bad pivot.
  With the code taken: k = x;  X' = M^-1 Qux' column by column (Qux' = Qux with the fixed rows 0.0), K_i = -X'_i for a free
  i and +0.0 for a fixed one;  W = Quu K (W_ij = sum_l Quu(i,l) K_lj), w = Quu k;
    P_ij = ((Qxx_ij + sum_l K_li W_lj) + sum_l K_li Qux_lj) + sum_l Qux_li K_lj, then symmetrised as before;
    p_i  = ((qx_i + sum_l K_li w_l) + sum_l K_li qu_l) + sum_l Qux_li k_l;
    dV   = dV + (-(2.0 * (sum_l qu_l k_l) + sum_l k_l w_l));     nclamp += the number of fixed components.
forward:  dx = 0;  t = 0 .. H-1:  v_i = k_i + sum_j K_ij dx_j; if v_i < lo_i: v_i = lo_i; if v_i > hi_i: v_i = hi_i (lo, hi
  as above; a NaN passes);  du_t,i = v_i (float32 output: rounded once);  dx <- A dx + B du as in gn_model.
Where status != 0, or dV or a float32 du is not finite: du = 0, dV = NaN, nclamp = 0.

The predicted change of the model at the full step is -dV/2 as in gn_model; sum(grad_u * du) = -dV does NOT hold once a
component is clamped (dV then contains the curvature term k^T Quu k that no longer cancels half of qu^T k).
"""
import numpy as np
import torch

import gn_model as gm
import tvlqr_model as tm
from tvlqr_model import _dot

INF = np.float64(np.inf)
ZERO, ONE = np.float64(0.0), np.float64(1.0)


def _ldl(M, m):
    """The L D L^T routine of tvlqr_model on the lower triangle M -> (L, D, bad)."""
    L = [[None] * m for _ in range(m)]
    D = [None] * m
    bad = False
    for j in range(m):
        w = [None] * m
        d = M[j][j]
        for k in range(j):
            w[k] = L[j][k] * D[k]
            d = d - L[j][k] * w[k]
        D[j] = d
        bad = bad or (not (d > 0.0)) or d == INF
        for i in range(j + 1, m):
            s = M[i][j]
            for k in range(j):
                s = s - L[i][k] * w[k]
            L[i][j] = s / d
    return L, D, bad


def _solve(L, D, rhs, m):
    """The column solve of tvlqr_model: forward, divide, backward."""
    y = [None] * m
    for i in range(m):
        s = rhs[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    for i in range(m):
        y[i] = y[i] / D[i]
    x = [None] * m
    for i in range(m - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, m):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x


def _sym(Q, i, j):
    return Q[i][j] if i >= j else Q[j][i]


def all_free(d, lo, hi, m):
    return not any((-d[i] < lo[i]) or (-d[i] > hi[i]) for i in range(m))


def enumerate_box_qp(Q, q, lo, hi, m):
    """The enumeration (codes 1 .. 3^m - 1) on the lower triangle Q -> (x, digits, L, D) of the first code that passes, or
    None."""
    for c in range(1, 3 ** m):
        dg = [(c // 3 ** i) % 3 for i in range(m)]
        x = [lo[i] if dg[i] == 1 else (hi[i] if dg[i] == 2 else ZERO) for i in range(m)]
        r = [ZERO] * m
        for i in range(m):
            if dg[i] == 0:
                s = q[i]
                for j in range(m):
                    if dg[j] != 0:
                        s = s + _sym(Q, i, j) * x[j]
                r[i] = s
        M = [[(Q[i][j] if dg[i] == 0 and dg[j] == 0 else (ONE if i == j else ZERO)) for j in range(i + 1)] for i in range(m)]
        L, D, bad = _ldl(M, m)
        if bad:
            continue
        y = _solve(L, D, r, m)
        for i in range(m):
            if dg[i] == 0:
                x[i] = -y[i]
        ok = True
        for i in range(m):
            if dg[i] == 0:
                ok = ok and bool(lo[i] <= x[i]) and bool(x[i] <= hi[i])
            else:
                g = q[i]
                for j in range(m):
                    g = g + _sym(Q, i, j) * x[j]
                ok = ok and (bool(g >= 0.0) if dg[i] == 1 else bool(g <= 0.0))
        if ok:
            return x, dg, L, D
    return None


def box_qp(Q, q, lo, hi):
    """min 1/2 x^T Q x + q^T x over lo <= x <= hi as the step does it (Q (m,m) symmetric, float64) ->
    dict(x (m) or None on failure, digits, free: the all-free path was taken, bad: the pivot rule failed)."""
    with np.errstate(all="ignore"):
        m = len(q)
        Ql = [[np.float64(Q[i][j]) for j in range(i + 1)] for i in range(m)]
        q, lo, hi = ([np.float64(v) for v in a] for a in (q, lo, hi))
        L, D, bad = _ldl(Ql, m)
        if bad:
            return dict(x=None, digits=None, free=False, bad=True)
        d = _solve(L, D, q, m)
        if all_free(d, lo, hi, m):
            return dict(x=np.array([-v for v in d]), digits=[0] * m, free=True, bad=False)
        r = enumerate_box_qp(Ql, q, lo, hi, m)
        if r is None:
            return dict(x=None, digits=None, free=False, bad=False)
        return dict(x=np.array(r[0]), digits=r[1], free=False, bad=False)


def step_bounds(u, cost):
    """u (B,H,m) float32 -> (lo, hi) (B,H,m) float64 of the step."""
    u64 = np.asarray(u, np.float32).astype(np.float64)
    if not cost.has_u_bounds:
        return np.full(u64.shape, -np.inf), np.full(u64.shape, np.inf)
    with np.errstate(all="ignore"):
        return np.float64(np.float32(cost.u_min)) - u64, np.float64(np.float32(cost.u_max)) - u64


def direction_box_core(A, Bm, Lxx, Luu, ldiag, lx, lu, mu, lo, hi):
    """gn_model.direction_core's arguments and lo, hi (B,H,m) float64 -> its dict plus nclamp (B) int32, clamped (B,H)
    int32, the fixed components of every backward step (kept on failure), and clipped (B,H) int32, the components the
    forward sweep moved onto a bound -- the last two for the tests' input conditions."""
    A = np.asarray(A, np.float32).astype(np.float64)
    Bm = np.asarray(Bm, np.float32).astype(np.float64)
    nb, H, n, _ = A.shape
    m = Bm.shape[3]
    mu = np.broadcast_to(np.asarray(mu, np.float64), (nb,))
    Lxx, Luu = np.asarray(Lxx, np.float64), np.asarray(Luu, np.float64)
    lo, hi = np.asarray(lo, np.float64).reshape(nb, H, m), np.asarray(hi, np.float64).reshape(nb, H, m)
    K = np.full((nb, H, m, n), np.nan)
    kk = np.full((nb, H, m), np.nan)
    Pall = np.full((nb, H + 1, n, n), np.nan)
    status = np.zeros(nb, np.int32)
    nclamp = np.zeros(nb, np.int32)
    clamped = np.zeros((nb, H), np.int32)
    clipped = np.zeros((nb, H), np.int32)
    dVs = np.zeros(nb)
    du64 = np.zeros((nb, H, m))
    du32 = np.zeros((nb, H, m), np.float32)
    rn, rm = range(n), range(m)
    with np.errstate(all="ignore"):
        for b in range(nb):
            def lxx_t(t, i, j):
                return ldiag[b, t, i] if i == j else Lxx[i][j]

            P = [[lxx_t(H, i, j) for j in rn] for i in rn]
            pv = [lx[b, H, i] for i in rn]
            Pall[b, H] = P
            dV = ZERO
            for t in range(H - 1, -1, -1):
                At = [[A[b, t, i, j] for j in rn] for i in rn]
                Bt = [[Bm[b, t, i, j] for j in rm] for i in rn]
                S = [[_dot((P[i][k], At[k][j]) for k in rn) for j in rn] for i in rn]
                T = [[_dot((P[i][k], Bt[k][j]) for k in rn) for j in rm] for i in rn]
                Qxx = [[lxx_t(t, i, j) + _dot((At[k][i], S[k][j]) for k in rn) for j in rn] for i in rn]
                qx = [lx[b, t, i] + _dot((At[k][i], pv[k]) for k in rn) for i in rn]
                Qux = [[_dot((Bt[k][i], S[k][j]) for k in rn) for j in rn] for i in rm]
                Quu = [[None] * m for _ in rm]
                for i in rm:
                    for j in range(i + 1):
                        q = Luu[i][j] + _dot((Bt[k][i], T[k][j]) for k in rn)
                        if i == j:
                            q = q + mu[b]
                        Quu[i][j] = q
                qu = [lu[b, t, i] + _dot((Bt[k][i], pv[k]) for k in rn) for i in rm]
                L, D, bad = _ldl(Quu, m)
                l, h = [lo[b, t, i] for i in rm], [hi[b, t, i] for i in rm]
                bad = bad or any(not (l[i] <= 0.0 and 0.0 <= h[i]) for i in rm)
                if bad:
                    status[b] = t + 1
                    break
                X = [[None] * (n + 1) for _ in rm]
                for c in range(n + 1):
                    col = _solve(L, D, [Qux[i][c] if c < n else qu[i] for i in rm], m)
                    for i in rm:
                        X[i][c] = col[i]
                if all_free([X[i][n] for i in rm], l, h, m):
                    Pn = [[Qxx[i][j] - _dot((Qux[k][i], X[k][j]) for k in rm) for j in rn] for i in rn]
                    pv = [qx[i] - _dot((Qux[k][i], X[k][n]) for k in rm) for i in rn]
                    dV = dV + _dot((qu[k], X[k][n]) for k in rm)
                    Kt = [[-X[i][j] for j in rn] for i in rm]
                    kt = [-X[i][n] for i in rm]
                else:
                    r = enumerate_box_qp(Quu, qu, l, h, m)
                    if r is None:
                        status[b] = t + 1
                        break
                    kt, dg, L, D = r
                    Kt = [[None] * n for _ in rm]
                    for c in rn:
                        col = _solve(L, D, [Qux[i][c] if dg[i] == 0 else ZERO for i in rm], m)
                        for i in rm:
                            Kt[i][c] = -col[i] if dg[i] == 0 else ZERO
                    W = [[_dot((_sym(Quu, i, k), Kt[k][j]) for k in rm) for j in rn] for i in rm]
                    w = [_dot((_sym(Quu, i, k), kt[k]) for k in rm) for i in rm]
                    Pn = [[((Qxx[i][j] + _dot((Kt[k][i], W[k][j]) for k in rm)) + _dot((Kt[k][i], Qux[k][j]) for k in rm))
                           + _dot((Qux[k][i], Kt[k][j]) for k in rm) for j in rn] for i in rn]
                    pv = [((qx[i] + _dot((Kt[k][i], w[k]) for k in rm)) + _dot((Kt[k][i], qu[k]) for k in rm))
                          + _dot((Qux[k][i], kt[k]) for k in rm) for i in rn]
                    dV = dV + (-(2.0 * _dot((qu[k], kt[k]) for k in rm) + _dot((kt[k], w[k]) for k in rm)))
                    clamped[b, t] = sum(1 for v in dg if v != 0)
                for i in rn:
                    for j in range(i, n):
                        s = 0.5 * (Pn[i][j] + Pn[j][i])
                        P[i][j] = s
                        P[j][i] = s
                K[b, t], kk[b, t], Pall[b, t] = Kt, kt, P
            dVs[b] = dV
            if status[b] != 0:
                continue
            nclamp[b] = clamped[b].sum()
            dx = [ZERO] * n
            for t in range(H):
                du = [None] * m
                for i in rm:
                    v = kk[b, t, i] + _dot((K[b, t, i, j], dx[j]) for j in rn)
                    if v < lo[b, t, i]:
                        v = lo[b, t, i]
                        clipped[b, t] += 1
                    if v > hi[b, t, i]:
                        v = hi[b, t, i]
                        clipped[b, t] += 1
                    du[i] = v
                    du64[b, t, i] = v
                    du32[b, t, i] = np.float32(v)
                dx = [_dot((A[b, t, i, j], dx[j]) for j in rn) + _dot((Bm[b, t, i, k], du[k]) for k in rm) for i in rn]
    ok = (status == 0) & np.isfinite(dVs) & np.isfinite(du32).all(axis=(1, 2))
    du32[~ok] = 0.0
    du64[~ok] = 0.0
    nclamp[~ok] = 0
    return dict(du=du32, du64=du64, dV=np.where(ok, dVs, np.nan), status=status, nclamp=nclamp, clamped=clamped, clipped=clipped,
                K=K, k=kk, P=Pall)


def direction_box(A, Bm, traj, u, cost, n, m, mu, ref=None):
    """k_gn_direction_box on the device's float32 A, Bm, traj, u; ref as in gn_model.direction."""
    Lxx, Luu = tm.cost_matrices_of(cost, n, m)
    ldiag, lx, lu = gm.gradients(traj, u, cost, n, m, ref)
    lo, hi = step_bounds(np.asarray(u, np.float32).reshape(lu.shape), cost)
    return direction_box_core(A, Bm, Lxx, Luu, ldiag, lx, lu, mu, lo, hi)


class GnBoxOracleEngine(gm.GnOracleEngine):
    """GnOracleEngine whose gn_direction takes box=True (the step of this file, with nclamp in the result)."""

    def gn_direction(self, A, Bm, traj, u, cost, mu, x_ref=None, ref_offset=0, box=False):
        if not box:
            return super().gn_direction(A, Bm, traj, u, cost, mu, x_ref=x_ref, ref_offset=ref_offset)
        self.calls.append("gn_direction")
        traj = np.asarray(traj)
        nb, H = traj.shape[0], traj.shape[1] - 1
        ref = None if x_ref is None else gm.reference_rows(np.asarray(x_ref), ref_offset, H, nb, self.n)
        r = direction_box(np.asarray(A), np.asarray(Bm), traj, np.asarray(u), cost, self.n, self.m, np.asarray(mu), ref)
        return {k: torch.from_numpy(r[k]) for k in ("du", "dV", "status", "nclamp")}


# the initial states of the convergence table: convergence_case()'s five and four hard ones
HARD_X0 = np.array([[0.0, 0.3, 0.0, 0.0], [1.0, -0.3, 0.5, 1.0], [0.0, 0.45, 0.0, -1.0], [-2.0, 0.2, 1.0, 2.0]], np.float32)


def convergence_x0():
    return np.vstack([gm.convergence_case()[0], HARD_X0]).astype(np.float32)
