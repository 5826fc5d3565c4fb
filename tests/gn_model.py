"""The three kernels of the Gauss-Newton solve (phnn_solve_gn), stated operation for operation
(TEST INFRASTRUCTURE, in the style of tvlqr_model.py, whose `_dot` and recursion this file builds on):

  gradients / direction_core / direction   k_gn_direction: float64, no fused multiply-adds, every inner product with its
                                            index ascending from an accumulator 0.0, each product rounded, then added
  candidates                                k_gn_candidates: float32, the product rounded, then the sum, then the clamp
  select                                    k_gn_select
  GnOracleEngine                            LinOracleEngine + the three step methods, so that solver.gn_solve and the
                                            controllers run without a GPU

direction, per problem (vectorised over the batch only, as in tvlqr_model):
  t = H .. 0:  e = (double)x_t - (double)r_t;  per component i:  lx_i = sum_k Lxx[i][k] e_k;
               v = (double)x_min_i - x_i: if v > 0: lx_i = lx_i - w2 v;  v = x_i - (double)x_max_i: if v > 0: lx_i = lx_i + w2 v
               (w2 = 2 (double)barrier_weight; lower bound first);  Lxx_t = Lxx with Lxx[i][i] + w2 on the diagonal of the
               active components (the others keep their bits)
  P_H = Lxx_H, p_H = lx_H;  t = H-1 .. 0:  S, T, Qxx (with Lxx_t), Qux, Quu (+ mu last), L D L^T, X and the symmetrised
               P_t exactly as tvlqr_model states them;  lu_i = sum_k Luu[i][k] (double)u_t,k;
               qx_i = lx_i + sum_k A[k][i] p_k;  qu_i = lu_i + sum_k B[k][i] p_k;  d = Quu^-1 qu by the column solve of X;
               K_t = -X, k_t = -d;  p_i = qx_i - sum_k Qux[k][i] d_k;  dV = dV + sum_k qu_k d_k
  forward:     dx = 0;  t = 0 .. H-1:  du_i = k_i + sum_j K[i][j] dx_j  (float32 output: rounded once);
               dx_i <- (sum_j A[i][j] dx_j) + (sum_k B[i][k] du_k)
  status as tvlqr_model's.  Where status != 0, or dV or a float32 du is not finite: du = 0, dV = NaN.
"""
import numpy as np
import torch

import tvlqr_model as tm
import variant_census as vc
from linearize_model import LinOracleEngine
from tvlqr_model import _dot


def barrier_w2(cost):
    return 2.0 * float(np.float32(cost.barrier_weight))


def reference_rows(x_ref, offset, H, B, n):
    """x_ref broadcastable to (B, rows, n) -> the (B, H+1, n) float32 rows min(offset + t, rows - 1), offset clamped."""
    r = np.asarray(x_ref, np.float32)
    while r.ndim < 3:
        r = r[None]
    r = np.broadcast_to(r, (B, r.shape[1], n))
    last = r.shape[1] - 1
    off = min(max(int(offset), 0), last)
    return np.stack([r[:, min(off + t, last)] for t in range(H + 1)], axis=1)


def gradients(traj, u, cost, n, m, ref=None):
    """traj (B,H+1,n), u (B,H,m) float32; ref (B,H+1,n) float32 rows or None (the cost's x_target) ->
    (ldiag (B,H+1,n) the diagonal of Lxx_t, lx (B,H+1,n), lu (B,H,m)), float64."""
    Lxx, Luu = tm.cost_matrices_of(cost, n, m)
    x = np.asarray(traj, np.float32).astype(np.float64)
    nb, H1, _ = x.shape
    uu = np.asarray(u, np.float32).astype(np.float64).reshape(nb, H1 - 1, m)
    if ref is None:
        r = np.broadcast_to(np.ctypeslib.as_array(cost.x_target)[:n].astype(np.float32).astype(np.float64), x.shape)
    else:
        r = np.asarray(ref, np.float32).astype(np.float64)
    w2 = barrier_w2(cost)
    xmin = np.ctypeslib.as_array(cost.x_min).astype(np.float64)
    xmax = np.ctypeslib.as_array(cost.x_max).astype(np.float64)
    ldiag, lx, lu = np.empty_like(x), np.empty_like(x), np.empty_like(uu)
    with np.errstate(all="ignore"):
        e = x - r
        for i in range(n):
            a = _dot((Lxx[i][k], e[:, :, k]) for k in range(n))
            act = np.zeros(a.shape, bool)
            if cost.has_x_min:
                v = xmin[i] - x[:, :, i]
                a = np.where(v > 0.0, a - w2 * v, a)
                act |= v > 0.0
            if cost.has_x_max:
                v = x[:, :, i] - xmax[i]
                a = np.where(v > 0.0, a + w2 * v, a)
                act |= v > 0.0
            lx[:, :, i] = a
            ldiag[:, :, i] = np.where(act, Lxx[i][i] + w2, Lxx[i][i])
        for i in range(m):
            lu[:, :, i] = _dot((Luu[i][k], uu[:, :, k]) for k in range(m))
    return ldiag, lx, lu


def direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, mu):
    """A (B,H,n,n), Bm (B,H,n,m) float32; Lxx (n,n), Luu (m,m), ldiag (B,H+1,n), lx (B,H+1,n), lu (B,H,m) float64; mu (B)
    or one value -> dict(du (B,H,m) float32, du64, dV (B), status (B) int32, K (B,H,m,n), k (B,H,m), P (B,H+1,n,n))."""
    A = np.asarray(A, np.float32).astype(np.float64)
    Bm = np.asarray(Bm, np.float32).astype(np.float64)
    nb, H, n, _ = A.shape
    m = Bm.shape[3]
    mu = np.broadcast_to(np.asarray(mu, np.float64), (nb,))
    K = np.full((nb, H, m, n), np.nan)
    kk = np.full((nb, H, m), np.nan)
    Pall = np.full((nb, H + 1, n, n), np.nan)
    status = np.zeros(nb, np.int32)
    alive = np.ones(nb, bool)
    dV = np.zeros(nb)

    def lxx_t(t, i, j):
        return ldiag[:, t, i] if i == j else np.full(nb, Lxx[i][j])

    P = [[lxx_t(H, i, j) for j in range(n)] for i in range(n)]
    pv = [lx[:, H, i] for i in range(n)]
    for i in range(n):
        for j in range(n):
            Pall[:, H, i, j] = P[i][j]
    with np.errstate(all="ignore"):
        for t in range(H - 1, -1, -1):
            At = [[A[:, t, i, j] for j in range(n)] for i in range(n)]
            Bt = [[Bm[:, t, i, j] for j in range(m)] for i in range(n)]
            S = [[_dot((P[i][k], At[k][j]) for k in range(n)) for j in range(n)] for i in range(n)]
            T = [[_dot((P[i][k], Bt[k][j]) for k in range(n)) for j in range(m)] for i in range(n)]
            Qxx = [[lxx_t(t, i, j) + _dot((At[k][i], S[k][j]) for k in range(n)) for j in range(n)] for i in range(n)]
            qx = [lx[:, t, i] + _dot((At[k][i], pv[k]) for k in range(n)) for i in range(n)]
            Qux = [[_dot((Bt[k][i], S[k][j]) for k in range(n)) for j in range(n)] for i in range(m)]
            Quu = [[None] * m for _ in range(m)]
            for i in range(m):
                for j in range(i + 1):
                    q = Luu[i][j] + _dot((Bt[k][i], T[k][j]) for k in range(n))
                    if i == j:
                        q = q + mu
                    Quu[i][j] = q
            qu = [lu[:, t, i] + _dot((Bt[k][i], pv[k]) for k in range(n)) for i in range(m)]
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
            X = [[None] * (n + 1) for _ in range(m)]
            for c in range(n + 1):
                y = [None] * m
                for i in range(m):
                    s = Qux[i][c] if c < n else qu[i]
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
            pv = [qx[i] - _dot((Qux[k][i], X[k][n]) for k in range(m)) for i in range(n)]
            dV = dV + _dot((qu[k], X[k][n]) for k in range(m))
            for i in range(m):
                for j in range(n):
                    K[alive, t, i, j] = (-X[i][j])[alive]
                kk[alive, t, i] = (-X[i][n])[alive]
            for i in range(n):
                for j in range(n):
                    Pall[alive, t, i, j] = P[i][j][alive]
        # forward on the linear model
        du64 = np.zeros((nb, H, m))
        du32 = np.zeros((nb, H, m), np.float32)
        dx = [np.zeros(nb) for _ in range(n)]
        for t in range(H):
            du = [kk[:, t, i] + _dot((K[:, t, i, j], dx[j]) for j in range(n)) for i in range(m)]
            for i in range(m):
                du64[:, t, i] = du[i]
                du32[:, t, i] = du[i].astype(np.float32)
            dx = [_dot((A[:, t, i, j], dx[j]) for j in range(n)) + _dot((Bm[:, t, i, k], du[k]) for k in range(m)) for i in range(n)]
    ok = (status == 0) & np.isfinite(dV) & np.isfinite(du32).all(axis=(1, 2))
    du32[~ok] = 0.0
    du64[~ok] = 0.0
    dV = np.where(ok, dV, np.nan)
    return dict(du=du32, du64=du64, dV=dV, status=status, K=K, k=kk, P=Pall)


def direction(A, Bm, traj, u, cost, n, m, mu, ref=None):
    """k_gn_direction on the device's float32 A, Bm, traj, u; ref: (B,H+1,n) reference rows (reference_rows) or None."""
    Lxx, Luu = tm.cost_matrices_of(cost, n, m)
    ldiag, lx, lu = gradients(traj, u, cost, n, m, ref)
    return direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, mu)


def clamp(v, cost):
    """The library's clamp: fminf(fmaxf(v, lo), hi) with a NaN passed on."""
    if not cost.has_u_bounds:
        return v
    lo, hi = np.float32(cost.u_min), np.float32(cost.u_max)
    return np.where(np.isnan(v), v, np.minimum(np.maximum(v, lo), hi)).astype(np.float32)


def alphas(L):
    return np.array([2.0 ** -j for j in range(L)], np.float32)


def candidates(u, du, L, cost):
    """u, du (B,H,m) float32 -> (B*L,H,m): row b*L + j = clamp(u_b + alpha_j * du_b), the product rounded first."""
    u, du = np.asarray(u, np.float32), np.asarray(du, np.float32)
    with np.errstate(all="ignore"):
        step = (alphas(L)[None, :, None, None] * du[:, None]).astype(np.float32)
        v = (u[:, None] + step).astype(np.float32)
    return clamp(v, cost).reshape((u.shape[0] * L,) + u.shape[1:])


def select(u, traj, cost_b, mu, accepts, cand, s, ctraj, status, L, mu_min, mu_max, mu_up, mu_down):
    """-> dict(u, traj, cost, mu, accepts, costs_row, alpha_row): copies with k_gn_select applied."""
    u, traj, cost_b = np.array(u, np.float32), np.array(traj, np.float32), np.array(cost_b, np.float32)
    mu, accepts = np.array(mu, np.float64), np.array(accepts, np.int32)
    nb = u.shape[0]
    cand = np.asarray(cand, np.float32).reshape((nb, L) + u.shape[1:])
    ctraj = np.asarray(ctraj, np.float32).reshape((nb, L) + traj.shape[1:])
    s = np.asarray(s, np.float32).reshape(nb, L)
    costs_row, alpha_row = cost_b.copy(), np.zeros(nb, np.float32)
    al = alphas(L)
    with np.errstate(all="ignore"):
        for b in range(nb):
            js = -1
            for j in range(L):
                if np.isfinite(s[b, j]) and (js < 0 or s[b, j] < s[b, js]):
                    js = j
            if status[b] == 0 and js >= 0 and s[b, js] < cost_b[b]:
                u[b], traj[b], cost_b[b] = cand[b, js], ctraj[b, js], s[b, js]
                v = mu[b] * mu_down
                mu[b] = v if v > mu_min else mu_min
                accepts[b] += 1
                alpha_row[b] = al[js]
            else:
                v = mu[b] * mu_up
                mu[b] = v if v < mu_max else mu_max
    return dict(u=u, traj=traj, cost=cost_b, mu=mu, accepts=accepts, costs_row=costs_row, alpha_row=alpha_row)


class GnOracleEngine(LinOracleEngine):
    """LinOracleEngine with the step methods of the Gauss-Newton solve, served by this file (CPU tensors)."""

    def gn_direction(self, A, Bm, traj, u, cost, mu, x_ref=None, ref_offset=0):
        self.calls.append("gn_direction")
        traj = np.asarray(traj)
        nb, H = traj.shape[0], traj.shape[1] - 1
        ref = None if x_ref is None else reference_rows(np.asarray(x_ref), ref_offset, H, nb, self.n)
        r = direction(np.asarray(A), np.asarray(Bm), traj, np.asarray(u), cost, self.n, self.m, np.asarray(mu), ref)
        return dict(du=torch.from_numpy(r["du"]), dV=torch.from_numpy(r["dV"]), status=torch.from_numpy(r["status"]))

    def gn_candidates(self, x0, u, du, cost, line_steps):
        self.calls.append("gn_candidates")
        x0 = np.asarray(x0, np.float32).reshape(-1, self.n)
        v = candidates(np.asarray(u), np.asarray(du), int(line_steps), cost)
        return torch.from_numpy(v), torch.from_numpy(np.repeat(x0, int(line_steps), axis=0))

    def gn_select(self, u, traj, cost_b, mu, accepts, cand, cand_cost, cand_traj, status, line_steps, mu_min, mu_max, mu_up,
                  mu_down, costs_row=None, alpha_row=None):
        self.calls.append("gn_select")
        r = select(u.numpy(), traj.numpy(), cost_b.numpy(), mu.numpy(), accepts.numpy(), cand.numpy(), cand_cost.numpy(),
                   cand_traj.numpy(), status.numpy(), int(line_steps), mu_min, mu_max, mu_up, mu_down)
        for dst, key in ((u, "u"), (traj, "traj"), (cost_b, "cost"), (mu, "mu"), (accepts, "accepts"), (costs_row, "costs_row"),
                         (alpha_row, "alpha_row")):
            if dst is not None:
                dst.copy_(torch.from_numpy(r[key]))


# ----------------------------------------------------------------------------- the slope identity (cross-check with K2)
# In exact arithmetic sum(grad_u * du) = -dV for every mu: du = -(H + mu)^-1 g and dV = g^T (H + mu)^-1 g with g the
# gradient of the cost at u.  The specs and inputs of that check, shared by the CPU measurement and the GPU test.
SLOPE_SPECS = list(vc.NM_SPEC.values())  # one per (n, m) a handle can have
SLOPE_SHAPE = (17, 7)
# worst |sum(g du) + dV| / dV of the float32 oracle on these inputs (test_gn_model prints it; the float64 oracle reaches
# 9.1e-8, because A, Bm and traj are rounded to float32 as the device returns them)
SLOPE_F32_ORACLE = 6.5e-7


def slope_case(sid):
    """x0 (B,n), in-bounds u (B,H,m), cost, dt of the slope check of one spec."""
    s = vc.CENSUS[sid]
    rng = np.random.default_rng(vc.seed_of(sid, s) + 77)
    B, H = SLOPE_SHAPE
    x0 = 0.3 * vc.states(rng, s["n"], B)
    u = np.clip(vc.controls(rng, B, H, s["m"]), vc.U_MIN, vc.U_MAX).astype(np.float32)
    return dict(x0=x0, u=u, cost=vc.cost_of(s, rng), dt=vc.dt_of(s))


def slope_mismatch(grad_u, du, dV):
    """-> (|sum(g du) + dV| per problem, max|g| sum|du| per problem), float64."""
    g, du = np.asarray(grad_u, np.float64), np.asarray(du, np.float64)
    return np.abs((g * du).sum(axis=(1, 2)) + dV), np.abs(g).max(axis=(1, 2)) * np.abs(du).sum(axis=(1, 2))


# ----------------------------------------------------------------------------- convergence against the Adam solve
def convergence_case():
    """The reference's cart-pole MPC configuration (configs/cartpole_mpc.yaml: H = 20, Q, R, bounds, Adam at lr 0.015 for
    30 iterations, zero start) and the initial states of the golden closed-loop runs -> (x0 (5,4), cost, H, lr, iters)."""
    import oracle_lib as ol
    from phnn_mpc_amd import _capi
    with np.load(ol.GOLDEN + "/golden_controllers.npz") as z:
        x0 = np.vstack([z["mpc_x0"][None], z["can_x_b"][None], z["plant_init"]]).astype(np.float32)
    return x0, _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], 0.01, None, -15.0, 15.0), 20, 0.015, 30


# DESIGN.md section 18's table (float64 oracle): one Gauss-Newton iteration is already below Adam's best of 30 on every
# x0 of the set, for both golden models; the tests assert it for two iterations.
CONVERGENCE_ITERS = 2
