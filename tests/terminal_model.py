"""The terminal cost (include/phnn_mpc.h: phnn_terminal), stated operation for operation (TEST
INFRASTRUCTURE, in the style of tvlqr_model.py and gn_model.py, on which it builds):

  terminal_cost          k_terminal_cost: float32; the fused multiply-adds written here are the only ones
                           e_i = x_H,i - r_i;  s_j = fma(e_i, W[i][j], s_j), i ascending from 0;  c = fma(s_j, e_j, c), j
                           ascending from 0;  cost = cost + c;  g_i = fma(W[i][j] + W[j][i], e_j, g_i), j ascending from 0,
                           the sum of the two weights rounded once in float32;  rows t < H of traj_bar are not touched
  dare                   k_dare: tvlqr_model's Riccati step on one (A, B) per problem from P_0 = Lxx.  After step k:
                           d = max |P_k - P_{k-1}|, s = max |P_k|;  a failed pivot, an s that is NaN or +inf: status 1;
                           d <= tol * s: status 0;  k == max_iters: status 2.  W = (float)(0.5 (P_k - Lxx)) entry by entry;
                           a W entry that is not finite: status 1.  Status 1: P, K, W all NaN.  iters = k.
  terminal_init          the start of the direction's backward sweep:  Tf[i][j] = (double)W[i][j] + (double)W[j][i],
                           P_H = Lxx_H + Tf,  p_H[i] = lx_H[i] + sum_k Tf[i][k] e_k (k ascending from 0.0, each product
                           rounded, then added), e = (double)x_H - (double)r_H
  direction              k_gn_direction / k_gn_direction_box with that start: gn_box_model.direction_box_core's step, one
                           problem at a time (with bounds -inf / +inf it is gn_model.direction_core's, operation for
                           operation -- tests/test_terminal_model.py pins both identities bit for bit without a terminal)
  TerminalOracleEngine   GnBoxOracleEngine + terminal_cost, dare, rollout_vjp and gn_direction(terminal=), so that the
                         solves and the controllers run with a terminal weight without a GPU

direction_core is a SECOND statement of gn_box_model.direction_box_core: that file may not change, so its hundred lines
are repeated here with the two lines of the terminal start added.  A change to the step there has to be made here by
hand; tests/test_terminal_model.py::test_without_a_terminal_weight_the_core_is_gn_models_bit_for_bit is what notices when
the two have drifted apart.
"""
import numpy as np
import torch

import gn_box_model as gb
import gn_model as gm
import tvlqr_model as tm
from adam_model import fma32
from gn_box_model import ZERO, _ldl, _solve, _sym, all_free, enumerate_box_qp
from tvlqr_model import _dot


def weights_of(terminal, nb, n, group=1):
    """terminal: a TerminalCost or an (n,n) / (P,n,n) array -> (nb,n,n) float32, row i the W of problem i // group."""
    W = np.asarray(getattr(terminal, "W", terminal), np.float32)
    if W.ndim == 2:
        return np.broadcast_to(W, (nb, n, n))
    return W[np.arange(nb) // int(group)]


def target_rows(cost, n, nb, H, x_ref=None, ref_offset=0):
    """The (nb,n) float32 row the terminal term is taken about: the reference row min(offset + H, rows - 1), or x_target."""
    if x_ref is None:
        return np.broadcast_to(np.ctypeslib.as_array(cost.x_target)[:n].astype(np.float32), (nb, n))
    return gm.reference_rows(np.asarray(x_ref), ref_offset, H, nb, n)[:, H]


def terminal_cost(traj, W, r, cost_b, traj_bar=None):
    """traj (B,H+1,n), W (B,n,n), r (B,n), cost_b (B) float32 -> (cost_b + c (B) float32, traj_bar with row H replaced or
    None)."""
    x = np.asarray(traj, np.float32)
    nb, H1, n = x.shape
    W = np.asarray(W, np.float32)
    with np.errstate(all="ignore"):
        e = (x[:, H1 - 1] - np.asarray(r, np.float32)).astype(np.float32)
        c = np.zeros(nb, np.float32)
        for j in range(n):
            s = np.zeros(nb, np.float32)
            for i in range(n):
                s = fma32(e[:, i], W[:, i, j], s)
            c = fma32(s, e[:, j], c)
        out = (np.asarray(cost_b, np.float32) + c).astype(np.float32)
        if traj_bar is None:
            return out, None
        tb = np.array(traj_bar, np.float32)
        for i in range(n):
            a = np.zeros(nb, np.float32)
            for j in range(n):
                a = fma32((W[:, i, j] + W[:, j, i]).astype(np.float32), e[:, j], a)
            tb[:, H1 - 1, i] = a
    return out, tb


def terminal_gradient64(traj, W, r):
    """The float64 gradient of e_H^T W e_H with respect to x_H: (W + W^T) e_H, (B,n)."""
    x = np.asarray(traj, np.float32).astype(np.float64)
    W = np.asarray(W, np.float32).astype(np.float64)
    e = x[:, -1] - np.asarray(r, np.float32).astype(np.float64)
    return np.einsum("bij,bj->bi", W + np.swapaxes(W, 1, 2), e)


def dare(A, Bm, Lxx, Luu, max_iters, tol, mu=0.0):
    """A (B,n,n), Bm (B,n,m) float32; Lxx, Luu float64 -> dict(P (B,n,n), K (B,m,n) float64, W (B,n,n) float32, iters (B)
    int32, status (B) int32).  One problem at a time (each runs its own number of steps), every step tvlqr_model's on
    the problem's (A, B) from the current P (_step; tests/test_terminal_model.py pins N steps against tm.tvlqr on N
    copies of (A, B) bit for bit)."""
    A = np.asarray(A, np.float32)
    Bm = np.asarray(Bm, np.float32)
    nb, n, m = A.shape[0], A.shape[1], Bm.shape[2]
    Lxx = np.asarray(Lxx, np.float64)
    P_out = np.full((nb, n, n), np.nan)
    K_out = np.full((nb, m, n), np.nan)
    W_out = np.full((nb, n, n), np.nan, np.float32)
    iters = np.zeros(nb, np.int32)
    status = np.zeros(nb, np.int32)
    with np.errstate(all="ignore"):
        for b in range(nb):
            P = Lxx.copy()
            K = np.zeros((m, n))
            st, k = 2, 0
            while k < int(max_iters):
                k += 1
                r = _step(A[b], Bm[b], P, Lxx, Luu, mu)
                if r is None:
                    st = 1
                    break
                Pn, K = r
                s = np.float64(0.0)
                d = np.float64(0.0)
                nan = False
                for i in range(n):
                    for j in range(n):
                        a, c = abs(Pn[i, j]), abs(Pn[i, j] - P[i, j])
                        nan = nan or bool(a != a)
                        if a > s:
                            s = a
                        if c > d:
                            d = c
                P = Pn
                if nan or s == np.inf:
                    st = 1
                    break
                if d <= float(tol) * s:
                    st = 0
                    break
            Wf = (0.5 * (P - Lxx)).astype(np.float32)
            if not np.all(np.isfinite(Wf)):
                st = 1
            iters[b], status[b] = k, st
            if st != 1:
                P_out[b], K_out[b], W_out[b] = P, K, Wf
    return dict(P=P_out, K=K_out, W=W_out, iters=iters, status=status)


def _step(A, Bm, P, Lxx, Luu, mu):
    """tvlqr_model's step t on (A (n,n), Bm (n,m) float32) from the cost-to-go P -> (P_t (n,n), K_t (m,n)) or None on a
    pivot failure.  The operations are tm.tvlqr's, line for line, on scalars."""
    A = np.asarray(A, np.float32).astype(np.float64)
    Bm = np.asarray(Bm, np.float32).astype(np.float64)
    n, m = A.shape[0], Bm.shape[1]
    rn, rm = range(n), range(m)
    S = [[_dot((P[i][k], A[k][j]) for k in rn) for j in rn] for i in rn]
    T = [[_dot((P[i][k], Bm[k][j]) for k in rn) for j in rm] for i in rn]
    Qxx = [[Lxx[i][j] + _dot((A[k][i], S[k][j]) for k in rn) for j in rn] for i in rn]
    Qux = [[_dot((Bm[k][i], S[k][j]) for k in rn) for j in rn] for i in rm]
    Quu = [[None] * m for _ in rm]
    for i in rm:
        for j in range(i + 1):
            q = Luu[i][j] + _dot((Bm[k][i], T[k][j]) for k in rn)
            if i == j:
                q = q + np.float64(mu)
            Quu[i][j] = q
    L, D, bad = _ldl(Quu, m)
    if bad:
        return None
    X = [[None] * n for _ in rm]
    for c in rn:
        col = _solve(L, D, [Qux[i][c] for i in rm], m)
        for i in rm:
            X[i][c] = col[i]
    Pn = [[Qxx[i][j] - _dot((Qux[k][i], X[k][j]) for k in rm) for j in rn] for i in rn]
    Pt = np.empty((n, n))
    for i in rn:
        for j in range(i, n):
            s = 0.5 * (Pn[i][j] + Pn[j][i])
            Pt[i, j] = s
            Pt[j, i] = s
    return Pt, np.array([[-X[i][j] for j in rn] for i in rm])


def terminal_init(W, e_H):
    """W (B,n,n) float32, e_H (B,n) float64 -> (Tf (B,n,n), Tf e_H (B,n)) float64 as the direction kernels form them."""
    W = np.asarray(W, np.float32).astype(np.float64)
    nb, n, _ = W.shape
    Tf = W + np.swapaxes(W, 1, 2)
    with np.errstate(all="ignore"):
        te = np.stack([_dot((Tf[:, i, k], e_H[:, k]) for k in range(n)) for i in range(n)], axis=1)
    return Tf, te


def direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, mu, lo, hi, Tf=None, te=None):
    """gn_box_model.direction_box_core with the terminal start of the backward sweep: Tf (B,n,n), te (B,n) float64 from
    terminal_init, or None for the plain start.  The rest is that function's, line for line."""
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
            if Tf is not None:  # the terminal weight: P_H = Lxx_H + Tf, p_H = lx_H + Tf e_H
                P = [[P[i][j] + Tf[b, i, j] for j in rn] for i in rn]
                pv = [lx[b, H, i] + te[b, i] for i in rn]
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
                    if v > hi[b, t, i]:
                        v = hi[b, t, i]
                    du[i] = v
                    du64[b, t, i] = v
                    du32[b, t, i] = np.float32(v)
                dx = [_dot((A[b, t, i, j], dx[j]) for j in rn) + _dot((Bm[b, t, i, k], du[k]) for k in rm) for i in rn]
    ok = (status == 0) & np.isfinite(dVs) & np.isfinite(du32).all(axis=(1, 2))
    du32[~ok] = 0.0
    du64[~ok] = 0.0
    nclamp[~ok] = 0
    return dict(du=du32, du64=du64, dV=np.where(ok, dVs, np.nan), status=status, nclamp=nclamp, K=K, k=kk, P=Pall)


def direction(A, Bm, traj, u, cost, n, m, mu, W=None, ref=None, box=False):
    """k_gn_direction (box False) / k_gn_direction_box (box True) with the terminal weight W (B,n,n) float32 or None, on
    the device's float32 A, Bm, traj, u; ref: (B,H+1,n) reference rows (gm.reference_rows) or None."""
    Lxx, Luu = tm.cost_matrices_of(cost, n, m)
    ldiag, lx, lu = gm.gradients(traj, u, cost, n, m, ref)
    if box:
        lo, hi = gb.step_bounds(np.asarray(u, np.float32).reshape(lu.shape), cost)
    else:
        lo, hi = np.full(lu.shape, -np.inf), np.full(lu.shape, np.inf)
    Tf = te = None
    if W is not None:
        x = np.asarray(traj, np.float32).astype(np.float64)
        nb = x.shape[0]
        if ref is None:
            r = np.broadcast_to(np.ctypeslib.as_array(cost.x_target)[:n].astype(np.float32).astype(np.float64), (nb, n))
        else:
            r = np.asarray(ref, np.float32).astype(np.float64)[:, -1]
        Tf, te = terminal_init(W, x[:, -1] - r)
    return direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, mu, lo, hi, Tf, te)


class TerminalOracleEngine(gb.GnBoxOracleEngine):
    """GnBoxOracleEngine with the terminal cost's methods, served by this file (CPU tensors)."""

    def terminal_cost(self, traj, cost, terminal, cost_b, traj_bar=None, want_traj_bar=False, x_ref=None, ref_offset=0,
                      group=1):
        self.calls.append("terminal_cost")
        traj = np.asarray(traj)
        nb, H = traj.shape[0], traj.shape[1] - 1
        if traj_bar is None and want_traj_bar:
            traj_bar = torch.zeros(nb, H + 1, self.n)
        W = weights_of(terminal, nb, self.n, group)
        r = target_rows(cost, self.n, nb, H, x_ref, ref_offset)
        c, tb = terminal_cost(traj, W, r, cost_b.numpy(), None if traj_bar is None else traj_bar.numpy())
        cost_b.copy_(torch.from_numpy(c))
        if traj_bar is not None:
            traj_bar.copy_(torch.from_numpy(tb))
        return traj_bar

    def dare(self, A, Bm, cost, max_iters=None, tol=None, mu=0.0):
        from phnn_mpc_amd.terminal import DARE_MAX_ITERS, DARE_TOL
        self.calls.append("dare")
        Lxx, Luu = tm.cost_matrices_of(cost, self.n, self.m)
        r = dare(np.asarray(A).reshape(-1, self.n, self.n), np.asarray(Bm).reshape(-1, self.n, self.m), Lxx, Luu,
                 DARE_MAX_ITERS if max_iters is None else max_iters, DARE_TOL if tol is None else tol, mu)
        return {k: torch.from_numpy(v) for k, v in r.items()}

    def rollout_vjp(self, x0, u, traj, cost, integrator="euler", dt=0.02, traj_bar=None, cost_bar=None):
        self.calls.append("rollout_vjp")
        gu, gx = self.m_.rollout_vjp(np.asarray(x0), np.asarray(u), cost, integrator, dt,
                                     None if traj_bar is None else np.asarray(traj_bar),
                                     None if cost_bar is None else np.asarray(cost_bar))
        return self._out(gu), self._out(gx)

    def gn_direction(self, A, Bm, traj, u, cost, mu, x_ref=None, ref_offset=0, box=False, terminal=None):
        if terminal is None:
            return super().gn_direction(A, Bm, traj, u, cost, mu, x_ref=x_ref, ref_offset=ref_offset, box=box)
        self.calls.append("gn_direction")
        traj = np.asarray(traj)
        nb, H = traj.shape[0], traj.shape[1] - 1
        ref = None if x_ref is None else gm.reference_rows(np.asarray(x_ref), ref_offset, H, nb, self.n)
        r = direction(np.asarray(A), np.asarray(Bm), traj, np.asarray(u), cost, self.n, self.m, np.asarray(mu),
                      weights_of(terminal, nb, self.n), ref, box)
        return {k: torch.from_numpy(r[k]) for k in (("du", "dV", "status", "nclamp") if box else ("du", "dV", "status"))}


# ----------------------------------------------------------------------------- the DARE cases of the tests
def linearize_at_target(name, integrator):
    """(A (1,n,n), Bm (1,n,m) float32, cost) of golden model `name` at (x_target, u = 0) by the float64 oracle, rounded to
    float32 as the device returns them.  The cost and dt are the fixture's own (golden_<name>.npz): for the cart-pole
    models Q_diag, R_diag and dt = 0.02 of configs/cartpole_mpc.yaml, for the pendulum models Q = diag(10, 1), R = 0.01
    and dt = 0.05 -- the settings behind the step counts of DESIGN.md section 22."""
    import oracle_lib as ol
    from linearize_model import oracle_linearize
    g = ol.load_golden(name)
    model = ol.OracleModel(ol.load_weights(name), "f64")
    n, m = model.n, model.m
    cost = ol.cost_from_golden(g)
    x = np.zeros((1, 2, n), np.float32)
    x[:, 0] = np.ctypeslib.as_array(cost.x_target)[:n]
    A, Bm = oracle_linearize(model, x, np.zeros((1, 1, m), np.float32), cost, integrator, float(g["dt"]))
    return A[:, 0].astype(np.float32), Bm[:, 0].astype(np.float32), cost
