"""The tracking law between two solves (phnn_feedback_control), stated operation for operation
(TEST INFRASTRUCTURE, in the style of ekf_model.py, whose `_dot` comes from tvlqr_model.py): float64, no fused
multiply-adds, the inner product with its index ascending from an accumulator 0.0, each product rounded, then added.
k_feedback_control (phnn_feedback.hip) follows this file and is pinned against it bit for bit
(tests/test_gpu_feedback.py).

Vectorised over the batch only: every operation below acts on arrays of shape (B,) element-wise, so each problem sees
exactly the scalar sequence written here.  j is the plan row, clampf the library's float32 clamp that keeps a NaN (applied
only with bounds):

  un_k = clampf(u[b,j,k])
  dx_i = (double)x[b,i] - (double)traj[b,j,i]
  s_k  = sum_i K[b,j,k,i] dx_i
  v_k  = clampf((float)((double)un_k + s_k));  where s_k == 0.0 the result is un_k itself (its bits: a -0.0 stays)
  status 2 where a dx_i is not finite, else 1 where an entry of K[b,j] is not finite, else 0
  u_out_k = v_k for status 0, un_k otherwise;  dev = max_i |dx_i|, NaN for status 2

  control               that statement
  plan                  the nominal trajectory and the gains of a plan on LinOracleEngine and tvlqr_model.tvlqr
  lq_plan               a seeded LQ problem's optimal plan (tvlqr_model.seeded_problem), stored as the device stores it
  FeedbackOracleEngine  EkfOracleEngine + feedback_control, so that feedback.Tracking and the closed loop with track= run
                        without a GPU
"""
import numpy as np
import torch

import tvlqr_model as tm
from ekf_model import EkfOracleEngine
from tvlqr_model import _dot, same_floats  # noqa: F401  (same_floats: re-exported for the tests)


def clampf(v, lo, hi, on):
    """fminf(fmaxf(v, lo), hi) in float32 where `on` and v is not NaN, else v."""
    v = np.asarray(v, np.float32)
    if not on:
        return v
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), v, np.minimum(np.maximum(v, lo), hi)).astype(np.float32)


def control(x, u, traj, K, j, bounds=None):
    """x (B,n) float32, u (B,H,m) float32, traj (B,H+1,n) float32, K (B,H,m,n) float64, j the plan row, bounds None or
    (u_min, u_max) -> dict(u (B,m) float32, status (B) int32, dev (B) float64, v64 (B,m): un + s before its rounding)."""
    x = np.asarray(x, np.float32)
    nb, n = x.shape
    K = np.asarray(K, np.float64)
    H, m = K.shape[1], K.shape[2]
    u = np.asarray(u, np.float32).reshape(nb, H, m)
    traj = np.asarray(traj, np.float32).reshape(nb, H + 1, n)
    on = bounds is not None
    lo, hi = bounds if on else (0.0, 0.0)
    with np.errstate(all="ignore"):
        dx = [x[:, i].astype(np.float64) - traj[:, j, i].astype(np.float64) for i in range(n)]
        bad_dx = np.zeros(nb, bool)
        dev = np.zeros(nb)
        for i in range(n):
            bad_dx |= ~np.isfinite(dx[i])
            dev = np.fmax(dev, np.abs(dx[i]))
        bad_K = np.zeros(nb, bool)
        out = np.empty((nb, m), np.float32)
        v64 = np.empty((nb, m))
        un = []
        for k in range(m):
            un.append(clampf(u[:, j, k], lo, hi, on))
            for i in range(n):
                bad_K |= ~np.isfinite(K[:, j, k, i])
            s = _dot((K[:, j, k, i], dx[i]) for i in range(n))
            v64[:, k] = un[k].astype(np.float64) + s
            v = clampf(v64[:, k].astype(np.float32), lo, hi, on)
            out[:, k] = np.where(s == 0.0, un[k], v)
        status = np.where(bad_dx, 2, np.where(bad_K, 1, 0)).astype(np.int32)
        for k in range(m):
            out[:, k] = np.where(status != 0, un[k], out[:, k])
    return dict(u=out, status=status, dev=np.where(bad_dx, np.nan, dev), v64=v64)


def plan(engine, x, u, cost, integrator, dt, mu=0.0):
    """The plan of phnn_feedback_plan on a LinOracleEngine: K1's trajectory from x with the cost's clamp, the
    linearisation of that rollout, tvlqr_model.tvlqr on it -> dict(traj (B,H+1,n) float32, K (B,H,m,n), status), numpy."""
    x = torch.as_tensor(np.asarray(x, np.float32))
    u = torch.as_tensor(np.asarray(u, np.float32))
    _, traj = engine.rollout_cost(x, u, cost, integrator, dt, want_traj=True)
    A, Bm, _ = engine.rollout_linearize(x, u, cost, integrator, dt, traj=traj)
    Lxx, Luu = tm.cost_matrices_of(cost, engine.n, engine.m)
    r = tm.tvlqr(A.numpy(), Bm.numpy(), Lxx, Luu, mu)
    return dict(traj=traj.numpy(), K=r["K"], status=r["status"])


def lq_plan(seed, nb, H, n, m):
    """tvlqr_model.seeded_problem with its LQ optimum from a seeded x0 = N(0,1) as the plan: u*_t = K_t x*_t,
    x*_{t+1} = A_t x*_t + B_t u*_t in float64, stored as float32 the way the device stores a plan ->
    dict(A, Bm (float64), Lxx, Luu, K (B,H,m,n), P (B,H+1,n,n), u (B,H,m) float32, traj (B,H+1,n) float32)."""
    A, Bm, Q, R = tm.seeded_problem(seed, nb, H, n, m)
    Lxx, Luu = tm.cost_matrices(Q, R, n, m)
    r = tm.tvlqr(A, Bm, Lxx, Luu)
    assert not r["status"].any()
    A, Bm = A.astype(np.float64), Bm.astype(np.float64)
    xs = np.empty((nb, H + 1, n))
    us = np.empty((nb, H, m))
    xs[:, 0] = np.random.default_rng(seed + 1000).normal(size=(nb, n))
    for t in range(H):
        us[:, t] = np.einsum("bki,bi->bk", r["K"][:, t], xs[:, t])
        xs[:, t + 1] = np.einsum("bij,bj->bi", A[:, t], xs[:, t]) + np.einsum("bik,bk->bi", Bm[:, t], us[:, t])
    return dict(A=A, Bm=Bm, Lxx=Lxx, Luu=Luu, K=r["K"], P=r["P"], u=us.astype(np.float32), traj=xs.astype(np.float32))


def lq_cost_to_go(p, x, j, law):
    """The LQ cost from row j to the end of the horizon from the float64 state x (B,n): sum_t 1/2 (x^T Lxx x + u^T Luu u)
    + 1/2 x_H^T Lxx x_H with u_t = law(x_t, t) (B,m), the states stepped through the problem's A_t, B_t in float64."""
    H = p["K"].shape[1]
    x = np.array(x, np.float64)
    total = np.zeros(x.shape[0])
    for t in range(j, H):
        u = np.asarray(law(x, t), np.float64)
        total += 0.5 * (np.einsum("bi,ij,bj->b", x, p["Lxx"], x) + np.einsum("bi,ij,bj->b", u, p["Luu"], u))
        x = np.einsum("bij,bj->bi", p["A"][:, t], x) + np.einsum("bik,bk->bi", p["Bm"][:, t], u)
    return total + 0.5 * np.einsum("bi,ij,bj->b", x, p["Lxx"], x)


class FeedbackOracleEngine(EkfOracleEngine):
    """EkfOracleEngine with feedback_control served by this file (CPU tensors), so that feedback.Tracking and the
    closed loop with track= (and an estimator) run without a GPU."""

    def feedback_control(self, x, u, traj, K, cost, solve_every, step=0, step_dev=None, u_out=None, status=True, dev=True,
                         log_status=None, log_dev=None):
        self.calls.append("feedback_control")
        step = int(step_dev[0]) if step_dev is not None else int(step)
        bounds = (cost.u_min, cost.u_max) if cost is not None and cost.has_u_bounds else None
        r = control(np.asarray(x), np.asarray(u), np.asarray(traj), np.asarray(K), step % int(solve_every), bounds)
        return dict(u=torch.from_numpy(r["u"]), status=torch.from_numpy(r["status"]), dev=torch.from_numpy(r["dev"]))
