"""Float64 references for the linearisation entry points (TEST INFRASTRUCTURE, in the style of cem_model.py), all built
on the CPU oracle (oracle_lib.OracleModel):

  oracle_jacobian      A = df/dx, Bm = df/du at points, row i = OracleModel.vjp with the unit cotangent e_i -- the
                       construction the GPU tests trust; test_linearize_model.py checks it against central differences
  oracle_linearize     A[b,t] = d x_{t+1} / d x_t, Bm[b,t] = d x_{t+1} / d u_t from one-step OracleModel.rollout_vjp
                       with traj_bar = (0, e_i) and cost_bar = 0 -- what phnn_rollout_linearize is pinned against on the
                       GPU, there with the engine's own rollout_vjp
  composed_step        the same step Jacobians composed by hand from the stage Jacobians (Euler: I + dt A; RK4: the
                       chain rule through the four stages)
  LinOracleEngine      OracleEngine + jacobian / rollout_linearize / tvlqr, so that the controllers' feedback_gains runs
                       without a GPU
"""
import numpy as np
import torch

import oracle_lib as ol
import tvlqr_model as tm
from oracle_engine import OracleEngine
from phnn_mpc_amd import _capi


def unit_rows(model, fn, npts):
    """Stack fn(e_i) over the unit cotangents e_i (npts, n) of the model's state: -> list over i."""
    out = []
    for i in range(model.n):
        e = np.zeros((npts, model.n), model.dtype)
        e[:, i] = 1.0
        out.append(fn(e))
    return out


def oracle_jacobian(model, x, u):
    """-> A (B,n,n), Bm (B,n,m): row i of both is model.vjp(x, u, e_i)."""
    x = np.asarray(x).reshape(-1, model.n)
    rows = unit_rows(model, lambda e: model.vjp(x, u, e), x.shape[0])
    return np.stack([r[0] for r in rows], axis=1), np.stack([r[1] for r in rows], axis=1)


def fd_jacobian(model, x, u, h=1e-5):
    """Central differences of model.forward (float64 model): -> A (B,n,n), Bm (B,n,m)."""
    x = np.asarray(x, np.float64).reshape(-1, model.n)
    u = np.asarray(u, np.float64).reshape(-1, model.m)
    A = np.empty((x.shape[0], model.n, model.n))
    Bm = np.empty((x.shape[0], model.n, model.m))
    for j in range(model.n):
        xp, xm = x.copy(), x.copy()
        xp[:, j] += h
        xm[:, j] -= h
        A[:, :, j] = (model.forward(xp, u)[0] - model.forward(xm, u)[0]) / (2 * h)
    for k in range(model.m):
        up, um = u.copy(), u.copy()
        up[:, k] += h
        um[:, k] -= h
        Bm[:, :, k] = (model.forward(x, up)[0] - model.forward(x, um)[0]) / (2 * h)
    return A, Bm


def no_clamp_cost():
    return _capi.Cost()  # all zero: no bounds, no cost


def oracle_linearize(model, traj, u, cost, integrator, dt):
    """traj (B,H+1,n), u (B,H,m) -> A (B,H,n,n), Bm (B,H,n,m) from the B*H one-step rollouts x0 = traj[b,t],
    u = u[b,t] with traj_bar = (0, e_i), cost_bar = 0.  cost None: no clamp."""
    traj = np.asarray(traj)
    B, H = traj.shape[0], traj.shape[1] - 1
    u = np.asarray(u).reshape(B, H, model.m)
    x0 = traj[:, :H].reshape(B * H, model.n)
    U = u.reshape(B * H, 1, model.m)
    cost = no_clamp_cost() if cost is None else cost
    zero = np.zeros(B * H, model.dtype)

    def row(e):
        tb = np.zeros((B * H, 2, model.n), model.dtype)
        tb[:, 1] = e
        gu, gx = model.rollout_vjp(x0, U, cost, integrator, dt, traj_bar=tb, cost_bar=zero)
        return gx, gu[:, 0]

    rows = unit_rows(model, row, B * H)
    A = np.stack([r[0] for r in rows], axis=1).reshape(B, H, model.n, model.n)
    Bm = np.stack([r[1] for r in rows], axis=1).reshape(B, H, model.n, model.m)
    return A, Bm


def composed_step(model, x, u, integrator, dt):
    """d x+ / d x, d x+ / d u of one integrator step at points (x (P,n), u (P,m), u used as given), composed from the
    point Jacobians: Euler I + dt A; RK4 by the chain rule through the stage states (src/integrators.py:97-109)."""
    x = np.asarray(x, np.float64).reshape(-1, model.n)
    u = np.asarray(u, np.float64).reshape(-1, model.m)
    I = np.eye(model.n)[None]
    A1, B1 = oracle_jacobian(model, x, u)
    if integrator == "euler":
        return I + dt * A1, dt * B1
    k1 = model.forward(x, u)[0]
    y2 = x + 0.5 * dt * k1
    A2, B2 = oracle_jacobian(model, y2, u)
    k2 = model.forward(y2, u)[0]
    y3 = x + 0.5 * dt * k2
    A3, B3 = oracle_jacobian(model, y3, u)
    k3 = model.forward(y3, u)[0]
    y4 = x + dt * k3
    A4, B4 = oracle_jacobian(model, y4, u)
    # d k_s / d x and d k_s / d u, stage by stage
    K1x, K1u = A1, B1
    K2x, K2u = A2 @ (I + 0.5 * dt * K1x), A2 @ (0.5 * dt * K1u) + B2
    K3x, K3u = A3 @ (I + 0.5 * dt * K2x), A3 @ (0.5 * dt * K2u) + B3
    K4x, K4u = A4 @ (I + dt * K3x), A4 @ (dt * K3u) + B4
    return (I + dt / 6.0 * (K1x + 2 * K2x + 2 * K3x + K4x), dt / 6.0 * (K1u + 2 * K2u + 2 * K3u + K4u))


def rows_of(a):
    """(B,H,n,k) -> (B*H, n*k): one row per rollout-step, for variant_census.err_rows."""
    a = np.asarray(a)
    return a.reshape(a.shape[0] * a.shape[1], -1)


class LinOracleEngine(OracleEngine):
    """OracleEngine with the three linearisation methods of RolloutEngine, served by the float64 oracle and
    tvlqr_model (results as CPU tensors; A and Bm rounded to float32 as the device returns them)."""

    def __init__(self, state_dict, precision="f32"):
        super().__init__(state_dict, precision)
        self.m64 = ol.OracleModel(state_dict, "f64")
        self.calls = []

    def jacobian(self, x, u):
        self.calls.append("jacobian")
        A, Bm = oracle_jacobian(self.m64, np.asarray(x), np.asarray(u))
        return self._out(A), self._out(Bm)

    def rollout_linearize(self, x0, u, cost, integrator="euler", dt=0.02, traj=None):
        self.calls.append("rollout_linearize")
        x0 = np.asarray(x0).reshape(-1, self.n)
        u = np.asarray(u).reshape(x0.shape[0], -1, self.m)
        if traj is None:
            traj = self.m_.rollout(x0, u, cost, integrator, dt, grad=False, traj=True)["traj"]
        A, Bm = oracle_linearize(self.m64, np.asarray(traj), u, cost, integrator, dt)
        return self._out(A), self._out(Bm), self._out(np.asarray(traj))

    def tvlqr(self, A, Bm, cost, mu=0.0, want_P=False):
        self.calls.append("tvlqr")
        Lxx, Luu = tm.cost_matrices_of(cost, self.n, self.m)
        r = tm.tvlqr(np.asarray(A), np.asarray(Bm), Lxx, Luu, mu)
        return dict(K=torch.from_numpy(r["K"]), P0=torch.from_numpy(r["P0"]),
                    P=torch.from_numpy(r["P"]) if want_P else None, status=torch.from_numpy(r["status"]))
