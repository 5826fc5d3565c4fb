"""Terminal cost of the Adam and Gauss-Newton solves (include/phnn_mpc.h: phnn_terminal).

Every solve minimises the reference's cost, which weights the last state of the horizon like every other one.  A
TerminalCost adds  e_H^T W e_H  (e_H = x_H - its target or reference row) to the cost of every rollout: W (n,n) shared
by the batch, or (B,n,n) with one matrix per problem.  TerminalCost.lqr builds the usual W: the cost-to-go of the
infinite-horizon LQR of the model linearised at the target, minus the Q the stage cost already charges at t = H.

  controller = MPCController(model, ..., terminal=TerminalCost.lqr(model.engine, cost, x_target, "euler", dt))
  config:  mpc: {terminal: {type: lqr}}   or   mpc: {terminal: {type: matrix, W: [[...], ...]}}

The Adam ('Adam') and Gauss-Newton ('GaussNewton') solves take one; L-BFGS, MPPI and CrossEntropy refuse it.
"""
import numpy as np
import torch

DARE_MAX_ITERS = 200000  # untrained models of this family need some 62 000 Riccati steps at tol 1e-12
DARE_TOL = 1e-12


class TerminalCost:
    """W: (n,n), or (B,n,n) for one matrix per problem -- anything np.asarray takes, or a torch tensor; kept as float32.
    The object keys a captured solve by identity and its device tensor is what the graph reads: keep the object."""

    def __init__(self, W):
        if isinstance(W, torch.Tensor):
            W = W.detach().cpu().numpy()
        W = np.ascontiguousarray(np.asarray(W, dtype=np.float32))
        if W.ndim not in (2, 3) or W.shape[-1] != W.shape[-2]:
            raise ValueError(f"TerminalCost: W must be (n,n) or (B,n,n), got {W.shape}")
        self.W = W
        self.info = None  # TerminalCost.lqr: dict(P, K, iters, status) of the DARE iteration
        self._dev = {}

    @property
    def n(self):
        return self.W.shape[-1]

    @property
    def per_problem(self):
        return self.W.ndim == 3

    def check(self, B, n):
        """Raises unless W fits B problems of state dimension n."""
        if self.n != n or (self.per_problem and self.W.shape[0] != B):
            raise ValueError(f"TerminalCost: W of shape {self.W.shape} does not fit B = {B} problems of state dimension {n}")

    def tensor(self, device):
        """The float32 tensor of W on `device`, made once per device."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.W).to(device).contiguous()
        return self._dev[device]

    @classmethod
    def lqr(cls, engine, cost, x_target=None, integrator="euler", dt=0.02, max_iters=DARE_MAX_ITERS, tol=DARE_TOL, mu=0.0):
        """The LQR terminal weight at x_target (None: the cost's) with u = 0: engine.rollout_linearize there with H = 1,
        then engine.dare.  x_target (n,) -> one W for the batch; (B,n) -> one per problem.  Raises RuntimeError where
        the iteration failed (status 1) or did not converge within max_iters (status 2)."""
        n, m = engine.n, engine.m
        if x_target is None:
            x_target = np.ctypeslib.as_array(cost.x_target)[:n]
        xt = np.asarray(x_target, dtype=np.float32)
        shared = xt.ndim == 1
        xt = xt.reshape(-1, n)
        x0 = torch.as_tensor(xt, dtype=torch.float32).to(engine.device)
        u = torch.zeros(xt.shape[0], 1, m, dtype=torch.float32, device=engine.device)
        A, Bm, _ = engine.rollout_linearize(x0, u, cost, integrator, dt)
        r = engine.dare(A[:, 0], Bm[:, 0], cost, max_iters=max_iters, tol=tol, mu=mu)
        status = r["status"].cpu().numpy()
        if np.any(status != 0):
            b = int(np.flatnonzero(status)[0])
            what = {1: "failed (a pivot of Quu that is not positive, or a value that is not finite)",
                    2: f"did not converge within max_iters = {int(max_iters)}"}.get(int(status[b]), f"status {int(status[b])}")
            raise RuntimeError(f"TerminalCost.lqr: the Riccati iteration of problem {b} {what} after "
                               f"{int(r['iters'].cpu().numpy()[b])} steps")
        W = r["W"].cpu().numpy()
        t = cls(W[0] if shared else W)
        t.info = {k: r[k].cpu().numpy() for k in ("P", "K", "iters", "status")}
        return t


def resolve(spec, engine, cost, integrator, dt):
    """The `terminal` section of an mpc config -> TerminalCost or None.  None / a TerminalCost pass through;
    {type: lqr[, max_iters, tol]} is TerminalCost.lqr at the cost's target; {type: matrix, W: [...]} the given matrix."""
    if spec is None or isinstance(spec, TerminalCost):
        return spec
    if not isinstance(spec, dict) or "type" not in spec:
        raise ValueError(f"terminal: a TerminalCost or a dict with a 'type' (lqr | matrix), got {spec!r}")
    kind = spec["type"]
    if kind == "lqr":
        unknown = set(spec) - {"type", "max_iters", "tol"}
        if unknown:
            raise ValueError(f"terminal: unknown key(s) {sorted(unknown)} for type lqr")
        return TerminalCost.lqr(engine, cost, None, integrator, dt, max_iters=spec.get("max_iters", DARE_MAX_ITERS),
                                tol=spec.get("tol", DARE_TOL))
    if kind == "matrix":
        if "W" not in spec:
            raise ValueError("terminal: type matrix needs W")
        return TerminalCost(spec["W"])
    raise ValueError(f"terminal: unknown type {kind!r} (lqr | matrix)")


def refuse(terminal, what):
    """The solves without a terminal term call this: a terminal weight is refused, never ignored."""
    if terminal is not None:
        raise ValueError(f"{what} takes no terminal cost: the Adam and Gauss-Newton solves do "
                         "(optimizer 'Adam' / 'GaussNewton')")
