"""Drop-in for src/mpc_controller_canonical.py: MPCControllerCanonical with the same constructor, methods, return
values and info dict, solved by the fused kernels, plus batched entry points.

Reference behaviour kept: full Q (n,n) and R (m,m) matrices; Euler rollout; the iterate returned is the BEST
clamped one (cost measured before the Adam step of the same iteration, strict '<', src/mpc_controller_canonical.py:
208-214); control() warm-starts by shifting the previous sequence by one and zero-filling the tail (:252-255) and
returns (u (m,), info{'u_sequence','solve_time','optimization'{'costs','final_cost','num_steps'}}).
optimizer='MPPI' (not in the reference): the same calls solved by the gradient-free sampling solve (engine.solve_mppi):
optimizer_steps iterations of `samples` perturbed rollouts per plant; the sequence returned is the best SAMPLE seen,
'costs' the nominal's cost at every iteration; learning_rate is not used.
optimizer='CrossEntropy' (not in the reference): the cross-entropy sampling solve (engine.solve_cem), called and
returning as the MPPI one does.  (The name is not 'CEM': that string stays an unknown optimizer.)
optimizer='GaussNewton' (not in the reference): projected Gauss-Newton shooting on the rollout's linearisation
(engine.solve_gn), optimizer_steps iterations; a problem's cost never rises, so the sequence returned (best_u) is the
last iterate and best_cost its cost; 'costs' is the cost at the start of every iteration; learning_rate is not used.
terminal= (not in the reference): a terminal.TerminalCost, or the config's `terminal` section, adds e_H^T W e_H to the
cost of the 'Adam' and 'GaussNewton' solves; 'MPPI' and 'CrossEntropy' refuse one.
"""
import os
import time

import numpy as np
import torch

from . import _capi
from .noise import resolve as resolve_noise
from .solver import SAMPLING, _noise_kw, _terminal_kw, gn_solver_for, solver_for
from .terminal import refuse as refuse_terminal
from .terminal import TerminalCost
from .terminal import resolve as resolve_terminal


class MPCControllerCanonical:
    def __init__(self, model, horizon=20, dt=0.02, Q=None, R=None, x_target=None, u_min=-10.0, u_max=10.0,
                 optimizer_steps=50, learning_rate=0.1, verbose=False, optimizer="Adam", samples=64, lam=1.0, sigma=1.0,
                 seed=0, elites=8, alpha=0.25, sigma_min=0.05, noise=None, gn_line_steps=8, mu_init=1e-6, mu_min=1e-9,
                 mu_max=1e6, mu_up=10.0, mu_down=0.1, gn_box=False, terminal=None):
        self.model = model
        self.model.eval()
        self.horizon, self.dt = horizon, dt
        self.optimizer_steps, self.learning_rate, self.verbose = optimizer_steps, learning_rate, verbose
        self.state_dim, self.input_dim = model.state_dim, model.input_dim
        if Q is None:
            Q = np.diag([10.0, 100.0, 1.0, 10.0])  # src/mpc_controller_canonical.py:68-74
        self.Q = torch.tensor(Q, dtype=torch.float32)
        if R is None:
            R = 0.01 * np.eye(self.input_dim)
        self.R = torch.tensor(R, dtype=torch.float32)
        if x_target is None:
            x_target = np.zeros(self.state_dim)
        self.x_target = torch.tensor(x_target, dtype=torch.float32)
        self.u_min, self.u_max = u_min, u_max
        if optimizer not in ("Adam", "MPPI", "CrossEntropy", "GaussNewton"):
            raise ValueError(f"Unknown optimizer type: {optimizer}")
        # optimizer='MPPI': samples per plant and iteration, softmin temperature (units of the cost), noise standard
        # deviation (one value or one per input), noise seed; `epoch` numbers the solves that are not given one
        self.optimizer, self.samples, self.lam, self.sigma, self.seed, self.epoch = optimizer, samples, lam, sigma, seed, 0
        # optimizer='CrossEntropy': samples, sigma (the initial standard deviation), seed and epoch as above; elites: how
        # many lowest-cost samples the distribution is refitted to, smoothing alpha in [0, 1), floor of sigma
        self.elites, self.alpha, self.sigma_min = elites, alpha, sigma_min
        # MPPI and CrossEntropy: the time correlation of the sampling noise (noise.resolve: None = white, a noise.Noise,
        # {"type": "ar1" | "colored" | "knots", ...} or an (H, P) array); ValueError for an unknown type or another horizon
        self.noise = resolve_noise(noise, horizon)
        # optimizer='GaussNewton': candidates per line search, and the Levenberg-Marquardt term's start, range and factors
        self.gn_line_steps, self.mu_init, self.mu_min, self.mu_max = gn_line_steps, mu_init, mu_min, mu_max
        self.mu_up, self.mu_down = mu_up, mu_down
        # gn_box: the LQ step of every iteration respects u_min / u_max (control-limited DDP)
        self.gn_box = bool(gn_box)
        # terminal weight of the Adam and Gauss-Newton solves: None, a terminal.TerminalCost, or its config section
        # ({type: lqr} is resolved on the engine at the first solve: terminal_cost())
        self.terminal = terminal
        self.integrator = "euler"
        # True (or PHNN_GRAPH=1): replay the whole solve as one HIP graph instead of 3 x iterations launches
        self.use_graph = os.environ.get("PHNN_GRAPH", "0") == "1"
        self._graphed = None

    def _solver(self, eng):
        self._graphed = solver_for(eng, self.use_graph, self._graphed)
        return self._graphed

    def _cost(self, clamp=True):
        c = _capi.make_cost(self.state_dim, self.input_dim, self.Q.numpy(), self.R.numpy(), self.x_target.numpy(),
                            self.u_min, self.u_max)
        if not clamp:
            c.has_u_bounds = 0
        return c

    def terminal_cost(self):
        """The controller's terminal.TerminalCost, or None.  A config section is resolved here, once (type lqr: the
        linearisation and the DARE iteration run on the engine); a solve without a terminal term refuses one."""
        if self.terminal is None:
            return None
        if self.optimizer not in ("Adam", "GaussNewton"):
            refuse_terminal(self.terminal, f"optimizer {self.optimizer!r}")
        if not isinstance(self.terminal, TerminalCost):  # a config section: resolved once, on the engine
            self.terminal = resolve_terminal(self.terminal, self.engine, self._cost(), self.integrator, self.dt)
        return self.terminal

    @property
    def engine(self):
        return self.model.engine

    # ------------------------------------------------------------------ reference methods
    def compute_cost(self, x_pred, u_seq):
        """(H+1,n), (H,m) -> scalar cost (src/mpc_controller_canonical.py:91-120), host arithmetic."""
        x_pred = torch.as_tensor(x_pred, dtype=torch.float32)
        u_seq = torch.as_tensor(u_seq, dtype=torch.float32)
        e = x_pred[: self.horizon + 1] - self.x_target
        u = u_seq[: self.horizon]
        return ((e @ self.Q) * e).sum() + ((u @ self.R) * u).sum()

    def rollout(self, x0, u_seq):
        """x0 (n,), u_seq (H,m) -> (H+1,n), controls used as given (src/mpc_controller_canonical.py:122-161)."""
        eng = self.engine
        x0d = torch.as_tensor(x0, dtype=torch.float32).reshape(1, -1).to(eng.device)
        ud = torch.as_tensor(u_seq, dtype=torch.float32).reshape(1, -1, self.input_dim).to(eng.device)
        _, traj = eng.rollout_cost(x0d, ud, self._cost(clamp=False), self.integrator, self.dt, want_traj=True)
        return traj[0].cpu()

    def feedback_gains(self, x0, u_seq, mu=0.0):
        """Time-varying LQR gains around the planned trajectory: x0 (B,n) or (n,), u_seq (B,H,m) or (H,m) -> dict(K
        (B,H,m,n), P0 (B,n,n), P (B,H+1,n,n), status (B), traj (B,H+1,n), A, Bm), all on the engine's device.  The
        nominal trajectory x^nominal = traj is this controller's rollout of u_seq (its cost, integrator and dt), and the
        law is  delta u_t = K_t (x_t - x_t^nominal),  to be added to u_seq[t] before the clamp.  Three launches: K1 ->
        linearise -> tvlqr.  status[b] != 0: the recursion failed for problem b (its early gains are NaN); mu > 0
        regularises Quu."""
        eng = self.engine
        x0 = torch.as_tensor(x0, dtype=torch.float32).reshape(-1, self.state_dim)
        u = torch.as_tensor(u_seq, dtype=torch.float32).reshape(x0.shape[0], -1, self.input_dim)
        cost = self._cost()
        A, Bm, traj = eng.rollout_linearize(x0, u, cost, self.integrator, self.dt)
        out = eng.tvlqr(A, Bm, cost, mu=mu, want_P=True)
        out.update(traj=traj, A=A, Bm=Bm)
        return out

    def optimize_control(self, x0, u_init=None):
        """x0 (n,), u_init (H,m) or None -> (u_opt (H,m) tensor, info)   (src/mpc_controller_canonical.py:163-228)"""
        x0 = torch.as_tensor(x0, dtype=torch.float32).reshape(1, -1)
        ui = None if u_init is None else torch.as_tensor(u_init, dtype=torch.float32).reshape(1, self.horizon, -1)
        out = self.optimize_control_batch(x0, ui)
        costs = [float(v) for v in out["costs"][:, 0].cpu()]
        if self.verbose:
            for step, c in enumerate(costs):
                if step % 10 == 0 or step == self.optimizer_steps - 1:
                    print(f"  Step {step:3d}: cost = {c:.4f}")
        info = {"costs": costs, "final_cost": float(out["best_cost"][0].cpu()), "num_steps": self.optimizer_steps}
        return out["best_u"][0].cpu(), info

    def control(self, x_current, u_prev=None):
        """x_current (n,), u_prev (H,m) or None -> (u (m,) np.ndarray, info)  (src/mpc_controller_canonical.py:230-273)"""
        start = time.time()
        x0 = torch.tensor(np.asarray(x_current), dtype=torch.float32)
        u_init = None
        if u_prev is not None:
            up = torch.tensor(np.asarray(u_prev), dtype=torch.float32)
            u_init = torch.cat([up[1:], torch.zeros(1, self.input_dim)], dim=0)
        u_seq_opt, opt_info = self.optimize_control(x0, u_init)
        u = u_seq_opt[0].detach().numpy()
        info = {"u_sequence": u_seq_opt.detach().numpy(), "solve_time": time.time() - start, "optimization": opt_info}
        return u, info

    # ------------------------------------------------------------------ batched (new)
    def mppi_options(self):
        """solve_mppi keyword arguments of this controller."""
        return dict(iters=self.optimizer_steps, samples=self.samples, lam=self.lam,
                    sigma=tuple(np.asarray(self.sigma, dtype=np.float64).reshape(-1).tolist()), seed=self.seed,
                    **_noise_kw(self.noise))

    def cem_options(self):
        """solve_cem keyword arguments of this controller."""
        return dict(iters=self.optimizer_steps, samples=self.samples, elites=self.elites, alpha=self.alpha,
                    sigma=tuple(np.asarray(self.sigma, dtype=np.float64).reshape(-1).tolist()), sigma_min=self.sigma_min,
                    seed=self.seed, **_noise_kw(self.noise))

    def _mppi_epoch(self, eng, epoch):
        """The epoch argument of one solve: `epoch` (None: the controller's own counter, advanced here); with use_graph
        a device counter holding it, so that the captured graph is replayed, not re-captured, when it changes."""
        if epoch is None:
            epoch, self.epoch = self.epoch, self.epoch + 1
        if not self.use_graph or eng.device.type != "cuda" or isinstance(epoch, torch.Tensor):
            return epoch
        if getattr(self, "_epoch_dev", None) is None or self._epoch_dev.device != eng.device:
            self._epoch_dev = torch.zeros(1, dtype=torch.int32, device=eng.device)
        self._epoch_dev.fill_(int(epoch))
        return self._epoch_dev

    def optimize_control_batch(self, x0, u_init=None, record_costs=True, x_ref=None, ref_offset=0, epoch=None):
        """x0 (B,n), u_init (B,H,m) or None -> dict(best_u (B,H,m) clamped, best_cost (B), costs (steps,B), u_last).
        x_ref: per-problem reference trajectories broadcastable to (B, rows, n), tracked from row ref_offset (int or
        device int32 tensor; past its end a reference holds its last row) instead of x_target.
        epoch (MPPI, CrossEntropy): the noise counter of this solve; None: self.epoch, which then advances by one."""
        eng = self.engine
        term = self.terminal_cost()  # refused here by the solves without a terminal term
        x0 = torch.as_tensor(x0, dtype=torch.float32).reshape(-1, self.state_dim).to(eng.device)
        B = x0.shape[0]
        if u_init is None:
            u0 = torch.zeros(B, self.horizon, self.input_dim, dtype=torch.float32, device=eng.device)
        else:
            u0 = torch.as_tensor(u_init, dtype=torch.float32).reshape(B, self.horizon, self.input_dim).to(eng.device)
        if self.optimizer in SAMPLING:
            return self._solve_batch_sampling(x0, u0, record_costs, x_ref, ref_offset, epoch)
        if self.optimizer == "GaussNewton":
            return self._solve_batch_gn(x0, u0, record_costs, x_ref, ref_offset)
        return self._solver(eng)(eng, x0, u0, self._cost(), self.integrator, self.dt, self.learning_rate,
                                 self.optimizer_steps, track_best=True, u_min=self.u_min, u_max=self.u_max,
                                 record_costs=record_costs, x_ref=x_ref, ref_offset=ref_offset, **_terminal_kw(term))

    def _solve_batch_sampling(self, x0, u0, record_costs, x_ref, ref_offset, epoch):
        """The MPPI or cross-entropy solve of optimize_control_batch (engine.solve_mppi / engine.solve_cem)."""
        eng = self.engine
        meth, graphed_or_eager = SAMPLING[self.optimizer]
        solve = graphed_or_eager(eng, self.use_graph, getattr(self, "_graphed_" + meth, None))
        setattr(self, "_graphed_" + meth, solve)
        return solve(eng, x0, u0, self._cost(), self.integrator, self.dt, epoch=self._mppi_epoch(eng, epoch),
                     record_costs=record_costs, x_ref=x_ref, ref_offset=ref_offset, **getattr(self, meth + "_options")())

    def gn_options(self):
        """solve_gn keyword arguments of this controller."""
        opt = dict(iters=self.optimizer_steps, line_steps=self.gn_line_steps, mu_init=self.mu_init, mu_min=self.mu_min,
                   mu_max=self.mu_max, mu_up=self.mu_up, mu_down=self.mu_down)
        if self.gn_box:  # present only when set: the plain solve is called as before
            opt["box"] = True
        opt.update(_terminal_kw(self.terminal_cost()))
        return opt

    def _solve_batch_gn(self, x0, u0, record_costs, x_ref, ref_offset):
        """The Gauss-Newton solve of optimize_control_batch (engine.solve_gn); the workspace stays with the controller.
        best_u / best_cost are the last iterate and its cost (the cost of a problem never rises)."""
        eng = self.engine
        self._graphed_gn = gn_solver_for(eng, self.use_graph, getattr(self, "_graphed_gn", None))
        if getattr(self, "_gn_ws", None) is None:
            self._gn_ws = {}
        out = self._graphed_gn(eng, x0, u0, self._cost(), self.integrator, self.dt, record_costs=record_costs,
                               workspace=self._gn_ws, x_ref=x_ref, ref_offset=ref_offset, **self.gn_options())
        return {**out, "best_u": out["u_last"], "best_cost": out["cost"]}

    def control_batch(self, x_current, u_prev=None, x_ref=None, ref_offset=0, epoch=None):
        """x_current (B,n), u_prev (B,H,m) or None -> (u (B,m), u_sequence (B,H,m), best_cost (B)) numpy arrays.
        x_ref, ref_offset, epoch: optimize_control_batch."""
        u_init = None
        if u_prev is not None:
            up = torch.as_tensor(u_prev, dtype=torch.float32)
            u_init = torch.cat([up[:, 1:], torch.zeros(up.shape[0], 1, self.input_dim)], dim=1)
        out = self.optimize_control_batch(x_current, u_init, record_costs=False, x_ref=x_ref, ref_offset=ref_offset,
                                          epoch=epoch)
        seq = out["best_u"].cpu().numpy()
        return seq[:, 0, :], seq, out["best_cost"].cpu().numpy()


def create_mpc_controller(model, config):
    """src/mpc_controller_canonical.py:276-316"""
    mpc = config.get("mpc", {})
    return MPCControllerCanonical(
        model=model, horizon=mpc.get("horizon", 20), dt=config["cartpole"]["dt"],
        Q=np.diag(mpc.get("Q_diag", [10.0, 100.0, 1.0, 10.0])), R=np.diag(mpc.get("R_diag", [0.01])),
        x_target=np.array(mpc.get("x_target", [0.0, 0.0, 0.0, 0.0])), u_min=mpc.get("u_min", -10.0),
        u_max=mpc.get("u_max", 10.0), optimizer_steps=mpc.get("optimizer_steps", 50),
        learning_rate=mpc.get("learning_rate", 0.1), verbose=mpc.get("verbose", False),
        **{k: mpc[k] for k in ("optimizer", "samples", "lam", "sigma", "seed", "elites", "alpha", "sigma_min", "noise",
                                   "gn_line_steps", "gn_box", "mu_init", "mu_min", "mu_max", "mu_up", "mu_down", "terminal")
           if k in mpc})
