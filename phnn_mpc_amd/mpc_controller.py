"""Drop-in for src/mpc_controller.py: MPCController with the same constructor and methods, solved by the fused
rollout / adjoint / Adam kernels, plus a batched entry point (many plants at once).

Reference behaviour kept:
  - cost sums the state error over t = 0..H inclusive, control effort over t = 0..H-1, optional soft barrier;
  - controls are clamped inside the differentiated closure only when BOTH u_min and u_max are given;
  - every call cold-starts from zeros, runs max_iterations Adam steps and returns clamp(u_0) of the LAST iterate
    as a numpy array of shape (1,).
optimizer_type='LBFGS': compute_control runs the reference's torch.optim.LBFGS on the host (one plant); solve_batch /
compute_control_batch run B such optimizers at once on the device (engine.solve_lbfgs, kernel k_lbfgs).
optimizer_type='MPPI' (not in the reference): the gradient-free sampling solve (engine.solve_mppi): every call
cold-starts the nominal from zeros, runs max_iterations iterations of `samples` perturbed rollouts per plant and returns
clamp(u_0) of the last nominal.  lr is not used.
optimizer_type='CrossEntropy' (not in the reference): the cross-entropy sampling solve (engine.solve_cem), called as
the MPPI one is; returns clamp(u_0) of the last mean.  (The name is not 'CEM': that string stays an unknown optimizer.)
optimizer_type='GaussNewton' (not in the reference): projected Gauss-Newton shooting on the rollout's linearisation
(engine.solve_gn): every call cold-starts from zeros, runs max_iterations iterations (linearise, LQ direction with
Levenberg-Marquardt term mu, gn_line_steps candidates u + 2^-j du in one K1 launch, select) and returns clamp(u_0) of the
last iterate, whose cost never rises from one iteration to the next.  lr is not used.
terminal= (not in the reference): a terminal.TerminalCost, or the config's `terminal` section, adds e_H^T W e_H to the
cost of the 'Adam' and 'GaussNewton' solves; 'LBFGS', 'MPPI' and 'CrossEntropy' refuse one.
"""
import os

import numpy as np
import torch

from . import _capi
from .noise import resolve as resolve_noise
from .solver import SAMPLING, _noise_kw, _terminal_kw, gn_solver_for, lbfgs_solver_for, solver_for
from .terminal import refuse as refuse_terminal
from .terminal import TerminalCost
from .terminal import resolve as resolve_terminal


class MPCController:
    def __init__(self, phnn_model, horizon, dt, Q, R, target_state=None, u_min=None, u_max=None, x_min=None, x_max=None,
                 optimizer_type="Adam", lr=0.1, max_iterations=50, samples=64, lam=1.0, sigma=1.0, seed=0, elites=8,
                 alpha=0.25, sigma_min=0.05, noise=None, gn_line_steps=8, mu_init=1e-6, mu_min=1e-9, mu_max=1e6, mu_up=10.0,
                 mu_down=0.1, gn_box=False, terminal=None):
        self.model = phnn_model
        self.model.eval()
        self.horizon, self.dt = horizon, dt
        self.Q = torch.diag(torch.tensor(Q, dtype=torch.float32)) if isinstance(Q, list) else torch.diag(Q)
        self.R = R
        self.state_dim = phnn_model.J.shape[0]
        if target_state is None:
            self.target_state = torch.zeros(self.state_dim)
        else:
            self.target_state = torch.tensor(target_state, dtype=torch.float32)
        self.u_min, self.u_max = u_min, u_max
        self.x_min = torch.tensor(x_min, dtype=torch.float32) if x_min is not None else None
        self.x_max = torch.tensor(x_max, dtype=torch.float32) if x_max is not None else None
        self.optimizer_type, self.lr, self.max_iterations = optimizer_type, lr, max_iterations
        # optimizer_type='MPPI': samples per plant and iteration, softmin temperature (units of the cost), noise standard
        # deviation, noise seed; `epoch` numbers the solves that are not given one (fresh noise at every control step)
        self.samples, self.lam, self.sigma, self.seed, self.epoch = samples, lam, sigma, seed, 0
        # optimizer_type='CrossEntropy': samples, sigma (the initial standard deviation), seed and epoch as above; elites:
        # how many lowest-cost samples the distribution is refitted to, smoothing alpha in [0, 1), floor of sigma
        self.elites, self.alpha, self.sigma_min = elites, alpha, sigma_min
        # MPPI and CrossEntropy: the time correlation of the sampling noise (noise.resolve: None = white, a noise.Noise,
        # {"type": "ar1" | "colored" | "knots", ...} or an (H, P) array); ValueError for an unknown type or another horizon
        self.noise = resolve_noise(noise, horizon)
        # optimizer_type='GaussNewton': candidates per line search, and the Levenberg-Marquardt term's start, range and factors
        self.gn_line_steps, self.mu_init, self.mu_min, self.mu_max = gn_line_steps, mu_init, mu_min, mu_max
        self.mu_up, self.mu_down = mu_up, mu_down
        # gn_box: the LQ step of every iteration respects u_min / u_max (control-limited DDP)
        self.gn_box = bool(gn_box)
        # terminal weight of the Adam and Gauss-Newton solves: None, a terminal.TerminalCost, or its config section
        # ({type: lqr} is resolved on the engine at the first solve: terminal_cost())
        self.terminal = terminal
        self.integrator = "euler"  # src/mpc_controller.py:137-138
        # True (or PHNN_GRAPH=1): replay the whole solve as one HIP graph instead of 3 x iterations launches
        self.use_graph = os.environ.get("PHNN_GRAPH", "0") == "1"
        self._graphed = None

    # ------------------------------------------------------------------ kernel parameters
    def _solver(self, eng):
        self._graphed = solver_for(eng, self.use_graph, self._graphed)
        return self._graphed

    def _cost(self):
        return _capi.make_cost(self.state_dim, 1, self.Q.numpy(), float(self.R), self.target_state.numpy(),
                               self.u_min, self.u_max,
                               None if self.x_min is None else self.x_min.numpy(),
                               None if self.x_max is None else self.x_max.numpy(), 1000.0)

    def terminal_cost(self):
        """The controller's terminal.TerminalCost, or None.  A config section is resolved here, once (type lqr: the
        linearisation and the DARE iteration run on the engine); a solve without a terminal term refuses one."""
        if self.terminal is None:
            return None
        if self.optimizer_type not in ("Adam", "GaussNewton"):
            refuse_terminal(self.terminal, f"optimizer_type {self.optimizer_type!r}")
        if not isinstance(self.terminal, TerminalCost):  # a config section: resolved once, on the engine
            self.terminal = resolve_terminal(self.terminal, self.engine, self._cost(), self.integrator, self.dt)
        return self.terminal

    def _cost_noclamp(self):
        c = self._cost()
        c.has_u_bounds = 0
        return c

    @property
    def engine(self):
        return self.model.engine

    # ------------------------------------------------------------------ reference methods (B = 1)
    def rollout_dynamics(self, x0, controls):
        """x0 (n,), controls (H,1) -> states (H+1,n); controls are used as given (src/mpc_controller.py:116-141)."""
        eng = self.engine
        x0d = torch.as_tensor(x0, dtype=torch.float32).reshape(1, -1).to(eng.device)
        ud = torch.as_tensor(controls, dtype=torch.float32).reshape(1, -1, 1).to(eng.device)
        _, traj = eng.rollout_cost(x0d, ud, self._cost_noclamp(), self.integrator, self.dt, want_traj=True)
        return traj[0].cpu()

    def feedback_gains(self, x0, u_seq, mu=0.0):
        """Time-varying LQR gains around the planned trajectory: x0 (B,n) or (n,), u_seq (B,H,1) or (H,1) -> dict(K
        (B,H,1,n), P0 (B,n,n), P (B,H+1,n,n), status (B), traj (B,H+1,n), A, Bm), all on the engine's device.  The
        nominal trajectory x^nominal = traj is this controller's rollout of u_seq (its cost, integrator and dt), and the
        law is  delta u_t = K_t (x_t - x_t^nominal),  to be added to u_seq[t] before the clamp.  Three launches: K1 ->
        linearise -> tvlqr.  status[b] != 0: the recursion failed for problem b (its early gains are NaN); mu > 0
        regularises Quu."""
        eng = self.engine
        x0 = torch.as_tensor(x0, dtype=torch.float32).reshape(-1, self.state_dim)
        u = torch.as_tensor(u_seq, dtype=torch.float32).reshape(x0.shape[0], -1, 1)
        cost = self._cost()
        A, Bm, traj = eng.rollout_linearize(x0, u, cost, self.integrator, self.dt)
        out = eng.tvlqr(A, Bm, cost, mu=mu, want_P=True)
        out.update(traj=traj, A=A, Bm=Bm)
        return out

    def compute_cost(self, states, controls):
        """Quadratic cost (+ barrier) of a given trajectory (src/mpc_controller.py:75-114); host arithmetic on
        (H+1,n)/(H,1) tensors -- the kernels fuse the same sum into the march."""
        states = torch.as_tensor(states, dtype=torch.float32)
        controls = torch.as_tensor(controls, dtype=torch.float32)
        e = states[: self.horizon + 1] - self.target_state
        cost = ((e @ self.Q) * e).sum()
        if self.x_min is not None:
            cost = cost + 1000.0 * (torch.relu(self.x_min - states[: self.horizon + 1]) ** 2).sum()
        if self.x_max is not None:
            cost = cost + 1000.0 * (torch.relu(states[: self.horizon + 1] - self.x_max) ** 2).sum()
        return cost + self.R * (controls[: self.horizon] ** 2).sum()

    def compute_control(self, current_state):
        """current_state (n,) -> optimal first control, np.ndarray (1,)   (src/mpc_controller.py:143-209)"""
        if isinstance(current_state, np.ndarray):
            current_state = torch.tensor(current_state, dtype=torch.float32)
        self.terminal_cost()  # refused here by the solves without a terminal term
        if self.optimizer_type == "LBFGS":
            return self._compute_control_lbfgs(current_state)
        u = self.compute_control_batch(current_state.reshape(1, -1))
        return u[0]

    def _compute_control_lbfgs(self, current_state):
        """The reference's L-BFGS branch (src/mpc_controller.py:169-170,196-197): torch.optim.LBFGS(lr, max_iter=20)
        stepped max_iterations times; the closure's cost and gradient come from K1/K2 instead of autograd.  One
        plant at a time (L-BFGS keeps a curvature history per problem)."""
        eng = self.engine
        x0 = current_state.reshape(1, -1).to(eng.device, torch.float32)
        control_sequence = torch.zeros(self.horizon, 1, requires_grad=True)
        optimizer = torch.optim.LBFGS([control_sequence], lr=self.lr, max_iter=20)
        cost_struct, ws = self._cost(), {}

        def closure():
            optimizer.zero_grad()
            c, g = eng.rollout_cost_grad(x0, control_sequence.detach().reshape(1, self.horizon, 1).to(eng.device), cost_struct,
                                         self.integrator, self.dt, workspace=ws)
            control_sequence.grad = g.reshape(self.horizon, 1).to(control_sequence.device).clone()
            return c.reshape(()).to(control_sequence.device).clone()

        for _ in range(self.max_iterations):
            optimizer.step(closure)
        with torch.no_grad():
            u0 = control_sequence[0]
            if self.u_min is not None and self.u_max is not None:
                u0 = torch.clamp(u0, self.u_min, self.u_max)
        return u0.detach().numpy()

    # ------------------------------------------------------------------ batched (new)
    def solve_batch(self, states, record_costs=False, x_ref=None, ref_offset=0, epoch=None):
        """states (B,n) -> dict with the last iterate of B independent problems (all on the engine's device).
        x_ref: per-problem reference trajectories broadcastable to (B, rows, n), tracked from row ref_offset (int or
        device int32 tensor; past its end a reference holds its last row) instead of target_state.
        epoch (MPPI, CrossEntropy): the noise counter of this solve; None: self.epoch, which then advances by one."""
        term = self.terminal_cost()  # refused here by the solves without a terminal term
        if self.optimizer_type == "LBFGS":
            return self._solve_batch_lbfgs(states, record_costs, x_ref, ref_offset)
        if self.optimizer_type in SAMPLING:
            return self._solve_batch_sampling(states, record_costs, x_ref, ref_offset, epoch)
        if self.optimizer_type == "GaussNewton":
            return self._solve_batch_gn(states, record_costs, x_ref, ref_offset)
        if self.optimizer_type != "Adam":
            raise ValueError(f"Unknown optimizer type: {self.optimizer_type}")
        eng = self.engine
        x0 = torch.as_tensor(states, dtype=torch.float32).reshape(-1, self.state_dim).to(eng.device)
        u0 = torch.zeros(x0.shape[0], self.horizon, 1, dtype=torch.float32, device=eng.device)
        return self._solver(eng)(eng, x0, u0, self._cost(), self.integrator, self.dt, self.lr, self.max_iterations,
                                 track_best=False, u_min=self.u_min, u_max=self.u_max, record_costs=record_costs,
                                 x_ref=x_ref, ref_offset=ref_offset, **_terminal_kw(term))

    def lbfgs_options(self):
        """solve_lbfgs keyword arguments of the reference's optimizer: torch.optim.LBFGS([u], lr=self.lr, max_iter=20)
        (torch's defaults for the rest) stepped max_iterations times (src/mpc_controller.py:169-170,196-197)."""
        return dict(lr=self.lr, outer_steps=self.max_iterations, max_iter=20, max_eval=None, tolerance_grad=1e-7,
                    tolerance_change=1e-9, history_size=100)

    def _solve_batch_lbfgs(self, states, record_costs, x_ref, ref_offset):
        """B independent copies of the reference's L-BFGS solve (cold start from zeros) in one batched device solve
        (engine.solve_lbfgs).  Engines without it raise NotImplementedError."""
        eng = self.engine
        if not hasattr(eng, "solve_lbfgs"):
            raise NotImplementedError("L-BFGS keeps a curvature history per problem: this engine has no batched "
                                      "L-BFGS solve (RolloutEngine has); use compute_control (one plant at a time)")
        self._graphed_lbfgs = lbfgs_solver_for(eng, self.use_graph, getattr(self, "_graphed_lbfgs", None))
        x0 = torch.as_tensor(states, dtype=torch.float32).reshape(-1, self.state_dim).to(eng.device)
        u0 = torch.zeros(x0.shape[0], self.horizon, 1, dtype=torch.float32, device=eng.device)
        return self._graphed_lbfgs(x0, u0, self._cost(), integrator=self.integrator, dt=self.dt, record_costs=record_costs,
                                   x_ref=x_ref, ref_offset=ref_offset, **self.lbfgs_options())

    def gn_options(self):
        """solve_gn keyword arguments of this controller."""
        opt = dict(iters=self.max_iterations, line_steps=self.gn_line_steps, mu_init=self.mu_init, mu_min=self.mu_min,
                   mu_max=self.mu_max, mu_up=self.mu_up, mu_down=self.mu_down)
        if self.gn_box:  # present only when set: the plain solve is called as before
            opt["box"] = True
        opt.update(_terminal_kw(self.terminal_cost()))
        return opt

    def _solve_batch_gn(self, states, record_costs, x_ref, ref_offset):
        """B independent Gauss-Newton solves (cold start from zeros) in one batched device solve (engine.solve_gn); the
        workspace stays with the controller."""
        eng = self.engine
        self._graphed_gn = gn_solver_for(eng, self.use_graph, getattr(self, "_graphed_gn", None))
        if getattr(self, "_gn_ws", None) is None:
            self._gn_ws = {}
        x0 = torch.as_tensor(states, dtype=torch.float32).reshape(-1, self.state_dim).to(eng.device)
        u0 = torch.zeros(x0.shape[0], self.horizon, 1, dtype=torch.float32, device=eng.device)
        return self._graphed_gn(eng, x0, u0, self._cost(), self.integrator, self.dt, record_costs=record_costs,
                                workspace=self._gn_ws, x_ref=x_ref, ref_offset=ref_offset, **self.gn_options())

    def mppi_options(self):
        """solve_mppi keyword arguments of this controller."""
        return dict(iters=self.max_iterations, samples=self.samples, lam=self.lam,
                    sigma=tuple(np.asarray(self.sigma, dtype=np.float64).reshape(-1).tolist()), seed=self.seed,
                    **_noise_kw(self.noise))

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

    def cem_options(self):
        """solve_cem keyword arguments of this controller."""
        return dict(iters=self.max_iterations, samples=self.samples, elites=self.elites, alpha=self.alpha,
                    sigma=tuple(np.asarray(self.sigma, dtype=np.float64).reshape(-1).tolist()), sigma_min=self.sigma_min,
                    seed=self.seed, **_noise_kw(self.noise))

    def _solve_batch_sampling(self, states, record_costs, x_ref, ref_offset, epoch):
        """B independent sampling solves, MPPI or cross-entropy (cold start from zeros), in one batched device solve
        (engine.solve_mppi / engine.solve_cem)."""
        eng = self.engine
        meth, graphed_or_eager = SAMPLING[self.optimizer_type]
        solve = graphed_or_eager(eng, self.use_graph, getattr(self, "_graphed_" + meth, None))
        setattr(self, "_graphed_" + meth, solve)
        x0 = torch.as_tensor(states, dtype=torch.float32).reshape(-1, self.state_dim).to(eng.device)
        u0 = torch.zeros(x0.shape[0], self.horizon, 1, dtype=torch.float32, device=eng.device)
        return solve(eng, x0, u0, self._cost(), self.integrator, self.dt, epoch=self._mppi_epoch(eng, epoch),
                     record_costs=record_costs, x_ref=x_ref, ref_offset=ref_offset, **getattr(self, meth + "_options")())

    def compute_control_batch(self, states, x_ref=None, ref_offset=0, epoch=None):
        """states (B,n) -> np.ndarray (B,1): first control of each plant's optimised sequence (x_ref, epoch:
        solve_batch)."""
        kw = {"epoch": epoch} if self.optimizer_type in SAMPLING else {}
        out = self.solve_batch(states, x_ref=x_ref, ref_offset=ref_offset, **kw)
        u0 = out["u_last"][:, 0, :]
        if self.u_min is not None and self.u_max is not None:
            u0 = torch.clamp(u0, self.u_min, self.u_max)
        return u0.cpu().numpy()


def _mppi_keys(mpc):
    """The solver keywords present in the `mpc` config section: samples, lam, sigma, seed, elites, alpha, sigma_min, noise
    (optimizer: MPPI or CrossEntropy), gn_line_steps, gn_box, mu_init, mu_min, mu_max, mu_up, mu_down (GaussNewton) and terminal
    (Adam, GaussNewton: {type: lqr} or {type: matrix, W: [...]})."""
    keys = ("samples", "lam", "sigma", "seed", "elites", "alpha", "sigma_min", "noise", "gn_line_steps", "gn_box", "mu_init", "mu_min",
            "mu_max", "mu_up", "mu_down", "terminal")
    return {k: mpc[k] for k in keys if k in mpc}


def create_mpc_from_config(phnn_model, config):
    """Accepts both key schemas the reference uses: src/mpc_controller.py:212-241 (Q/R/dt/lr/max_iterations) and
    scripts/run_cartpole_mpc.py:57-88 (Q_diag/R_diag/learning_rate/optimizer_steps, dt from config['cartpole'])."""
    mpc = config["mpc"]
    if "Q_diag" in mpc:
        return MPCController(phnn_model=phnn_model, horizon=mpc.get("horizon", 20), dt=config["cartpole"]["dt"],
                             Q=mpc.get("Q_diag", [10.0, 100.0, 1.0, 10.0]), R=mpc.get("R_diag", [0.01])[0],
                             target_state=mpc.get("x_target", [0.0, 0.0, 0.0, 0.0]), u_min=mpc.get("u_min", -10.0),
                             u_max=mpc.get("u_max", 10.0), optimizer_type=mpc.get("optimizer", "Adam"),
                             lr=mpc.get("learning_rate", 0.1), max_iterations=mpc.get("optimizer_steps", 50), **_mppi_keys(mpc))
    return MPCController(phnn_model=phnn_model, horizon=mpc["horizon"], dt=mpc["dt"], Q=mpc["Q"], R=mpc["R"],
                         target_state=mpc.get("target_state", None), u_min=mpc.get("u_min", None),
                         u_max=mpc.get("u_max", None), x_min=mpc.get("x_min", None), x_max=mpc.get("x_max", None),
                         optimizer_type=mpc.get("optimizer", "Adam"), lr=mpc.get("lr", 0.1),
                         max_iterations=mpc.get("max_iterations", 50), **_mppi_keys(mpc))
