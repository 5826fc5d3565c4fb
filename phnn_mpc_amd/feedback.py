"""Tracking the last plan between two solves with its time-varying LQR feedback (include/phnn_mpc.h:
phnn_feedback_plan, phnn_feedback_control).

  Tracking          the settings of a closed loop that solves only every `solve_every`-th control step: on a solve step
                    the solve runs as always and its sequence becomes the plan -- its nominal trajectory and the TV-LQR
                    gains around it are computed once (plan) --, and on every step, the solve step included, the control
                    is row j = step % solve_every of the plan plus the feedback on the deviation from the nominal row
                    (control):  u = clamp(clamp(u_j) + K_j (x - x_j^nominal)).  At j = 0 the deviation is zero and the
                    control is the plan's own, so solve_every = 1 is the plain loop bit for bit.
  Tracking.plan     the Python statement of phnn_feedback_plan over the engine's step methods (rollout_cost with
                    trajectories, rollout_linearize, tvlqr): the same three launches on a RolloutEngine, and it runs on a
                    CPU stand-in that has those methods, the way estimation.EKF.step serves a filter stand-in.
  Tracking.control  engine.feedback_control with this object's solve_every.

The closed-loop drivers (closed_loop.run_mpc_batch, DeviceClosedLoop, run_mpc_batch_device) take track=Tracking(...).
"""
import math

PLAN_METHODS = ("rollout_cost", "rollout_linearize", "tvlqr")


class Tracking:
    """solve_every: k >= 1, the solve runs at the control steps s with s % k == 0 (at most the controller's horizon: the
    plan has that many rows).  mu: the regularisation of Quu in the LQ backward pass (phnn_tvlqr_options.mu; >= 0 and
    finite).  log: the closed-loop drivers record the status and the deviation of every step.
    The TV-LQR of the plan stays on the stage cost: a controller's terminal weight (terminal.TerminalCost) shapes the solve
    that makes the plan, not the gains that track it (P_H = Q + Q^T in the backward pass, with or without one)."""

    def __init__(self, solve_every, mu=0.0, log=True):
        if isinstance(solve_every, bool) or int(solve_every) != solve_every or int(solve_every) < 1:
            raise ValueError(f"solve_every must be an integer >= 1, got {solve_every!r}")
        self.solve_every = int(solve_every)
        self.mu = float(mu)
        if not (self.mu >= 0.0 and math.isfinite(self.mu)):
            raise ValueError(f"mu must be >= 0 and finite, got {mu!r}")
        self.log = bool(log)

    @classmethod
    def from_config(cls, config):
        """A Tracking from the optional `tracking:` section of a config dict (keys: solve_every, mu, log), or None when
        there is no such section."""
        sec = config.get("tracking")
        if sec is None:
            return None
        sec = dict(sec)
        unknown = set(sec) - {"solve_every", "mu", "log"}
        if unknown:
            raise ValueError(f"tracking: unknown key(s) {sorted(unknown)}")
        if "solve_every" not in sec:
            raise ValueError("tracking: solve_every is required")
        return cls(**sec)

    def check(self, engine, horizon, controller_dt=None, plant_dt=None):
        """The refusals of a closed loop with tracking: solve_every outside 1 .. horizon, a plant that steps over another
        interval than the rows of the plan are spaced by (ValueError), an engine without the step methods
        (NotImplementedError)."""
        if not 1 <= self.solve_every <= int(horizon):
            raise ValueError(f"track: solve_every ({self.solve_every}) must lie in 1 .. horizon ({horizon}): the plan has "
                             "one row per step of the horizon")
        if plant_dt is not None and controller_dt is not None and float(plant_dt) != float(controller_dt):
            raise ValueError(f"track: the plant's dt ({plant_dt}) differs from the controller's ({controller_dt}); the "
                             "rows of the plan are spaced by the controller's dt")
        missing = [name for name in PLAN_METHODS + ("feedback_control",) if not hasattr(engine, name)]
        if missing:
            raise NotImplementedError(f"{type(engine).__name__} has no {', '.join(missing)} (RolloutEngine has)")

    def plan(self, engine, x, u, cost, integrator, dt):
        """The nominal trajectory and the gains of the plan (x (B,n), u (B,H,m)), the statement of phnn_feedback_plan
        over the engine's step methods: K1 from x with trajectories and the caller's cost (so the control clamp is
        K1's), the linearisation of that rollout with the cost's bounds, the LQ backward pass with the cost's Q and R.
        -> dict(traj (B,H+1,n) float32, K (B,H,m,n) float64, status (B) int32: phnn_tvlqr's)."""
        _, traj = engine.rollout_cost(x, u, cost, integrator, dt, want_traj=True)
        A, Bm, _ = engine.rollout_linearize(x, u, cost, integrator, dt, traj=traj)
        r = engine.tvlqr(A, Bm, cost, mu=self.mu)
        return dict(traj=traj, K=r["K"], status=r["status"])

    def control(self, engine, x, u, plan, cost, step=0, step_dev=None, **out):
        """The control of this step: engine.feedback_control on row step % solve_every of the plan (u, plan["traj"],
        plan["K"]) from the current measurement or estimate x (B,n); cost: its bounds only.  **out: the optional
        outputs of engine.feedback_control.  -> dict(u (B,m) float32, status (B), dev (B))."""
        return engine.feedback_control(x, u, plan["traj"], plan["K"], cost, self.solve_every, step=step, step_dev=step_dev,
                                       **out)
