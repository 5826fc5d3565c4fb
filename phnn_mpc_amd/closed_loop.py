"""Closed-loop receding-horizon drivers for MANY plants at once.

  BatchedCartPole        the reference's ground-truth plant (src/cartpole_simulator.py:63-112: float64, explicit
                         Euler, standard cart-pole equations, termination |x| > 10 or |theta| > 0.5) vectorised over
                         B plants with numpy -- it runs once per control step on the host, like the reference's.
  run_mpc_batch          the loop of scripts/run_cartpole_mpc.py:91-182 / scripts/run_mpc_canonical.py:26-110 for B
                         plants: every control step is ONE batched solve on the GPU (cold start for MPCController,
                         warm start by shift for MPCControllerCanonical), then one plant step.
  run_mpc_batch_device   the same loop with NOTHING on the host: the plant (k_plant_step, float64), the warm-start shift,
                         the logs and the done mask are device kernels, one control step = solve + plant step is
                         captured as a HIP graph and replayed num_steps times; the host synchronises once, at the end.
  x_ref                  (all three drivers) per-plant reference trajectories broadcastable to (B, rows, 4): control
                         step s solves with the window starting at row s (past its end a reference holds its last
                         row) -- the loop index on the host, the device step counter in the device loop.
  noise                  (all three drivers) an MPPI / CrossEntropy controller built with noise= (time-correlated sampling
                         noise, phnn_mpc_amd/noise.py) solves with it at every step: it travels in the controller's
                         mppi_options() / cem_options(), and a captured control step reads its device tensor in place.
  stability_report       the "stability achieved" criterion of scripts/run_cartpole_mpc.py:117-159 with the
                         tolerances of the `stability` config section, per plant.
"""
import numpy as np


class BatchedCartPole:
    def __init__(self, dt=0.02, gravity=9.8, masscart=1.0, masspole=0.1, length=0.5, x_limit=10.0, theta_limit=0.5):
        """The defaults are the reference's plant; the other arguments are the fields of phnn_plant (_capi.Plant)."""
        self.dt = dt
        self.gravity, self.masscart, self.masspole, self.length = gravity, masscart, masspole, length
        self.x_limit, self.theta_limit = x_limit, theta_limit
        self.polemass_length = self.masspole * self.length
        self.total_mass = self.masspole + self.masscart
        self.state = None

    def reset(self, initial_states):
        self.state = np.array(initial_states, dtype=np.float64).reshape(-1, 4)
        return self.state.copy()

    def step(self, action):
        """action (B,) or (B,1) forces -> (states (B,4), done (B,) bool)"""
        force = np.asarray(action, dtype=np.float64).reshape(-1)
        x, theta, x_dot, theta_dot = self.state.T
        costheta, sintheta = np.cos(theta), np.sin(theta)
        temp = (force + self.polemass_length * theta_dot ** 2 * sintheta) / self.total_mass
        thetaacc = (self.gravity * sintheta - costheta * temp) / (
            self.length * (4.0 / 3.0 - self.masspole * costheta ** 2 / self.total_mass))
        xacc = temp - self.polemass_length * thetaacc * costheta / self.total_mass
        self.state = np.stack([x + self.dt * x_dot, theta + self.dt * theta_dot, x_dot + self.dt * xacc,
                               theta_dot + self.dt * thetaacc], axis=1)
        done = (np.abs(self.state[:, 0]) > self.x_limit) | (np.abs(self.state[:, 1]) > self.theta_limit)
        return self.state.copy(), done

    def get_state(self):
        return self.state.copy()


def run_mpc_batch(simulator, controller, initial_states, num_steps, x_ref=None):
    """-> dict(states (T+1,B,4), controls (T,B,1), done_step (B,) first step a plant terminated at, or -1).
    x_ref: reference trajectories broadcastable to (B, rows, 4); control step s tracks them from row s."""
    x = simulator.reset(initial_states)
    B = x.shape[0]
    states, controls = [x.copy()], []
    done_step = np.full(B, -1, dtype=np.int64)
    canonical = hasattr(controller, "control_batch")
    u_prev = None
    from .solver import SAMPLING
    sampling = getattr(controller, "optimizer", getattr(controller, "optimizer_type", None)) in SAMPLING
    for step in range(num_steps):
        rkw = {"epoch": step} if sampling else {}  # the noise counter of an MPPI / CrossEntropy solve: the control step
        if x_ref is not None:
            rkw.update(x_ref=x_ref, ref_offset=step)
        if canonical:
            u, u_prev, _ = controller.control_batch(x.astype(np.float32), u_prev, **rkw)
        else:
            u = controller.compute_control_batch(x.astype(np.float32), **rkw)
        x, done = simulator.step(u)
        newly = done & (done_step < 0)
        done_step[newly] = step
        states.append(x.copy())
        controls.append(np.asarray(u, dtype=np.float64).reshape(B, -1))
    return {"states": np.stack(states), "controls": np.stack(controls), "done_step": done_step}


class DeviceClosedLoop:
    """Closed loop of B cart-poles resident on the engine's GPU (SURVEY.md 8 rows f1 + f3).

    controller: MPCController (cold start, last iterate, clamp(u_0)) or MPCControllerCanonical (warm start by shift,
    best clamped iterate).  One control step enqueues engine.solve -- a copy of the initial iterate, the memsets that
    reset Adam's state, iters x (K1, K2, K3) -- then k_plant_step and k_shift_controls (an MPCController with
    optimizer_type='LBFGS': engine.solve_lbfgs, i.e. the state reset and max_iterations x 20 x (K1, K2, k_lbfgs), then
    k_plant_step); with use_graph the step is captured once and replayed.  Per-plant arithmetic is identical to
    run_mpc_batch (same kernels, same order); the plant differs from the numpy one only by the device's
    double-precision sin/cos.  An MPPI controller (optimizer_type / optimizer 'MPPI'): engine.solve_mppi -- the clamp
    and resets, iters x (k_sample, K1, k_mppi_update) -- with step_dev as the noise epoch, so every replay draws the
    noise run_mpc_batch draws at that step.  A 'CrossEntropy' controller: engine.solve_cem in the same way.

    x_ref: reference trajectories broadcastable to (B, rows, 4) (engine.reference_view); every solve tracks them from
    row step_dev, the device counter the plant step logs with and the shift advances, so each replay of the captured
    step moves one row along.  The graph reads the reference through a pointer taken here: a float32 tensor on the
    engine's device with a contiguous last dimension is read in place (keep it alive and in place -- the loop holds a
    view of it; values changed in place between runs are seen), anything else is copied once, here.
    """

    def __init__(self, controller, initial_states, num_steps, use_graph=True, dt=None, x_ref=None):
        import torch
        from . import _capi
        self.torch, self.ctl = torch, controller
        eng = self.eng = controller.engine
        dev = eng.device
        self.canonical = hasattr(controller, "control_batch")
        x = np.asarray(initial_states, dtype=np.float64).reshape(-1, 4)
        B, H, m = x.shape[0], controller.horizon, 1
        self.B, self.T = B, int(num_steps)
        self.plant = _capi.Plant.default(controller.dt if dt is None else dt)
        self.state = torch.tensor(x, dtype=torch.float64, device=dev)
        self.x32 = self.state.to(torch.float32)  # what the reference hands the controller (float32 of the state)
        self.log_states = torch.empty(self.T + 1, B, 4, dtype=torch.float64, device=dev)
        self.log_states[0].copy_(self.state)
        self.log_controls = torch.empty(self.T, B, dtype=torch.float32, device=dev)
        self.done_step = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.u_init = torch.zeros(B, H, m, dtype=torch.float32, device=dev)
        self.ws = {}  # the engine's buffers of the solve, kept across steps
        self.cost = controller._cost()
        self.x_ref = None
        if x_ref is not None:
            from .engine import reference_view
            self.x_ref = reference_view(x_ref, B, 4, dev)[0]
        from .solver import SAMPLING
        # "mppi" / "cem" for a sampling controller, else None
        self.sampling = SAMPLING.get(controller.optimizer if self.canonical else controller.optimizer_type, (None,))[0]
        if self.sampling and not hasattr(eng, "solve_" + self.sampling):
            raise NotImplementedError(f"{type(eng).__name__} has no batched {self.sampling.upper()} solve (RolloutEngine has)")
        if self.sampling and x_ref is not None:  # one row set per rollout, expanded once, here (samples x the bytes)
            self.x_ref = eng.mppi_reference(self.x_ref, B, controller.samples)
        self.iters = controller.optimizer_steps if self.canonical else controller.max_iterations
        self.lr = controller.learning_rate if self.canonical else controller.lr
        self.lbfgs = not self.canonical and controller.optimizer_type == "LBFGS"
        if not self.canonical and controller.optimizer_type not in ("Adam", "LBFGS", "MPPI", "CrossEntropy"):
            raise ValueError(f"Unknown optimizer type: {controller.optimizer_type}")
        if self.lbfgs and not hasattr(eng, "solve_lbfgs"):
            raise NotImplementedError(f"{type(eng).__name__} has no batched L-BFGS solve (RolloutEngine has)")
        self.graph = None
        self.use_graph = use_graph and dev.type == "cuda"

    def _control_step(self):
        eng, c = self.eng, self.ctl
        log = dict(state_f32=self.x32, done_step=self.done_step, step_dev=self.step_dev, log_states=self.log_states,
                   log_controls=self.log_controls)
        H = self.u_init.shape[1] * self.u_init.shape[2]
        if self.sampling:
            out = self._solve_sampling()
        elif self.lbfgs:  # the reference's L-BFGS solve
            out = eng.solve_lbfgs(self.x32, self.u_init, self.cost, integrator=c.integrator, dt=c.dt, record_costs=False,
                                  workspace=self.ws, x_ref=self.x_ref, ref_offset=self.step_dev, **c.lbfgs_options())
        else:
            out = eng.solve(self.x32, self.u_init, self.cost, c.integrator, c.dt, lr=self.lr, iters=self.iters,
                            track_best=self.canonical, record_costs=False, workspace=self.ws, x_ref=self.x_ref,
                            ref_offset=self.step_dev)
        if self.canonical:  # best clamped iterate; next call warm-starts from its shift
            eng.plant_step(self.plant, self.state, out["best_u"], H, **log)
            eng.shift_controls(out["best_u"], self.u_init, step_dev=self.step_dev)
        else:  # last iterate, clamp(u_0); every call cold-starts from zeros (u_init stays zero)
            eng.plant_step(self.plant, self.state, out["u_last"], H, u_min=c.u_min, u_max=c.u_max, **log)
            eng.advance_step(self.step_dev)

    def _solve_sampling(self):
        """engine.solve_mppi / engine.solve_cem with the step counter as the noise epoch.  self.x_ref is already one row
        set per rollout (or shared): it is handed to the library as it is, not expanded again."""
        eng, c = self.eng, self.ctl
        return getattr(eng, "solve_" + self.sampling)(
            self.x32, self.u_init, self.cost, c.integrator, c.dt, epoch=self.step_dev, record_costs=False, workspace=self.ws,
            x_ref=self.x_ref, ref_offset=self.step_dev, expanded_ref=True, **getattr(c, self.sampling + "_options")())

    def run(self):
        torch = self.torch
        dev = self.eng.device
        if self.use_graph and self.T > 1:
            from .solver import capture
            self.graph, _ = capture(dev, self._control_step)  # runs step 0; replay for steps 1 .. T-1
            for _ in range(1, self.T):
                self.graph.replay()
        else:
            for _ in range(self.T):
                self._control_step()
        torch.cuda.synchronize(dev)
        return {"states": self.log_states.cpu().numpy(), "controls": self.log_controls.cpu().numpy()[:, :, None].astype(np.float64),
                "done_step": self.done_step.cpu().numpy().astype(np.int64)}


def run_mpc_batch_device(controller, initial_states, num_steps, use_graph=True, x_ref=None):
    """Device-resident version of run_mpc_batch: same return dict, one host synchronisation at the end."""
    return DeviceClosedLoop(controller, initial_states, num_steps, use_graph=use_graph, x_ref=x_ref).run()


def stability_report(states, target, tolerance, min_duration, dt):
    """Per plant: was |x_t - target| <= tolerance held for at least min_duration seconds?  states (T+1,B,n)."""
    ok = np.all(np.abs(states - np.asarray(target)) <= np.asarray(tolerance), axis=2)  # (T+1,B)
    need = max(int(np.ceil(min_duration / dt)), 1)
    run = np.zeros(ok.shape[1], dtype=np.int64)
    best = np.zeros(ok.shape[1], dtype=np.int64)
    for t in range(ok.shape[0]):
        run = np.where(ok[t], run + 1, 0)
        best = np.maximum(best, run)
    return {"stable": best >= need, "longest_run_s": best * dt}
