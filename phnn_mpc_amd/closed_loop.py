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
  PlantScenario          (all three drivers, scenario=) what makes the plants differ from the model and from each other:
                         per-plant gravity / masses / length, a constant force bias, Gaussian force and measurement
                         noise, and a freeze at termination (include/phnn_mpc.h: phnn_plant_step_ex).
                         The device loop can also keep per-plant metrics (metrics=) and drop the logs (log=False).
  estimator              (all three drivers, estimator=) an estimation.EKF between the measurement and the solve: the
                         controller solves from the estimate xhat instead of the raw float32 measurement, and after every
                         plant step the filter advances with the control the plant applied and the new measurement
                         (phnn_ekf_step).  Only the `measured` components of the measurement are used, so a
                         loop can run on positions alone.  The result gains estimates (T+1,B,4) float32, nis (T,B) and
                         ekf_status (B,), the last step's.  An estimation.DisturbanceEKF also estimates an input
                         disturbance d (phnn_dekf_step): the result gains disturbances (T+1,B,m), and with
                         its compensate the plant is handed c(c(v) - dhat) (phnn_dist_compensate) instead of the command v.
                         An estimation.UKF is the unscented filter on the same state (xhat, P) (phnn_ukf_step; DESIGN.md
                         24): the same results, the step goes through the sigma points instead of a Jacobian.
  track                  (all three drivers, track=) a feedback.Tracking: the solve runs every solve_every-th control step
                         only, and every step applies row step % solve_every of the last plan plus the time-varying LQR
                         feedback on the deviation from its nominal trajectory (phnn_feedback_plan, phnn_feedback_control;
                         DESIGN.md 21).  The result gains track_status (T,B) and track_dev (T,B).
  terminal               (all three drivers) a controller built with terminal= (terminal.TerminalCost: the terminal weight
                         of the Adam and Gauss-Newton solves) solves with it at every step, inside the
                         captured control step too; a controller whose solve has no terminal term refuses it.
"""
import numpy as np

PARAMS = ("gravity", "masscart", "masspole", "length")  # the columns of a (B,4) per-plant parameter array
PLANT_DEFAULTS = dict(gravity=9.8, masscart=1.0, masspole=0.1, length=0.5)
STABILITY_DEFAULTS = dict(tolerance=[0.5, 0.1, 0.5, 0.5], min_duration=1.0)


class PlantScenario:
    """How the B plants of a closed loop differ from the nominal one (the fields of phnn_plant_ex).

    params      (B,4) array of gravity, masscart, masspole, length per plant, or a dict of those names to (B,) arrays or
                scalars (a missing name keeps the plant's shared value); None: the shared plant
    force_bias  (B,) constant force offset per plant (float32), or None
    force_sigma standard deviation of additive Gaussian force noise, drawn afresh at every control step
    meas_sigma  standard deviation of Gaussian noise on the float32 state the controller is handed, one value or four;
                the true state, the logs and the termination test never see it
    seed        key of the noise; plant gid at step s draws from (seed, gid, s) alone.  Use a seed other than the
                controller's sampling seed (MPPI / CEM): the draws share the sampler's counter space
    plant_offset  global id of plant 0 (a batch split over calls or devices draws what the whole batch would)
    freeze_done a plant that has terminated is not stepped any more: its state stays, its metrics stop"""

    def __init__(self, params=None, force_bias=None, force_sigma=0.0, meas_sigma=0.0, seed=0x706C616E74, plant_offset=0,
                 freeze_done=False):
        self.params, self.force_bias = params, force_bias
        self.force_sigma = float(np.float32(force_sigma))
        ms = np.broadcast_to(np.asarray(meas_sigma, dtype=np.float32).reshape(-1), (4,)).copy()
        self.meas_sigma = ms
        if not (self.force_sigma >= 0 and np.isfinite(self.force_sigma) and np.all(ms >= 0) and np.all(np.isfinite(ms))):
            raise ValueError("force_sigma and meas_sigma must be >= 0 and finite")
        self.seed, self.plant_offset, self.freeze_done = int(seed), int(plant_offset), bool(freeze_done)
        if not 0 <= self.seed < 1 << 64 or self.plant_offset < 0:
            raise ValueError("seed must fit 64 bits and plant_offset be >= 0")

    @staticmethod
    def spread(B, rel, rng):
        """(B,4) parameters spread uniformly within +-rel about the defaults: rel one value for all four columns, four
        values (gravity, masscart, masspole, length) or a dict of names (a missing name: no spread); rng a
        numpy Generator.  Every entry lies in [default * (1 - rel), default * (1 + rel)]."""
        if isinstance(rel, dict):
            unknown = set(rel) - set(PARAMS)
            if unknown:
                raise ValueError(f"spread: unknown parameter(s) {sorted(unknown)}")
            rel = [rel.get(k, 0.0) for k in PARAMS]
        rel = np.broadcast_to(np.asarray(rel, dtype=np.float64).reshape(-1), (4,))
        if np.any(rel < 0) or np.any(rel >= 1):
            raise ValueError("spread: 0 <= rel < 1")
        base = np.array([PLANT_DEFAULTS[k] for k in PARAMS])
        lo, hi = base * (1.0 - rel), base * (1.0 + rel)
        return np.clip(base * (1.0 + rel * rng.uniform(-1.0, 1.0, size=(int(B), 4))), lo, hi)

    def params_array(self, B, shared):
        """-> (B,4) float64, or None when the scenario has no per-plant parameters.  shared: the four shared values."""
        if self.params is None:
            return None
        if isinstance(self.params, dict):
            unknown = set(self.params) - set(PARAMS)
            if unknown:
                raise ValueError(f"PlantScenario: unknown parameter(s) {sorted(unknown)}")
            cols = [np.broadcast_to(np.asarray(self.params.get(k, shared[i]), dtype=np.float64).reshape(-1), (B,))
                    for i, k in enumerate(PARAMS)]
            return np.ascontiguousarray(np.stack(cols, axis=1))
        p = np.ascontiguousarray(self.params, dtype=np.float64)
        if p.shape != (B, 4):
            raise ValueError(f"PlantScenario: params must be ({B},4), got {p.shape}")
        return p

    def bias_array(self, B):
        """-> (B,) float32 or None"""
        if self.force_bias is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(self.force_bias, dtype=np.float32).reshape(-1), (B,)))

    @property
    def measured(self):
        return bool(np.any(self.meas_sigma > 0))


class BatchedCartPole:
    def __init__(self, dt=0.02, gravity=9.8, masscart=1.0, masspole=0.1, length=0.5, x_limit=10.0, theta_limit=0.5,
                 scenario=None, replay=None):
        """The defaults are the reference's plant; the other arguments are the fields of phnn_plant (_capi.Plant).
        scenario: a PlantScenario -- per-plant parameters, force bias and noise, measurement noise, freeze; the noise is
        the device plant's, drawn in float64 (noise.plant_normals).  replay: a (T,B) float32 disturbance log (the device
        loop's `disturbance`): step t applies row t instead of computing bias + noise."""
        self.dt = dt
        self.gravity, self.masscart, self.masspole, self.length = gravity, masscart, masspole, length
        self.x_limit, self.theta_limit = x_limit, theta_limit
        self.polemass_length = self.masspole * self.length
        self.total_mass = self.masspole + self.masscart
        self.state = None
        self.scenario = scenario
        self.replay = None if replay is None else np.asarray(replay, dtype=np.float32)
        self.t = 0
        self.disturbance = None  # (B,) float32: what the last step added to the force (with a scenario or a replay)

    def reset(self, initial_states):
        self.state = np.array(initial_states, dtype=np.float64).reshape(-1, 4)
        self.t = 0
        B = self.state.shape[0]
        self._terminated = np.zeros(B, dtype=bool)
        self._bias = None
        sc = self.scenario
        if sc is not None:
            p = sc.params_array(B, (self.gravity, self.masscart, self.masspole, self.length))
            if p is not None:
                self.gravity, self.masscart, self.masspole, self.length = p.T.copy()
                self.polemass_length = self.masspole * self.length
                self.total_mass = self.masspole + self.masscart
            self._bias = sc.bias_array(B)
        return self.state.copy()

    def _disturbance(self, B):
        """-> (B,) float32 added to the force at this step, or None: nothing is added."""
        sc = self.scenario
        if self.replay is not None:
            return self.replay[self.t].reshape(B)
        if sc is None or (self._bias is None and not sc.force_sigma > 0):
            return None
        w = np.zeros(B, np.float32) if self._bias is None else self._bias.copy()
        if sc.force_sigma > 0:
            from .noise import plant_normals
            z0 = plant_normals(sc.seed, self.t, sc.plant_offset + np.arange(B), 0)[:, 0].astype(np.float32)
            w = w + np.float32(sc.force_sigma) * z0
        return w

    def step(self, action):
        """action (B,) or (B,1) forces -> (states (B,4), done (B,) bool)"""
        force = np.asarray(action, dtype=np.float64).reshape(-1)
        self.disturbance = self._disturbance(self.state.shape[0])
        if self.disturbance is not None:
            force = force + self.disturbance.astype(np.float64)
        x, theta, x_dot, theta_dot = self.state.T
        costheta, sintheta = np.cos(theta), np.sin(theta)
        temp = (force + self.polemass_length * theta_dot ** 2 * sintheta) / self.total_mass
        thetaacc = (self.gravity * sintheta - costheta * temp) / (
            self.length * (4.0 / 3.0 - self.masspole * costheta ** 2 / self.total_mass))
        xacc = temp - self.polemass_length * thetaacc * costheta / self.total_mass
        new = np.stack([x + self.dt * x_dot, theta + self.dt * theta_dot, x_dot + self.dt * xacc,
                        theta_dot + self.dt * thetaacc], axis=1)
        if self.scenario is not None and self.scenario.freeze_done:  # terminated on entry: not stepped
            new = np.where(self._terminated[:, None], self.state, new)
        self.state = new
        done = (np.abs(self.state[:, 0]) > self.x_limit) | (np.abs(self.state[:, 1]) > self.theta_limit)
        self._terminated |= done
        self.t += 1
        return self.state.copy(), done

    def measurement(self):
        """The float32 state the controller is handed: float32(state), plus the scenario's measurement noise of the step
        that produced it (none on the initial state)."""
        x32 = self.state.astype(np.float32)
        sc = self.scenario
        if sc is None or not sc.measured or self.t == 0:
            return x32
        from .noise import plant_normals
        z = plant_normals(sc.seed, self.t - 1, sc.plant_offset + np.arange(x32.shape[0]), 1).astype(np.float32)
        on = sc.meas_sigma > 0
        x32[:, on] = x32[:, on] + sc.meas_sigma[on] * z[:, on]
        return x32

    def get_state(self):
        return self.state.copy()


def _track_solve(controller, canonical, x32, u_prev, k, rkw):
    """The solve of a solve step of a loop with tracking -> the sequence that becomes the plan, (B,H,m) on the engine's
    device: an MPCController's last iterate (cold start), a canonical controller's best clamped iterate, warm-started
    from the previous one shifted by k rows (dst[t] = src[t+k], zeros in the last k rows: k shifts by one)."""
    import torch
    if not canonical:
        return controller.solve_batch(x32, **rkw)["u_last"]
    u_init = None
    if u_prev is not None:
        up = u_prev.cpu()
        u_init = torch.cat([up[:, k:], torch.zeros(up.shape[0], k, up.shape[2])], dim=1)
    return controller.optimize_control_batch(x32, u_init, record_costs=False, **rkw)["best_u"]


def run_mpc_batch(simulator, controller, initial_states, num_steps, x_ref=None, scenario=None, estimator=None, track=None):
    """-> dict(states (T+1,B,4), controls (T,B,1), done_step (B,) first step a plant terminated at, or -1).
    x_ref: reference trajectories broadcastable to (B, rows, 4); control step s tracks them from row s.
    scenario: a PlantScenario for the simulator (a BatchedCartPole built with scenario= / replay= has its own); the
    result then also holds disturbance (T,B) float32, what each step added to the commanded force.
    estimator: an estimation.EKF; every solve starts from its estimate, and after every plant step EKF.step advances it
    on the controller's engine with the applied control and the new measurement.  The result then also holds estimates
    (T+1,B,4) float32, nis (T,B) and ekf_status (B,).  An estimation.DisturbanceEKF also estimates an input disturbance:
    the result gains disturbances (T+1,B,m) float32, and with its compensate the simulator is handed
    engine.dist_compensate(u, dhat) -- the controller's (or the tracking law's) control with dhat taken off -- and the
    filter advances with that.
    track: a feedback.Tracking; the solve runs at the steps s with s % solve_every == 0 only, Tracking.plan turns its
    sequence into a plan, and every step applies Tracking.control from the measurement (or the estimate).  The result
    then also holds track_status (T,B) and track_dev (T,B), or None with the tracking's log=False."""
    if track is not None:
        track.check(controller.engine, controller.horizon, controller.dt, getattr(simulator, "dt", None))
    if scenario is not None:
        simulator.scenario = scenario
    measured = hasattr(simulator, "measurement")
    x = simulator.reset(initial_states)
    B = x.shape[0]
    states, controls = [x.copy()], []
    done_step = np.full(B, -1, dtype=np.int64)
    canonical = hasattr(controller, "control_batch")
    u_prev = None
    from .solver import SAMPLING
    sampling = getattr(controller, "optimizer", getattr(controller, "optimizer_type", None)) in SAMPLING
    dist = []
    if estimator is not None:
        import torch
        eng = controller.engine
        start = estimator.start(x, eng.n, eng.m)
        filt = {name: torch.tensor(v, device=eng.device) for name, v in start.items()}  # the state of the running filter
        ekf_opt, ekf_cost = estimator.bind(eng.n, eng.m), estimator.filter_cost(controller._cost(), canonical)
        estimates, nis, ekf_status = [start["xhat"]], [], None
        extra = {name: [start[name]] for name in estimator.log_rows}
    if track is not None:
        import torch
        eng = controller.engine
        track_cost = controller._cost()  # the plan's Q and R, and the bounds of both clamps
        track_status, track_dev = [], []
    for step in range(num_steps):
        rkw = {"epoch": step} if sampling else {}  # the noise counter of an MPPI / CrossEntropy solve: the control step
        if x_ref is not None:
            rkw.update(x_ref=x_ref, ref_offset=step)
        if estimator is not None:
            x32 = filt["xhat"].cpu().numpy()
        else:
            x32 = simulator.measurement() if measured else x.astype(np.float32)
        if track is not None:
            xd = torch.as_tensor(np.ascontiguousarray(x32, dtype=np.float32)).to(eng.device)
            if step % track.solve_every == 0:  # the solve as always; its sequence becomes the plan
                u_prev = seq = _track_solve(controller, canonical, x32, u_prev, track.solve_every, rkw).contiguous()
                plan = track.plan(eng, xd, seq, track_cost, controller.integrator, controller.dt)
            r = track.control(eng, xd, seq, plan, track_cost, step=step)
            u = r["u"].cpu().numpy()
            if track.log:
                track_status.append(r["status"].cpu().numpy().astype(np.int64))
                track_dev.append(r["dev"].cpu().numpy())
        elif canonical:
            u, u_prev, _ = controller.control_batch(x32, u_prev, **rkw)
        else:
            u = controller.compute_control_batch(x32, **rkw)
        if estimator is not None and estimator.compensate:  # the plant is handed c(c(v) - dhat)
            v = torch.as_tensor(np.ascontiguousarray(np.asarray(u, dtype=np.float32).reshape(B, -1))).to(eng.device)
            u = eng.dist_compensate(v, eng.m, filt["dhat"], ekf_cost)[0].cpu().numpy()
        x, done = simulator.step(u)
        newly = done & (done_step < 0)
        done_step[newly] = step
        states.append(x.copy())
        controls.append(np.asarray(u, dtype=np.float64).reshape(B, -1))
        if getattr(simulator, "disturbance", None) is not None:
            dist.append(simulator.disturbance.copy())
        if estimator is not None:  # the filter advances with the control the plant applied and the new measurement
            y32 = simulator.measurement() if measured else x.astype(np.float32)
            r = estimator.step(eng, *filt.values(), torch.as_tensor(np.asarray(u, dtype=np.float32).reshape(B, -1)),
                               torch.tensor(np.ascontiguousarray(y32, dtype=np.float32), device=eng.device), ekf_cost,
                               controller.integrator, controller.dt, opt=ekf_opt)
            filt, ekf_status = {name: r[name] for name in filt}, r["status"]
            for name, rows in extra.items():
                rows.append(filt[name].cpu().numpy())
            estimates.append(filt["xhat"].cpu().numpy())
            nis.append(r["nis"].cpu().numpy())
    out = {"states": np.stack(states), "controls": np.stack(controls), "done_step": done_step}
    if dist:
        out["disturbance"] = np.stack(dist)
    if estimator is not None:
        out.update(estimates=np.stack(estimates), nis=np.stack(nis) if nis else np.zeros((0, B)),
                   ekf_status=None if ekf_status is None else ekf_status.cpu().numpy().astype(np.int64))
        out.update({key: np.stack(extra[name]) for name, key in estimator.log_rows.items()})
    if track is not None:
        kept = track.log
        out.update(track_status=(np.stack(track_status) if track_status else np.zeros((0, B), np.int64)) if kept else None,
                   track_dev=(np.stack(track_dev) if track_dev else np.zeros((0, B))) if kept else None)
    return out


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
    noise run_mpc_batch draws at that step.  A 'CrossEntropy' controller: engine.solve_cem in the same way.  A
    'GaussNewton' controller: engine.solve_gn -- the clamp, the state reset and the set-up K1, then iters x
    (k_rollout_linearize, k_gn_direction, k_gn_candidates, K1, k_gn_select) -- in a workspace kept across the steps; a
    controller with gn_box=True hands box=True on (gn_options), and the direction is k_gn_direction_box.

    x_ref: reference trajectories broadcastable to (B, rows, 4) (engine.reference_view); every solve tracks them from
    row step_dev, the device counter the plant step logs with and the shift advances, so each replay of the captured
    step moves one row along.  The graph reads the reference through a pointer taken here: a float32 tensor on the
    engine's device with a contiguous last dimension is read in place (keep it alive and in place -- the loop holds a
    view of it; values changed in place between runs are seen), anything else is copied once, here.

    scenario: a PlantScenario; the plant step is then k_plant_step_ex (phnn_plant_step_ex), with the step counter as the
    noise step, so eager and replayed runs draw the same noise, and the result holds disturbance (T,B) float32 (what
    each step added to the force; hand it to BatchedCartPole(replay=) to repeat the run on the host).  metrics: True or
    the config's `stability` section (tolerance, min_duration): the plant step also accumulates, per plant, the
    closed-loop cost sum_t e_t^T Q e_t + R u_t^2 (the controller's Q, R and target, float64, on the true states 1..T) and
    the longest run inside the stability band; the result gains cost (B,), longest_run_s (B,) and stable (B,), the
    latter two equal to stability_report over states 0..T.  log=False: the (T+1,B,4) and (T,B) logs are neither
    allocated nor written; states, controls (and disturbance) are None.  With none of the three the loop is what it was.

    estimator: an estimation.EKF.  The plant step then writes its float32 measurement into a buffer of its own (y32), the
    solve reads the estimate (xhat32), and between the plant step and the shift / step advance engine.ekf_step -- the
    control row, K1 with H = 1, its linearisation, k_ekf_update -- advances the estimate with the control the plant
    applied (read in place from the solve's sequence, with the plant's bounds) and y32; all of it inside the captured
    control step.  The result gains estimates (T+1,B,4) float32 and nis (T,B) (None with the estimator's log=False) and
    ekf_status (B,), the last step's.  The filter predicts over the controller's dt: an estimator together with a dt=
    other than controller.dt is refused (ValueError).  Without an estimator the loop is what it was: same launches, same
    bits.  An estimation.DisturbanceEKF: the filter step is engine.dekf_step on (xhat, dhat, Pz), the result gains
    disturbances (T+1,B,m) float32 (None with log=False), and with its compensate engine.dist_compensate turns the
    solve's first control (or the tracking law's output) into u_cmd = c(c(v) - dhat) in a (B,m) buffer that the plant
    step and the filter step read with stride m -- one more launch per control step, inside the captured step.

    track: a feedback.Tracking(solve_every=k).  A solve step (s % k == 0) runs the solve as above, then
    engine.feedback_plan from the same state on the solve's sequence (best_u of a canonical controller, u_last of an
    MPCController, read in place): K1 with trajectories, the linearisation, the LQ backward pass.  Every step, the solve
    step included, runs engine.feedback_control -- row s % k of the plan plus K (x - x_nominal), from the measurement or
    the estimate, the row taken from the step counter --, the plant step (and the filter step) with the control it wrote
    and the step advance; a tracking step runs nothing else.  A canonical controller's next warm start is its best
    sequence shifted k times (made on the solve step, the last shift advancing the step); an MPCController cold-starts
    as always.  With use_graph two graphs are captured, a solve step and a tracking step, and replayed by s % k from the
    host, still with one synchronisation at the end.  The result gains track_status (T,B) and track_dev (T,B) (None with
    the tracking's log=False).  solve_every outside 1 .. horizon and a dt= other than controller.dt are refused
    (ValueError).  Without track the loop is what it was: same launches, same bits.
    """

    def __init__(self, controller, initial_states, num_steps, use_graph=True, dt=None, x_ref=None, scenario=None,
                 metrics=False, log=True, estimator=None, track=None):
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
        self.log_states = self.log_controls = None
        if log:
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
        self.gn = (controller.optimizer if self.canonical else controller.optimizer_type) == "GaussNewton"
        if self.gn and not hasattr(eng, "solve_gn"):
            raise NotImplementedError(f"{type(eng).__name__} has no batched Gauss-Newton solve (RolloutEngine has)")
        if self.gn and x_ref is not None:  # one row set per candidate rollout, expanded once, here
            self.x_ref = eng.mppi_reference(self.x_ref, B, controller.gn_line_steps)
        self.iters = controller.optimizer_steps if self.canonical else controller.max_iterations
        self.lr = controller.learning_rate if self.canonical else controller.lr
        self.lbfgs = not self.canonical and controller.optimizer_type == "LBFGS"
        if not self.canonical and controller.optimizer_type not in ("Adam", "LBFGS", "MPPI", "CrossEntropy", "GaussNewton"):
            raise ValueError(f"Unknown optimizer type: {controller.optimizer_type}")
        if self.lbfgs and not hasattr(eng, "solve_lbfgs"):
            raise NotImplementedError(f"{type(eng).__name__} has no batched L-BFGS solve (RolloutEngine has)")
        # the controller's terminal weight (None: none); its device tensor is read in place by the captured step.  The
        # solves without a terminal term refuse one here (controller.terminal_cost)
        self.terminal = controller.terminal_cost() if hasattr(controller, "terminal_cost") else None
        if self.terminal is not None and not hasattr(eng, "terminal_cost"):
            raise NotImplementedError(f"{type(eng).__name__} has no terminal cost (RolloutEngine has)")
        self.graph = None
        self.use_graph = use_graph and dev.type == "cuda"
        self.ex = self.metrics = None
        self._keep = {}  # the device tensors the two structs point at
        if scenario is not None:
            self._scenario(scenario, log)
        if metrics:
            self._metrics(STABILITY_DEFAULTS if metrics is True else metrics, x)
        self.ekf = estimator
        self.comp = None  # the command the plant takes when a filter's dhat is taken off it
        if estimator is not None:
            self._estimator(estimator, x)
        self.track = track
        if track is not None:
            self._tracking(track)

    def _tracking(self, tr):
        """The buffers of a loop with tracking: the control the plant takes, the plan's workspace, the status and the
        deviation with their logs, and for a canonical controller with solve_every > 1 the scratch of the k-fold shift."""
        torch, eng, B, k = self.torch, self.eng, self.B, self._keep
        tr.check(eng, self.ctl.horizon, self.ctl.dt, self.plant.dt)
        if not hasattr(eng, "feedback_plan"):
            raise NotImplementedError(f"{type(eng).__name__} has no batched plan call (RolloutEngine has)")
        dev = eng.device
        self.seq = None  # the sequence of the last solve: the plan's controls, read in place
        self.fb_ws = {}  # the device buffers of feedback_plan, kept across steps
        k["track_u"] = torch.zeros(B, eng.m, dtype=torch.float32, device=dev)
        k["track_status"] = torch.zeros(B, dtype=torch.int32, device=dev)
        k["track_dev"] = torch.zeros(B, dtype=torch.float64, device=dev)
        self.track_log = {}
        if tr.log:
            k["track_status_log"] = torch.zeros(self.T, B, dtype=torch.int32, device=dev)
            k["track_dev_log"] = torch.zeros(self.T, B, dtype=torch.float64, device=dev)
            self.track_log = dict(log_status=k["track_status_log"], log_dev=k["track_dev_log"])
        if self.canonical and tr.solve_every > 1:
            k["shift"] = [torch.zeros_like(self.u_init) for _ in range(min(tr.solve_every - 1, 2))]

    def _estimator(self, est, x0):
        """The filter's state and buffers: the estimate the solve reads, the covariance, the measurement the plant
        writes, the logs and the options."""
        torch, eng, B, k = self.torch, self.eng, self.B, self._keep
        if self.plant.dt != float(self.ctl.dt):  # the filter predicts over the controller's dt, as the solve does
            raise ValueError(f"estimator: the plant's dt ({self.plant.dt}) differs from the controller's ({self.ctl.dt}); "
                             "the filter's one-step prediction would cover another interval than the plant stepped")
        if not hasattr(eng, est.engine_step):
            raise NotImplementedError(f"{type(eng).__name__} has no batched filter step {est.engine_step} (RolloutEngine has)")
        dev = eng.device
        # the state of the running filter by est.state_names, updated in place by the engine's step
        self.filt = {name: torch.tensor(v, device=dev) for name, v in est.start(x0, eng.n, eng.m).items()}
        if est.compensate:
            k["u_cmd"] = torch.zeros(B, eng.m, dtype=torch.float32, device=dev)
            self.comp = k["u_cmd"]
        self.y32 = self.x32  # the plant keeps writing its measurement here
        self.x32 = self.xhat32 = self.filt["xhat"]  # what every solve reads: the estimate
        self.ekf_opt = est.bind(eng.n, eng.m)
        self.ekf_cost = est.filter_cost(self.cost, self.canonical)
        k["ekf_status"] = torch.zeros(B, dtype=torch.int32, device=dev)
        k["ekf_nis"] = torch.empty(B, dtype=torch.float64, device=dev)
        self.ekf_ws = {}  # the device buffer of the filter step, kept across steps
        self.ekf_log = None
        if est.log:
            k["estimates"] = torch.empty(self.T + 1, B, eng.n, dtype=torch.float32, device=dev)
            k["estimates"][0].copy_(self.xhat32)
            k["nis"] = torch.empty(self.T, B, dtype=torch.float64, device=dev)
            self.ekf_log = dict(log_xhat=k["estimates"], log_nis=k["nis"], step_dev=self.step_dev)
            for name, key in est.log_rows.items():
                k[key] = torch.empty(self.T + 1, *self.filt[name].shape, dtype=self.filt[name].dtype, device=dev)
                k[key][0].copy_(self.filt[name])
                self.ekf_log["log_" + name] = k[key]

    def _applied(self, v, stride):
        """The control the plant takes and its stride: the command v itself, or with a compensating DisturbanceEKF
        c(c(v) - dhat), written by engine.dist_compensate into a (B,m) buffer."""
        if self.comp is None:
            return v, stride
        self.eng.dist_compensate(v, stride, self.filt["dhat"], self.ekf_cost, u_cmd=self.comp)
        return self.comp, self.eng.m

    def _ekf_step(self, u, stride):
        c = self.ctl
        getattr(self.eng, self.ekf.engine_step)(
            *self.filt.values(), u, stride, self.y32, self.ekf_cost, c.integrator, c.dt, self.ekf_opt,
            nis=self._keep["ekf_nis"], innov=False, status=self._keep["ekf_status"], log=self.ekf_log, workspace=self.ekf_ws)

    def _scenario(self, sc, log):
        """Fills self.ex (phnn_plant_ex) from a PlantScenario."""
        torch, dev, B, pl = self.torch, self.eng.device, self.B, self.plant
        from . import _capi
        ex, k = _capi.PlantEx(), self._keep
        params = sc.params_array(B, (pl.gravity, pl.masscart, pl.masspole, pl.length))
        if params is not None:
            k["params"] = torch.tensor(params, dtype=torch.float64, device=dev)
            ex.params_dev = k["params"].data_ptr()
        bias = sc.bias_array(B)
        if bias is not None:
            k["bias"] = torch.tensor(bias, dtype=torch.float32, device=dev)
            ex.force_bias_dev = k["bias"].data_ptr()
        ex.force_sigma = sc.force_sigma
        for i in range(4):
            ex.meas_sigma[i] = float(sc.meas_sigma[i])
        ex.seed, ex.plant_offset, ex.freeze_done = sc.seed, sc.plant_offset, int(sc.freeze_done)
        if log:
            k["disturbance"] = torch.zeros(self.T, B, dtype=torch.float32, device=dev)
            ex.disturbance_log_dev = k["disturbance"].data_ptr()
        self.ex = ex

    def _metrics(self, stab, x0):
        """Fills self.metrics (phnn_plant_metrics) from the controller's cost and a `stability` section; the run counters
        start from the initial state, as stability_report counts it."""
        torch, dev, B = self.torch, self.eng.device, self.B
        from . import _capi
        if self.eng.n != 4 or self.eng.m != 1:
            raise ValueError("closed-loop metrics are the cart-pole's: a 4-state, 1-input model")
        mt, k, cost = _capi.PlantMetrics(), self._keep, self.cost
        for i in range(4):
            for j in range(4):
                mt.Q[4 * i + j] = float(cost.Q[4 * i + j])
            mt.target[i] = float(cost.x_target[i])
        mt.R = float(cost.R[0])
        tol = np.broadcast_to(np.asarray(stab.get("tolerance", STABILITY_DEFAULTS["tolerance"]), dtype=np.float64).reshape(-1), (4,))
        for i in range(4):
            mt.tol[i] = float(tol[i])
        self.need = max(int(np.ceil(stab.get("min_duration", STABILITY_DEFAULTS["min_duration"]) / self.plant.dt)), 1)
        ok0 = np.all(np.abs(x0 - np.array(list(mt.target))) <= tol, axis=1).astype(np.int32)
        k["cost"] = torch.zeros(B, dtype=torch.float64, device=dev)
        k["run"] = torch.tensor(ok0, dtype=torch.int32, device=dev)
        k["best_run"] = k["run"].clone()
        mt.cost_acc_dev, mt.run_dev, mt.best_run_dev = k["cost"].data_ptr(), k["run"].data_ptr(), k["best_run"].data_ptr()
        self.metrics = mt

    def _plant_log(self):
        """The keyword arguments every plant step of the loop takes."""
        log = dict(state_f32=self.x32 if self.ekf is None else self.y32, done_step=self.done_step, step_dev=self.step_dev,
                   log_states=self.log_states, log_controls=self.log_controls)
        if self.ex is not None or self.metrics is not None:
            log.update(ex=self.ex, metrics=self.metrics)
        return log

    def _solve(self):
        """The solve of one control step -> the engine's result dict."""
        eng, c = self.eng, self.ctl
        if self.sampling:
            out = self._solve_sampling()
        elif self.gn:  # self.x_ref is already one row set per candidate rollout (or shared)
            out = eng.solve_gn(self.x32, self.u_init, self.cost, c.integrator, c.dt, record_costs=False, workspace=self.ws,
                               x_ref=self.x_ref, ref_offset=self.step_dev, expanded_ref=True, **c.gn_options())
            out["best_u"] = out["u_last"]  # the cost of a problem never rises: the last iterate is the best one
        elif self.lbfgs:  # the reference's L-BFGS solve
            out = eng.solve_lbfgs(self.x32, self.u_init, self.cost, integrator=c.integrator, dt=c.dt, record_costs=False,
                                  workspace=self.ws, x_ref=self.x_ref, ref_offset=self.step_dev, **c.lbfgs_options())
        else:
            out = eng.solve(self.x32, self.u_init, self.cost, c.integrator, c.dt, lr=self.lr, iters=self.iters,
                            track_best=self.canonical, record_costs=False, workspace=self.ws, x_ref=self.x_ref,
                            ref_offset=self.step_dev, **({} if self.terminal is None else {"terminal": self.terminal}))
        return out

    def _control_step(self):
        eng, c = self.eng, self.ctl
        log = self._plant_log()
        H = self.u_init.shape[1] * self.u_init.shape[2]
        out = self._solve()
        if self.canonical:  # best clamped iterate; next call warm-starts from its shift
            u, stride = self._applied(out["best_u"], H)
            eng.plant_step(self.plant, self.state, u, stride, **log)
            if self.ekf is not None:
                self._ekf_step(u, stride)
            eng.shift_controls(out["best_u"], self.u_init, step_dev=self.step_dev)
        else:  # last iterate, clamp(u_0); every call cold-starts from zeros (u_init stays zero)
            u, stride = self._applied(out["u_last"], H)
            eng.plant_step(self.plant, self.state, u, stride, u_min=c.u_min, u_max=c.u_max, **log)
            if self.ekf is not None:
                self._ekf_step(u, stride)
            eng.advance_step(self.step_dev)

    def _track_step(self, solve):
        """One control step of a loop with tracking.  A solve step (solve=True): the solve as in _control_step, then
        feedback_plan from the same state on the solve's sequence, read in place.  Every step: feedback_control on row
        step % solve_every of the plan, the plant step (and the filter step) with the control it wrote, the step advance.
        A canonical controller's warm start is made on the solve step, all at once: its best sequence shifted
        solve_every times, the last shift advancing the step."""
        eng, c, tr, k = self.eng, self.ctl, self.track, self._keep
        if solve:
            out = self._solve()
            self.seq_before, self.seq = self.seq, out["best_u" if self.canonical else "u_last"]
            eng.feedback_plan(self.x32, self.seq, self.cost, c.integrator, c.dt, mu=tr.mu, workspace=self.fb_ws)
        eng.feedback_control(self.x32, self.seq, self.fb_ws["fb_traj"], self.fb_ws["fb_K"], self.cost, tr.solve_every,
                             step_dev=self.step_dev, u_out=k["track_u"], status=k["track_status"], dev=k["track_dev"],
                             **self.track_log)
        bounds = {} if self.canonical else dict(u_min=c.u_min, u_max=c.u_max)
        u, stride = self._applied(k["track_u"], eng.m)
        eng.plant_step(self.plant, self.state, u, stride, **bounds, **self._plant_log())
        if self.ekf is not None:
            self._ekf_step(u, stride)
        if self.canonical and solve:
            src = self.seq
            for i in range(tr.solve_every):
                last = i == tr.solve_every - 1
                dst = self.u_init if last else k["shift"][i % 2]
                eng.shift_controls(src, dst, step_dev=self.step_dev if last else None)
                src = dst
        else:
            eng.advance_step(self.step_dev)

    def _run_tracking(self):
        """The steps of a loop with tracking: with a graph, the solve step and the tracking step are captured once each
        (the plan row of a tracking step comes from the step counter, so one graph serves them all) and replayed by
        s % solve_every from the host."""
        ke = self.track.solve_every
        if not (self.use_graph and self.T > 1):
            for s in range(self.T):
                self._track_step(s % ke == 0)
            return
        from .solver import capture
        dev = self.eng.device
        self.graph, _ = capture(dev, lambda: self._track_step(True))  # runs step 0
        # the recorded step reads the solve's sequence where the graph will write it; step 0 wrote its own elsewhere
        self.seq.copy_(self.seq_before)
        self.seq_before = None
        self.track_graph = None
        for s in range(1, self.T):
            if s % ke == 0:
                self.graph.replay()
            elif self.track_graph is None:
                self.track_graph, _ = capture(dev, lambda: self._track_step(False))  # runs this step
            else:
                self.track_graph.replay()

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
        if self.track is not None:
            self._run_tracking()
        elif self.use_graph and self.T > 1:
            from .solver import capture
            self.graph, _ = capture(dev, self._control_step)  # runs step 0; replay for steps 1 .. T-1
            for _ in range(1, self.T):
                self.graph.replay()
        else:
            for _ in range(self.T):
                self._control_step()
        torch.cuda.synchronize(dev)
        logged = self.log_states is not None
        out = {"states": self.log_states.cpu().numpy() if logged else None,
               "controls": self.log_controls.cpu().numpy()[:, :, None].astype(np.float64) if logged else None,
               "done_step": self.done_step.cpu().numpy().astype(np.int64)}
        if self.ex is not None:
            out["disturbance"] = self._keep["disturbance"].cpu().numpy() if logged else None
        if self.metrics is not None:
            best = self._keep["best_run"].cpu().numpy().astype(np.int64)
            out.update(cost=self._keep["cost"].cpu().numpy(), longest_run_s=best * self.plant.dt, stable=best >= self.need)
        if self.ekf is not None:
            kept = self.ekf_log is not None
            out.update(estimates=self._keep["estimates"].cpu().numpy() if kept else None,
                       nis=self._keep["nis"].cpu().numpy() if kept else None,
                       ekf_status=self._keep["ekf_status"].cpu().numpy().astype(np.int64))
            out.update({key: self._keep[key].cpu().numpy() if kept else None for key in self.ekf.log_rows.values()})
        if self.track is not None:
            kept = self.track.log
            out.update(track_status=self._keep["track_status_log"].cpu().numpy().astype(np.int64) if kept else None,
                       track_dev=self._keep["track_dev_log"].cpu().numpy() if kept else None)
        return out


def run_mpc_batch_device(controller, initial_states, num_steps, use_graph=True, x_ref=None, scenario=None, metrics=False,
                         log=True, estimator=None, track=None):
    """Device-resident version of run_mpc_batch: same return dict, one host synchronisation at the end.  scenario,
    metrics, log, estimator, track: as in DeviceClosedLoop."""
    return DeviceClosedLoop(controller, initial_states, num_steps, use_graph=use_graph, x_ref=x_ref, scenario=scenario,
                            metrics=metrics, log=log, estimator=estimator, track=track).run()


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
