"""Model-based state estimation between the measurement and the solve (include/phnn_mpc.h: phnn_ekf_update,
phnn_ekf_step).

  EKF        an extended Kalman filter on the learned model for a measurement that is a selection of state components:
             the prediction is one K1 step, its Jacobian the linearisation of exactly that step, the covariance algebra
             k_ekf_update.  It holds the settings only (which components are measured, Qn, Rn, P0, the initial estimate);
             the state of a running filter -- xhat (B,n) float32 and P (B,n,n) float64 -- belongs to the caller, so one EKF
             serves any number of loops.
  EKF.step   the Python statement of phnn_ekf_step over the engine's step methods (rollout_cost, rollout_linearize,
             ekf_update): the same four launches on a RolloutEngine, and it runs on a CPU stand-in that has those three
             methods, the way solver.gn_solve serves a Gauss-Newton stand-in.

  DisturbanceEKF  the same filter on the state (x, d) with an input disturbance d that enters where the control enters
             (x+ = F(x, c(u) + d), d+ = d; phnn_dekf_update, phnn_dekf_step), and the switch that
             lets the closed loops take dhat off the command (phnn_dist_compensate): offset-free control against a
             constant force bias.

  UKF        the unscented filter on the same state (xhat, P): no Jacobian -- the 2 n + 1 sigma points of (xhat, P) go
             through the real integrator step, clamp and activations included, as K1 rollouts, and the prediction is
             their weighted mean and covariance (phnn_ukf_sigma, phnn_ukf_moments, phnn_ukf_step).
  from_config  the estimator of a config's `estimator:` section, whatever its type.

The closed-loop drivers (closed_loop.run_mpc_batch, DeviceClosedLoop, run_mpc_batch_device) take estimator=EKF(...): the
controller then solves from the estimate instead of the raw measurement.
"""
import numpy as np

from . import _capi


def _square(v, n, what):
    """scalar -> v I, (n,) -> diag(v), (n,n) -> as given; float64."""
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.eye(n) * float(a)
    elif a.ndim == 1:
        a = np.diag(a)
    if a.shape != (n, n):
        raise ValueError(f"{what} must be a scalar, ({n},) or ({n},{n}), got {np.shape(v)}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what} must be finite")
    return np.ascontiguousarray(a)


def _bounds(cost):
    """What a prediction takes from a cost, the clamp: a zero _capi.Cost with the cost's bounds (None: without bounds)."""
    bounds = _capi.Cost()
    if cost is not None:
        bounds.has_u_bounds, bounds.u_min, bounds.u_max = cost.has_u_bounds, cost.u_min, cost.u_max
    return bounds


def _copy_noise(dst, src, n):
    """meas_mask, Qn and Rn of an n-state model from one options struct to another -> dst."""
    dst.meas_mask = src.meas_mask
    for i in range(n * n):
        dst.Qn[i] = src.Qn[i]
    for i in range(n):
        dst.Rn[i] = src.Rn[i]
    return dst


class EKF:
    """measured: indices of the measured state components (no duplicates; () = predict only).  Qn: process noise
    covariance added at every step -- a scalar (times I), a diagonal or a full (n,n) matrix.  Rn: measurement noise
    VARIANCES -- a scalar, or one value per state component (n,) or per measured component (len(measured),); positive
    and finite where measured.  P0: the initial covariance, like Qn.  x0_hat: the initial estimate, broadcastable to
    (B,n); None = float32 of the true initial state.  log: the closed-loop drivers record the estimates and the nis of
    every step.

    What the closed-loop drivers use of a filter, and all they know of it:
      state_names   the tensors of a running filter, in the order step and the engine's device step take them
      start(x0, n, m)  -> their initial values, a dict of numpy arrays by those names
      bind(n, m)    -> the options struct of an n-state, m-input model
      filter_cost(cost, canonical)  -> the cost whose bounds the filter clamps with, or None
      engine_step   the name of the engine's device step
      log_rows      the extra per-step logs, {state name: key of the drivers' result}
      compensate    the drivers hand the plant engine.dist_compensate(u, dhat) instead of u
      step, log     below"""

    state_names = ("xhat", "P")
    engine_step = "ekf_step"
    log_rows = {}
    compensate = False

    def __init__(self, measured=(0, 1), Qn=1e-6, Rn=1e-4, P0=1e-2, x0_hat=None, log=True):
        self.measured = tuple(int(i) for i in measured)
        if len(set(self.measured)) != len(self.measured) or any(i < 0 or i >= _capi.PHNN_MAX_N for i in self.measured):
            raise ValueError(f"measured: distinct component indices in 0 .. {_capi.PHNN_MAX_N - 1}, got {measured}")
        self.Qn, self.Rn, self.P0 = Qn, Rn, P0
        self.x0_hat = None if x0_hat is None else np.asarray(x0_hat, dtype=np.float32)
        self.log = bool(log)

    @classmethod
    def from_config(cls, config):
        """An EKF from the optional `estimator:` section of a config dict (keys: measured, Qn, Rn, P0, x0_hat, log; type:
        "ekf" may be given), a DisturbanceEKF for type "ekf_disturbance", or None when there is no such section: the
        module's from_config with these two types."""
        return from_config(config, types=("ekf", "ekf_disturbance"))

    @property
    def mask(self):
        return sum(1 << i for i in self.measured)

    def rn_vector(self, n):
        """-> (n,) float64 variances, 0 at unmeasured components."""
        r = np.asarray(self.Rn, dtype=np.float64).reshape(-1)
        out = np.zeros(n)
        idx = list(self.measured)
        if r.size == 1:
            out[idx] = r[0]
        elif r.size == n:
            out[idx] = r[idx]
        elif r.size == len(idx):
            out[idx] = r
        else:
            raise ValueError(f"Rn must be a scalar, ({n},) or ({len(idx)},), got {r.shape}")
        if not (np.all(out[idx] > 0) and np.all(np.isfinite(out[idx]))):
            raise ValueError("Rn must be positive and finite at the measured components")
        return out

    def _fill(self, o, n):
        """meas_mask, Qn and Rn of an n-state model into an options struct that has them -> o."""
        if any(i >= n for i in self.measured):
            raise ValueError(f"measured {self.measured}: the model has {n} state components")
        o.meas_mask = self.mask
        Qn, Rn = _square(self.Qn, n, "Qn"), self.rn_vector(n)
        for i in range(n):
            for j in range(n):
                o.Qn[i * n + j] = Qn[i, j]
            o.Rn[i] = Rn[i]
        return o

    def options(self, n):
        """-> _capi.EkfOptions (phnn_ekf_options) for an n-state model."""
        return self._fill(_capi.EkfOptions(), n)

    def bind(self, n, m):
        return self.options(n)

    def start(self, x0, n, m):
        return dict(zip(self.state_names, self.initial(x0, n)))

    def filter_cost(self, cost, canonical):
        """The plant's clamp; a canonical controller's sequence is clamped already."""
        return None if canonical else cost

    def initial(self, x0, n=None):
        """x0 (B,n) true initial states -> (xhat0 (B,n) float32, P0 (B,n,n) float64), numpy."""
        x0 = np.asarray(x0, dtype=np.float64)
        B, n = x0.shape[0], x0.shape[1] if n is None else n
        xh = x0.astype(np.float32) if self.x0_hat is None else np.broadcast_to(self.x0_hat, (B, n)).astype(np.float32)
        P = np.broadcast_to(_square(self.P0, n, "P0"), (B, n, n))
        return np.ascontiguousarray(xh), np.ascontiguousarray(P)

    def step(self, engine, xhat, P, u, y, cost, integrator, dt, opt=None, log=None):
        """One filter step, the statement of phnn_ekf_step over the engine's step methods.  xhat (B,n) float32, P
        (B,n,n) float64, u (B,m) or (B,1,m) the applied control, y (B,n) float32 (only the measured components matter),
        tensors on the engine's device; cost: its bounds clamp the control as K1 and the plant do (None: no clamp).
        -> dict(xhat, P, nis, innov, status); xhat and P are new tensors, the inputs keep their values."""
        import torch
        B = xhat.shape[0]
        opt = self.options(engine.n) if opt is None else opt
        row = torch.as_tensor(u, dtype=torch.float32).to(engine.device).reshape(B, 1, engine.m).contiguous()
        bounds = _bounds(cost)
        _, traj = engine.rollout_cost(xhat, row, bounds, integrator, dt, want_traj=True)
        A, _, _ = engine.rollout_linearize(xhat, row, bounds, integrator, dt, traj=traj)
        return engine.ekf_update(traj[:, 1].contiguous(), A.reshape(B, engine.n, engine.n), y, P.clone(), opt, log=log)


class DisturbanceEKF(EKF):
    """EKF on the augmented state z = (x, d): d (m components) is an input disturbance, constant in the model, that adds
    to the clamped command.  measured, Qn, Rn, P0, x0_hat, log: as in EKF (the measurement is a selection of STATE
    components).  Qd: the process noise covariance of d and Pd0 its initial covariance -- a scalar, (m,) or (m,m); Qz:
    optionally the full (n+m, n+m) process noise covariance, which then replaces Qn and Qd.  d0_hat: the initial
    disturbance estimate, broadcastable to (B,m).  compensate: the closed-loop drivers hand the plant
    c(c(v) - dhat) instead of the controller's command v (engine.dist_compensate); False: the plain loop's control, the
    disturbance is estimated only."""

    state_names = ("xhat", "dhat", "P")
    engine_step = "dekf_step"
    log_rows = {"dhat": "disturbances"}

    def __init__(self, measured=(0, 1), Qn=1e-6, Rn=1e-4, P0=1e-2, Qd=0.0, Pd0=1.0, Qz=None, x0_hat=None, d0_hat=0.0,
                 compensate=True, log=True):
        super().__init__(measured=measured, Qn=Qn, Rn=Rn, P0=P0, x0_hat=x0_hat, log=log)
        self.Qd, self.Pd0, self.Qz = Qd, Pd0, Qz
        self.d0_hat = np.asarray(d0_hat, dtype=np.float32)
        self.compensate = bool(compensate)

    def options(self, n, m):
        """-> _capi.DekfOptions (phnn_dekf_options) for an n-state, m-input model."""
        if any(i >= n for i in self.measured):
            raise ValueError(f"measured {self.measured}: the model has {n} state components")
        nz = n + m
        if nz > _capi.PHNN_DEKF_MAX_Z:
            raise ValueError(f"n + m = {nz}: the disturbance filter holds at most {_capi.PHNN_DEKF_MAX_Z} components")
        if self.Qz is not None:
            Qz = _square(self.Qz, nz, "Qz")
        else:
            Qz = np.zeros((nz, nz))
            Qz[:n, :n], Qz[n:, n:] = _square(self.Qn, n, "Qn"), _square(self.Qd, m, "Qd")
        o = _capi.DekfOptions()
        o.meas_mask = self.mask
        Rn = self.rn_vector(n)
        for i in range(nz * nz):
            o.Qz[i] = Qz.reshape(-1)[i]
        for i in range(n):
            o.Rn[i] = Rn[i]
        return o

    def bind(self, n, m):
        return self.options(n, m)

    def start(self, x0, n, m):
        return dict(zip(self.state_names, self.initial(x0, m, n)))

    def filter_cost(self, cost, canonical):
        """The bounds of the command's clamps, in the compensation and in the filter."""
        return cost

    def initial(self, x0, m, n=None):
        """x0 (B,n) true initial states -> (xhat0 (B,n) float32, dhat0 (B,m) float32, Pz0 (B,n+m,n+m) float64 =
        blockdiag(P0, Pd0)), numpy."""
        xh, P = super().initial(x0, n)
        B, n = xh.shape
        Pz = np.zeros((B, n + m, n + m))
        Pz[:, :n, :n], Pz[:, n:, n:] = P, _square(self.Pd0, m, "Pd0")
        return xh, np.ascontiguousarray(np.broadcast_to(self.d0_hat, (B, m)).astype(np.float32)), Pz

    def step(self, engine, xhat, dhat, Pz, u, y, cost, integrator, dt, opt=None, log=None):
        """One filter step, the statement of phnn_dekf_step over the engine's step methods.  xhat (B,n) and dhat (B,m)
        float32, Pz (B,n+m,n+m) float64, u (B,m) or (B,1,m) the applied command, y (B,n) float32, tensors on the engine's
        device; cost: its bounds clamp the command (None: no clamp) -- the model itself runs without bounds on c(u) + dhat.
        -> dict(xhat, dhat, P, nis, innov, status); xhat, dhat and P are new tensors, the inputs keep their values."""
        import torch
        B, n, m = xhat.shape[0], engine.n, engine.m
        opt = self.options(n, m) if opt is None else opt
        cu = torch.as_tensor(u, dtype=torch.float32).to(engine.device).reshape(B, m)
        if cost is not None and cost.has_u_bounds:
            if cost.u_min > cost.u_max:
                raise ValueError("u_min > u_max")
            cu = torch.clamp(cu, float(cost.u_min), float(cost.u_max))  # a NaN stays NaN
        row = (cu + dhat.reshape(B, m)).reshape(B, 1, m).contiguous()
        _, traj = engine.rollout_cost(xhat, row, _bounds(None), integrator, dt, want_traj=True)  # a zero cost, no bounds
        A, Bm, _ = engine.rollout_linearize(xhat, row, None, integrator, dt, traj=traj)
        return engine.dekf_update(traj[:, 1].contiguous(), A.reshape(B, n, n), Bm.reshape(B, n, m), y, Pz.clone(),
                                  dhat.clone().reshape(B, m), opt, log=log)


class UKF(EKF):
    """Unscented Kalman filter with additive process noise on the EKF's state (xhat (B,n) float32, P (B,n,n) float64),
    n in {2, 3, 4}.  measured, Qn, Rn, P0, x0_hat, log: as in EKF.  alpha, beta, kappa: the scaled unscented transform,
    lambda = alpha^2 (n + kappa) - n, gamma = sqrt(n + lambda), wm0 = lambda / (n + lambda), wc0 = wm0 + (1 - alpha^2 +
    beta), wi = 1 / (2 (n + lambda)), computed here in float64; the library sees gamma and the weights only.

    The defaults (1, 0, 1) are deliberate and not the textbook alpha = 1e-3: the sigma points and their images are
    float32 (K1 is), and with a small alpha the spread gamma sqrt(P) sinks into the rounding of xhat.  Deviation of P
    from the Kalman filter's P on a linear system (n = 4, positions measured, 60 steps of
    tests/ekf_model.consistency_system, CPU model of the kernels):
        (alpha, beta, kappa) = (1, 0, 1)      3.0e-7
                               (0.1, 2, 0)    3.6e-6
                               (1e-3, 2, 0)   4.2e-1
    P must stay positive definite: a problem whose P has no Cholesky factor ends its step with status 2 and NaN."""

    engine_step = "ukf_step"

    def __init__(self, measured=(0, 1), Qn=1e-6, Rn=1e-4, P0=1e-2, x0_hat=None, log=True, alpha=1.0, beta=0.0, kappa=1.0):
        super().__init__(measured=measured, Qn=Qn, Rn=Rn, P0=P0, x0_hat=x0_hat, log=log)
        self.alpha, self.beta, self.kappa = float(alpha), float(beta), float(kappa)

    def weights(self, n):
        """-> (gamma, wm0, wc0, wi) in float64 for n state components."""
        a2 = self.alpha * self.alpha
        lam = a2 * (n + self.kappa) - n
        c = n + lam
        if not (np.isfinite(c) and c > 0.0):
            raise ValueError(f"alpha = {self.alpha}, kappa = {self.kappa}: n + lambda = {c} must be positive and finite")
        wm0 = lam / c
        return float(np.sqrt(c)), float(wm0), float(wm0 + (1.0 - a2 + self.beta)), float(1.0 / (2.0 * c))

    def options(self, n):
        """-> _capi.UkfOptions (phnn_ukf_options) for an n-state model."""
        if n > _capi.PHNN_UKF_MAX_N:
            raise ValueError(f"n = {n}: the unscented filter holds at most {_capi.PHNN_UKF_MAX_N} state components")
        o = self._fill(_capi.UkfOptions(), n)
        o.gamma, o.wm0, o.wc0, o.wi = self.weights(n)
        return o

    def initial(self, x0, n=None):
        """EKF.initial; a P0 that is not positive definite is refused (the filter factors P at every step)."""
        xh, P = super().initial(x0, n)
        if P.shape[0]:
            try:
                np.linalg.cholesky(P[0])
            except np.linalg.LinAlgError:
                raise ValueError("P0 must be positive definite") from None
        return xh, P

    def step(self, engine, xhat, P, u, y, cost, integrator, dt, opt=None, log=None):
        """One filter step, the statement of phnn_ukf_step over the engine's methods (ukf_sigma, rollout_cost,
        ukf_moments, ekf_update); arguments and result as in EKF.step."""
        import torch
        B, n, m = xhat.shape[0], engine.n, engine.m
        S = 2 * n + 1
        opt = self.options(n) if opt is None else opt
        row = torch.as_tensor(u, dtype=torch.float32).to(engine.device).reshape(B, m).contiguous()
        bounds = _bounds(cost)
        chi, ctrl = engine.ukf_sigma(xhat, P, opt, u=row)
        _, traj = engine.rollout_cost(chi.reshape(B * S, n), ctrl.reshape(B * S, 1, m), bounds, integrator, dt, want_traj=True)
        mo = engine.ukf_moments(traj[:, 1].contiguous(), B, opt)
        e = _copy_noise(_capi.EkfOptions(), opt, n)  # the update's share of the options
        return engine.ekf_update(mo["xm"], mo["eye"], y, mo["Pm"], e, log=log)


_KEYS = {"measured", "Qn", "Rn", "P0", "x0_hat", "log"}  # of every estimator
_TYPES = {"ekf": (EKF, set()),
          "ekf_disturbance": (DisturbanceEKF, {"Qd", "Pd0", "Qz", "d0_hat", "compensate"}),
          "ukf": (UKF, {"alpha", "beta", "kappa"})}  # type -> (class, the keys it adds)


def from_config(config, types=tuple(_TYPES)):
    """The estimator of the optional `estimator:` section of a config dict, or None without one: the class of its
    `type` (default "ekf") in the table above, built from the section's other keys.  types: the types accepted."""
    sec = config.get("estimator")
    if sec is None:
        return None
    sec = dict(sec)
    kind = str(sec.pop("type", "ekf")).lower()
    if kind not in types:
        raise ValueError(f"Unknown estimator type: {kind}")
    cls, extra = _TYPES[kind]
    unknown = set(sec) - _KEYS - extra
    if unknown:
        raise ValueError(f"estimator: unknown key(s) {sorted(unknown)}")
    return cls(**sec)
