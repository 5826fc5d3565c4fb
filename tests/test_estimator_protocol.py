"""The surface the closed-loop drivers use of an estimator (estimation.EKF's docstring), without a
GPU: a filter the drivers have never seen runs through run_mpc_batch on that surface alone, and for the three shipped
filters the surface says what the per-class methods and the drivers' former choices said."""
import re

import numpy as np
import pytest
import torch

import ekf_model as em
import oracle_lib as ol
from phnn_mpc_amd import _capi, estimation
from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch
from phnn_mpc_amd.estimation import EKF, UKF, DisturbanceEKF
from phnn_mpc_amd.models import pHNN
from phnn_mpc_amd.mpc_controller import MPCController
from test_ekf_model import CFG, X0


class MeasurementAsEstimate(EKF):
    """The estimate is the measurement: nothing but step, and that without the engine."""

    def step(self, engine, xhat, P, u, y, cost, integrator, dt, opt=None, log=None):
        B = xhat.shape[0]
        return dict(xhat=y.to(torch.float32), P=P, nis=torch.zeros(B, dtype=torch.float64),
                    status=torch.zeros(B, dtype=torch.int32))


def test_a_filter_the_drivers_have_never_seen():
    w = ol.load_weights("phnn_cartpole")
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    ctl = MPCController(phnn_model=m.set_engine(em.EkfOracleEngine(w)), horizon=5, dt=0.02, Q=[10.0, 100.0, 1.0, 10.0], R=0.01,
                        u_min=-10.0, u_max=10.0, optimizer_type="Adam", lr=0.1, max_iterations=3)
    plain = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2)
    out = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, estimator=MeasurementAsEstimate())
    # without measurement noise the measurement is float32(x): what the solve reads without an estimator
    for k in ("states", "controls", "done_step"):
        assert out[k].dtype == plain[k].dtype and np.array_equal(out[k], plain[k]), k
    assert out["estimates"].dtype == np.float32 and np.array_equal(out["estimates"][0], X0.astype(np.float32))
    assert np.array_equal(out["estimates"][1:], out["states"][1:].astype(np.float32))
    assert set(out) == {"states", "controls", "done_step", "estimates", "nis", "ekf_status"}
    assert not out["nis"].any() and not out["ekf_status"].any()


FILTERS = [(EKF, {}, (4, 1)), (EKF, {}, (2, 1)), (EKF, {}, (4, 2)),
           (DisturbanceEKF, dict(Qd=1e-6), (4, 1)), (DisturbanceEKF, dict(Qd=1e-6), (2, 1)), (DisturbanceEKF, dict(Qd=1e-6), (4, 2)),
           (UKF, {}, (4, 1))]


@pytest.mark.parametrize("cls,kw,nm", FILTERS, ids=[f"{c.__name__}-{n}x{m}" for c, _, (n, m) in FILTERS])
def test_the_protocol_equals_the_per_class_surface(cls, kw, nm):
    n, m = nm
    est = cls(Qn=[1e-8, 1e-5] * (n // 2), Rn=[1e-4, 2.5e-5], P0=1e-3, **kw)
    augmented = cls is DisturbanceEKF
    x0 = np.random.default_rng(3).standard_normal((5, n))
    # bind = options, start = initial, each called with the arity of its class
    old_opt = est.options(n, m) if augmented else est.options(n)
    assert type(est.bind(n, m)) is type(old_opt) and bytes(est.bind(n, m)) == bytes(old_opt)
    old_state = est.initial(x0, m) if augmented else est.initial(x0)
    state = est.start(x0, n, m)
    assert tuple(state) == est.state_names == (("xhat", "dhat", "P") if augmented else ("xhat", "P"))
    assert len(old_state) == len(state)
    for a, b in zip(state.values(), old_state):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    # the clamp cost: the drivers gave the EKF and the UKF None with a canonical controller, the disturbance filter the cost
    cost = _capi.make_cost(n, m, [1.0] * n, 0.01, None, -10.0, 10.0)
    assert est.filter_cost(cost, False) is cost
    assert est.filter_cost(cost, True) is (cost if augmented else None)
    # the device step, the extra log and the compensation
    assert est.engine_step == {EKF: "ekf_step", DisturbanceEKF: "dekf_step", UKF: "ukf_step"}[cls]
    assert est.log_rows == ({"dhat": "disturbances"} if augmented else {})
    assert est.compensate is augmented
    if augmented:
        assert cls(compensate=False, **kw).compensate is False


def test_one_from_config_for_every_type():
    base = {"measured": [0], "Rn": 1e-3}
    for kind, cls, extra in ((None, EKF, {}), ("ekf", EKF, {}), ("ekf_disturbance", DisturbanceEKF, {"Qd": 1e-6, "compensate": False}),
                             ("ukf", UKF, {"alpha": 0.5})):
        sec = dict(base, **extra, **({} if kind is None else {"type": kind}))
        e = estimation.from_config({"estimator": sec})
        assert type(e) is cls and e.measured == (0,) and e.Rn == 1e-3
        for k, v in extra.items():
            assert getattr(e, k) == v
    assert estimation.from_config({"mpc": {}}) is None and EKF.from_config({"mpc": {}}) is None
    assert type(EKF.from_config({"estimator": {"type": "ekf_disturbance"}})) is DisturbanceEKF
    with pytest.raises(ValueError, match="^" + re.escape("Unknown estimator type: mhe") + "$"):
        estimation.from_config({"estimator": {"type": "mhe"}})
    for kind, key in (("ekf", "alpha"), ("ukf", "Qd"), ("ekf_disturbance", "kappa")):  # a key of another type
        with pytest.raises(ValueError, match="^" + re.escape(f"estimator: unknown key(s) ['{key}', 'measure']") + "$"):
            estimation.from_config({"estimator": {"type": kind, key: 1.0, "measure": [0]}})
