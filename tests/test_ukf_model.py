"""The unscented Kalman filter without a GPU: the stated operation order (ukf_model.sigma,
ukf_model.moments) against numpy.linalg, the exactness of the transform, its equivalence with the Kalman filter on linear
systems, failures and isolation, estimation.UKF on the CPU stand-in, the closed loop with it, the configuration entry
point and the structs against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dekf_model as dm
import ekf_model as em
import oracle_lib as ol
import ukf_model as um
from phnn_mpc_amd import _capi, estimation
from phnn_mpc_amd.closed_loop import BatchedCartPole, PlantScenario, run_mpc_batch
from phnn_mpc_amd.estimation import EKF, UKF, DisturbanceEKF
from phnn_mpc_amd.models import pHNN
from phnn_mpc_amd.mpc_controller import MPCController

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")

# DESIGN.md section 18's rule: the deviation measured on the test's own inputs, asserted at 64 x that figure and never
# above 1e-8 for the float64 quantities.  Measured (printed by the tests):
MARGIN, CEILING = 64.0, 1e-8
# stated order against numpy.linalg: L 1.11e-16, Pm 1.11e-16.  The mean came out equal to einsum's, 0.0; a sum of up to
# nine terms in another order may differ by an ulp of its largest partial sum (|x-| < 4: 4.4e-16), which is the figure taken
MEASURED_L, MEASURED_PM, MEASURED_MEAN = 1.2e-16, 1.2e-16, 4.4e-16
# Y = chi: what the float32 rounding of the sigma points leaves of (xhat, P): 1.99e-8 / 4.22e-8, the textbook moments of
# the same chi the same to the printed digits
MEASURED_BACK_X, MEASURED_BACK_P = 2.0e-8, 4.3e-8
MEASURED_QUAD = 1.3e-7  # mean of x + c x^2 (float32 images) against the analytic second-order value; the textbook moments the same
W = um.weights  # (gamma, wm0, wc0, wi)


def bound(measured):
    return min(MARGIN * measured, CEILING)


def _cases():
    return [(n, name, seed) for n in (2, 3, 4) for name in em.MASKS[n] for seed in (0, 1, 2)]


def _images(p, chi):
    """The sigma points through the problem's own linear map A (float64), rounded to float32."""
    return np.einsum("bij,bkj->bki", p["A"].astype(np.float64), chi.astype(np.float64)).astype(np.float32)


# ----------------------------------------------------------------------------- against numpy.linalg
def test_the_stated_order_against_numpy_linalg():
    worst = dict(L=0.0, Pm=0.0, mean=0.0)
    for n, name, seed in _cases():
        p = em.seeded_problem(100 * n + seed, 33, n, em.MASKS[n][name])
        g, wm0, wc0, wi = W(n)
        s = um.sigma(p["xpred"], p["P"], g)
        assert not s["fail"].any()
        chi_t, L_t = um.textbook_sigma(p["xpred"], p["P"], g)
        worst["L"] = max(worst["L"], float(np.abs(s["L"] - L_t).max()))
        # chi: bit-equal to the float32 rounding of the stated order's own float64 values
        x = p["xpred"].astype(np.float64)
        assert np.array_equal(s["chi"][:, 0], p["xpred"])
        for c in range(n):
            assert np.array_equal(s["chi"][:, 1 + c], (x + g * s["L"][:, :, c]).astype(np.float32))
            assert np.array_equal(s["chi"][:, 1 + n + c], (x - g * s["L"][:, :, c]).astype(np.float32))
        assert np.abs(s["chi"] - chi_t).max() <= 2.0 ** -23 * max(1.0, np.abs(chi_t).max())
        Y = _images(p, s["chi"])
        m = um.moments(Y, wm0, wc0, wi)
        xm_t, Pm_t = um.textbook_moments(Y, wm0, wc0, wi)
        worst["Pm"] = max(worst["Pm"], float(np.abs(m["Pm"] - Pm_t).max()))
        worst["mean"] = max(worst["mean"], float(np.abs(m["xm64"] - xm_t).max()))
        assert np.array_equal(m["xm"], m["xm64"].astype(np.float32)), "rounded once"
        assert np.array_equal(m["Pm"], np.swapaxes(m["Pm"], 1, 2)) and np.all(np.linalg.eigvalsh(m["Pm"]) > 0)
        assert np.array_equal(m["eye"], np.broadcast_to(np.eye(n, dtype=np.float32), (33, n, n)))
    print(f"\nmodel vs numpy.linalg: L {worst['L']:.2e}, Pm {worst['Pm']:.2e}, mean {worst['mean']:.2e}")
    assert worst["L"] <= bound(MEASURED_L) and worst["Pm"] <= bound(MEASURED_PM) and worst["mean"] <= bound(MEASURED_MEAN)


def test_the_weights():
    for n in (2, 3, 4):
        g, wm0, wc0, wi = W(n)  # the defaults (1, 0, 1): lambda = 1
        assert (g, wm0, wc0, wi) == (np.sqrt(n + 1.0), 1.0 / (n + 1), 1.0 / (n + 1), 0.5 / (n + 1))
        assert UKF().weights(n) == (g, wm0, wc0, wi)
        g, wm0, wc0, wi = W(n, 0.1, 2.0, 0.0)
        lam = 0.01 * n - n
        assert np.isclose(g, np.sqrt(n + lam)) and np.isclose(wm0 + 2 * n * wi, 1.0) and np.isclose(wc0 - wm0, 1 - 0.01 + 2)
        assert UKF(alpha=0.1, beta=2.0, kappa=0.0).weights(n) == (g, wm0, wc0, wi)


# ----------------------------------------------------------------------------- exactness of the transform
@pytest.mark.parametrize("n", [2, 3, 4])
def test_unpropagated_sigma_points_return_the_mean_and_the_covariance(n):
    worst = dict(x=0.0, P=0.0, tx=0.0, tP=0.0)
    for seed in (0, 1, 2):
        p = em.seeded_problem(200 * n + seed, 33, n, 0)
        g, wm0, wc0, wi = W(n)
        s = um.sigma(p["xpred"], p["P"], g)
        m = um.moments(s["chi"], wm0, wc0, wi)
        xm_t, Pm_t = um.textbook_moments(s["chi"], wm0, wc0, wi)
        worst["x"] = max(worst["x"], float(np.abs(m["xm64"] - p["xpred"]).max()))
        worst["P"] = max(worst["P"], float(np.abs(m["Pm"] - p["P"]).max()))
        worst["tx"] = max(worst["tx"], float(np.abs(xm_t - p["xpred"]).max()))
        worst["tP"] = max(worst["tP"], float(np.abs(Pm_t - p["P"]).max()))
    print(f"\nn {n}: Y = chi gives back xhat to {worst['x']:.2e} (textbook {worst['tx']:.2e}), P to {worst['P']:.2e} "
          f"(textbook {worst['tP']:.2e})")
    assert worst["x"] <= MARGIN * MEASURED_BACK_X and worst["P"] <= MARGIN * MEASURED_BACK_P


@pytest.mark.parametrize("n", [2, 3, 4])
def test_the_mean_of_a_quadratic_map_is_the_second_order_value(n):
    """x -> x + c x^2 per component: the unscented mean is xhat + c (xhat^2 + P_ii), exact to second order; the
    linearised prediction f(xhat) = xhat + c xhat^2 misses c P_ii."""
    c = 0.7
    worst, worst_t, gap = 0.0, 0.0, np.inf
    for seed in (0, 1, 2):
        p = em.seeded_problem(300 * n + seed, 33, n, 0)
        g, wm0, wc0, wi = W(n)
        chi = um.sigma(p["xpred"], p["P"], g)["chi"].astype(np.float64)
        Y = (chi + c * chi * chi).astype(np.float32)
        x = p["xpred"].astype(np.float64)
        exact = x + c * (x * x + np.einsum("bii->bi", p["P"]))
        worst = max(worst, float(np.abs(um.moments(Y, wm0, wc0, wi)["xm64"] - exact).max()))
        worst_t = max(worst_t, float(np.abs(um.textbook_moments(Y, wm0, wc0, wi)[0] - exact).max()))
        gap = min(gap, float(np.abs((x + c * x * x) - exact).min()))
    print(f"\nn {n}: unscented mean of x + c x^2 off the analytic value by {worst:.2e} (textbook {worst_t:.2e}); f(xhat) by >= {gap:.2e}")
    assert worst <= MARGIN * MEASURED_QUAD
    assert gap > 1000 * MARGIN * MEASURED_QUAD, "the linearised prediction is not the second-order mean"


# ----------------------------------------------------------------------------- the Kalman filter on linear systems
# 16 x what this model measures over the twelve runs (printed below): 2.1e-7 of the largest |xhat|, 7.7e-7 of the largest
# |P|, the z scores of the two filters equal to the printed digits with |z| <= 1.44; never above 2e-5 (wrong weights
# give >= 1e-2)
KF_X, KF_P, KF_CEILING = 2.1e-7, 7.7e-7, 2e-5


def _linear_run(seed, n, mask, w=None):
    s = em.consistency_system(seed, n, mask)
    nb, T = s["xhat0"].shape[0], s["ys"].shape[0]
    w = W(n) if w is None else w
    F32 = np.broadcast_to(s["F"].astype(np.float32), (nb, n, n))
    xu, Pu = s["xhat0"].copy(), np.broadcast_to(s["P0"], (nb, n, n)).copy()
    xk, Pk = xu.copy(), Pu.copy()
    dev_x = dev_P = big_x = big_P = 0.0
    nis_u = nis_k = 0.0
    fails = 0
    for t in range(T):
        r = um.step(xu, Pu, lambda chi: (chi.astype(np.float64) @ s["F"].T).astype(np.float32), s["ys"][t], mask, s["Qn"], s["Rn"], w)
        k = em.update((xk.astype(np.float64) @ s["F"].T).astype(np.float32), F32, Pk, s["ys"][t], mask, s["Qn"], s["Rn"])
        fails += int((r["status"] != 0).sum()) + int((k["status"] != 0).sum()) + int(np.isnan(r["chi"]).any(axis=(1, 2)).sum())
        xu, Pu, xk, Pk = r["xhat"], r["P"], k["xhat"], k["P"]
        dev_x, big_x = max(dev_x, float(np.abs(xu.astype(np.float64) - xk).max())), max(big_x, float(np.abs(xk).max()))
        dev_P, big_P = max(dev_P, float(np.abs(Pu - Pk).max())), max(big_P, float(np.abs(Pk).max()))
        nis_u += float(r["nis"].sum())
        nis_k += float(k["nis"].sum())
    p = len(s["idx"])
    return dict(fails=fails, x=dev_x / big_x, P=dev_P / big_P, z_ukf=em.consistency_z(nis_u, nb * T, p),
                z_kf=em.consistency_z(nis_k, nb * T, p))


@pytest.mark.parametrize("n,mask", [(2, 0b1), (3, 0b101), (4, 0b0011), (4, 0b1111)])
@pytest.mark.parametrize("seed", [0, 2, 4])
def test_on_a_linear_system_the_filter_is_the_kalman_filter(seed, n, mask):
    r = _linear_run(seed, n, mask)
    print(f"\nseed {seed} n {n} mask {mask:04b}: failures {r['fails']}, xhat {r['x']:.2e}, P {r['P']:.2e} of the largest entry; "
          f"z ukf {r['z_ukf']:+.3f}, kf {r['z_kf']:+.3f}")
    assert r["fails"] == 0
    assert r["x"] <= min(16 * KF_X, KF_CEILING) and r["P"] <= min(16 * KF_P, KF_CEILING)
    assert abs(r["z_ukf"]) <= 3.0 and abs(r["z_kf"]) <= 3.0


def test_wrong_weights_are_seen_by_the_linear_bound():
    g, wm0, wc0, wi = W(4)
    r = _linear_run(0, 4, 0b0011, (g, wm0, wc0, 1.1 * wi))
    assert r["P"] >= 1e-2


# ----------------------------------------------------------------------------- failures and isolation
def _one_step(p, n, mask):
    w = W(n)
    A = p["A"].astype(np.float64)
    return um.step(p["xpred"], p["P"], lambda chi: np.einsum("bij,bj->bi", np.repeat(A, 2 * n + 1, axis=0), chi.astype(np.float64)).astype(np.float32),
                   p["y"], mask, p["Qn"], p["Rn"], w)


@pytest.mark.parametrize("n,name", [(2, "all"), (3, "pair02"), (4, "pair02"), (4, "empty")])
def test_failures_and_dropouts_are_per_problem(n, name):
    mask = em.MASKS[n][name]
    p = em.seeded_problem(20 + n, 17, n, mask)
    clean = _one_step({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}, n, mask)
    assert not clean["status"].any()
    p["P"][2] = np.diag(np.full(n, -50.0))  # indefinite
    p["P"][5][n - 1, 0] = np.inf  # an infinite entry in the lower triangle
    p["xpred"][7, n - 1] = np.nan
    p["P"][9][:] = 0.0  # exactly singular: a failure, not a special case
    p["P"][12][0, n - 1] = np.nan  # the upper triangle is not read
    failed = [2, 5, 7, 9]
    if mask:
        p["y"][11, em.measured_of(mask, n)[-1]] = np.inf  # a dropped measurement
    r = _one_step(p, n, mask)
    for b in failed:
        assert np.isnan(r["chi"][b]).all() and r["status"][b] == 2
        assert np.isnan(r["xhat"][b]).all() and np.isnan(r["P"][b]).all() and np.isnan(r["nis"][b])
    if mask:
        assert r["status"][11] == 1 and np.array_equal(r["xhat"][11], r["xm"][11]) and np.isnan(r["nis"][11])
        pred = 0.5 * ((r["Pm"][11] + p["Qn"]) + (r["Pm"][11] + p["Qn"]).T)
        assert np.abs(r["P"][11] - pred).max() <= 1e-15, "a dropped measurement leaves the prediction"
    else:  # nothing measured: the prediction, status 0
        assert not r["status"][[b for b in range(17) if b not in failed]].any() and np.isnan(r["nis"]).all()
        assert np.array_equal(r["xhat"][0], r["xm"][0])
    rest = [b for b in range(17) if b not in failed + [11]]
    for k in ("chi", "xm", "Pm", "xhat", "P", "nis", "status"):
        assert em.same_floats(r[k][rest], clean[k][rest]), f"{k}: the neighbours keep their bits"


@pytest.mark.parametrize("n,name", [(2, "single"), (3, "pair02"), (4, "all")])
def test_covariance_stays_symmetric_bit_for_bit_over_50_steps(n, name):
    mask = em.MASKS[n][name]
    p = em.seeded_problem(11, 5, n, mask)
    rng = np.random.default_rng(12)
    x, P = p["xpred"], p["P"]
    for _ in range(50):
        q = em.seeded_problem(int(rng.integers(1 << 30)), 5, n, mask)
        r = _one_step(dict(q, xpred=x, P=P, Qn=p["Qn"], Rn=p["Rn"]), n, mask)
        x, P = r["xhat"], r["P"]
        assert not r["status"].any() and np.array_equal(P, np.swapaxes(P, 1, 2)) and np.array_equal(r["Pm"], np.swapaxes(r["Pm"], 1, 2))
    assert np.all(np.linalg.eigvalsh(P) > 0)


# ----------------------------------------------------------------------------- UKF on the CPU stand-in
X0 = np.array([[0.3, 0.1, 0.2, -0.1], [-0.5, 0.05, -0.3, 0.2], [0.1, -0.15, 0.4, 0.3], [0.8, 0.19, -0.2, -0.4]])
KW = dict(measured=(0, 1), Qn=[1e-6, 1e-6, 1e-4, 1e-4], Rn=[1e-4, 2.5e-5], P0=0.01)


def _model(cls=um.UkfOracleEngine):
    w = ol.load_weights("phnn_cartpole")
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    eng = cls(w)
    return m.set_engine(eng), eng


def _inputs():
    u = torch.tensor([[3.0], [-25.0], [0.5], [40.0]])  # two of them outside the bounds
    y = torch.tensor((X0 + 0.01).astype(np.float32))
    y[:, 2:] = float("nan")  # velocities are not measured: never read
    return u, y, _capi.make_cost(4, 1, [10.0, 100.0, 1.0, 10.0], 0.01, None, -10.0, 10.0)


def test_ukf_step_on_the_oracle_engine_with_the_golden_cartpole_phnn():
    _, eng = _model()
    ukf = UKF(**KW)
    u, y, cost = _inputs()
    xh0, P0 = ukf.initial(X0)
    xhat, P = torch.tensor(xh0), torch.tensor(P0)
    r = ukf.step(eng, xhat, P, u, y, cost, "euler", 0.02)
    assert eng.calls == ["ukf_sigma", "ukf_moments", "ekf_update"]
    assert torch.equal(xhat, torch.tensor(xh0)) and torch.equal(P, torch.tensor(P0)), "the inputs keep their values"
    # the same by hand: the stated sigma points, K1 with the clamped control on each, the stated moments and update
    o = ukf.options(4)
    w = (o.gamma, o.wm0, o.wc0, o.wi)
    assert w == um.weights(4)
    sg = um.sigma(xh0, P0, w[0], u.numpy())
    assert np.array_equal(sg["ctrl"][:, :, 0, 0], np.repeat(u.numpy(), 9, axis=1)), "the control rows are unclamped copies"
    uc = torch.from_numpy(sg["ctrl"]).clamp(-10.0, 10.0).reshape(36, 1, 1)
    _, traj = eng.rollout_cost(torch.from_numpy(sg["chi"]).reshape(36, 4), uc, _capi.Cost(), "euler", 0.02, want_traj=True)
    mo = um.moments(traj[:, 1].numpy().reshape(4, 9, 4), *w[1:])
    ref = em.update(mo["xm"], mo["eye"], mo["Pm"], y.numpy(), 0b0011, np.array(o.Qn[:16]).reshape(4, 4), np.array(o.Rn[:4]))
    for k in ("xhat", "P", "nis", "innov", "status"):
        assert em.same_floats(r[k].numpy(), ref[k]), k
    assert not ref["status"].any() and np.all(ref["nis"] > 0)
    # sigma point 0 is the EKF's prediction; the estimate moves from the mean towards the measurement
    _, t0 = eng.rollout_cost(xhat, u.clamp(-10.0, 10.0).reshape(4, 1, 1), _capi.Cost(), "euler", 0.02, want_traj=True)
    assert torch.equal(traj.reshape(4, 9, 2, 4)[:, 0, 1], t0[:, 1])
    pred, est, meas = mo["xm"][:, :2], r["xhat"][:, :2].numpy(), y[:, :2].numpy()
    assert np.all(np.abs(est - meas) < np.abs(pred - meas))
    # close to the EKF where the model is smooth and P small, and not the same numbers
    e = EKF(**KW).step(eng, xhat, P, u, y, cost, "euler", 0.02)
    assert np.abs(r["xhat"].numpy() - e["xhat"].numpy()).max() < 1e-3 and not torch.equal(r["P"], e["P"])


def _controller(model, **kw):
    return MPCController(phnn_model=model, horizon=5, dt=0.02, Q=[10.0, 100.0, 1.0, 10.0], R=0.01, u_min=-10.0, u_max=10.0,
                         optimizer_type="Adam", lr=0.1, max_iterations=3, **kw)


def test_run_mpc_batch_with_a_ukf_on_the_oracle_engine():
    model, eng = _model()
    ctl = _controller(model)
    steps, B = 3, X0.shape[0]
    sc = PlantScenario(meas_sigma=[0.01, 0.005, 0.05, 0.05], seed=77)
    ukf = UKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4)
    out = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, steps, scenario=sc, estimator=ukf)
    assert out["estimates"].shape == (steps + 1, B, 4) and out["estimates"].dtype == np.float32
    assert out["nis"].shape == (steps, B) and np.all(out["nis"] > 0) and not out["ekf_status"].any()
    assert set(out) == {"states", "controls", "done_step", "estimates", "nis", "ekf_status"}
    assert eng.calls.count("ukf_sigma") == eng.calls.count("ukf_moments") == eng.calls.count("ekf_update") == steps
    assert "rollout_linearize" not in eng.calls, "no Jacobian anywhere"
    for s in range(steps):  # every control is the controller's answer to the estimate
        assert np.array_equal(out["controls"][s], ctl.compute_control_batch(out["estimates"][s]).astype(np.float64))
    assert np.abs(out["estimates"] - out["states"]).max() < 0.2
    blind = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, estimator=UKF(measured=(), Qn=1e-6, P0=1e-4))
    assert np.isnan(blind["nis"]).all() and not blind["ekf_status"].any() and np.isfinite(blind["estimates"]).all()


def test_the_other_estimators_are_what_they_were():
    class Both(um.UkfOracleEngine, dm.DekfOracleEngine):
        pass

    u, y, cost = _inputs()
    _, old = _model(em.EkfOracleEngine)
    _, new = _model(Both)
    ekf = EKF(**KW)
    xh0, P0 = ekf.initial(X0)
    a = ekf.step(old, torch.tensor(xh0), torch.tensor(P0), u, y, cost, "euler", 0.02)
    b = ekf.step(new, torch.tensor(xh0), torch.tensor(P0), u, y, cost, "euler", 0.02)
    assert old.calls == new.calls == ["rollout_linearize", "ekf_update"]
    _, oldd = _model(dm.DekfOracleEngine)
    _, newd = _model(Both)
    dk = DisturbanceEKF(Qd=1e-6, Pd0=1.0, **KW)
    xh0, dh0, Pz0 = dk.initial(X0, 1)
    c = dk.step(oldd, torch.tensor(xh0), torch.tensor(dh0), torch.tensor(Pz0), u, y, cost, "euler", 0.02)
    d = dk.step(newd, torch.tensor(xh0), torch.tensor(dh0), torch.tensor(Pz0), u, y, cost, "euler", 0.02)
    assert oldd.calls == newd.calls and "ukf_sigma" not in newd.calls
    for p, q in ((a, b), (c, d)):
        for k in p:
            assert em.same_floats(p[k].numpy(), q[k].numpy()), k
    model, eng = _model()
    ctl = _controller(model)
    sc = PlantScenario(meas_sigma=0.01, seed=5)
    p = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, scenario=sc)
    q = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, scenario=sc, estimator=None)
    assert set(p) == set(q) == {"states", "controls", "done_step"} and all(np.array_equal(p[k], q[k]) for k in p)
    assert not any(c.startswith(("ukf", "ekf")) for c in eng.calls)
    e = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, scenario=sc, estimator=EKF(measured=(0, 1), Qn=1e-6, Rn=1e-4, P0=1e-4))
    assert eng.calls.count("ekf_update") == 2 and "ukf_sigma" not in eng.calls and not e["ekf_status"].any()


# ----------------------------------------------------------------------------- options and configuration
def test_option_and_initial_refusals():
    o = UKF(measured=(0, 2), Rn=[1e-4, 4e-4], Qn=np.arange(16.0).reshape(4, 4)).options(4)
    assert o.meas_mask == 0b0101 and list(o.Rn) == [1e-4, 0.0, 4e-4, 0.0] and list(o.Qn) == list(np.arange(16.0))
    assert list(o.reserved) == [0, 0, 0, 0] and (o.gamma, o.wm0, o.wc0, o.wi) == um.weights(4)
    o3 = UKF(measured=(1,), Qn=np.arange(9.0).reshape(3, 3)).options(3)
    assert list(o3.Qn[:9]) == list(np.arange(9.0)) and o3.gamma == 2.0
    with pytest.raises(ValueError, match="state components"):
        UKF(measured=(0, 2)).options(2)
    with pytest.raises(ValueError, match="at most 4"):
        UKF().options(5)
    with pytest.raises(ValueError, match="n \\+ lambda"):
        UKF(alpha=1.0, kappa=-4.0).options(4)
    for p0 in (0.0, -1.0, np.diag([1.0, 1.0, 1.0, -1e-3]), np.ones((4, 4))):
        with pytest.raises(ValueError, match="positive definite"):
            UKF(P0=p0).initial(X0)
    xh, P = UKF(P0=[1.0, 2.0, 3.0, 4.0]).initial(X0)
    assert np.array_equal(P[3], np.diag([1.0, 2.0, 3.0, 4.0])) and np.array_equal(xh, X0.astype(np.float32))


def test_from_config_builds_a_ukf_and_delegates_the_rest():
    assert estimation.from_config({"mpc": {}}) is None
    u = estimation.from_config({"estimator": {"type": "ukf", "measured": [0, 1], "Qn": [1e-8, 1e-8, 1e-5, 1e-5], "Rn": 1e-4,
                                              "P0": 1e-3, "log": False, "alpha": 0.5, "beta": 2.0, "kappa": 0.0}})
    assert type(u) is UKF and u.measured == (0, 1) and u.log is False and (u.alpha, u.beta, u.kappa) == (0.5, 2.0, 0.0)
    assert u.options(4).Qn[15] == 1e-5 and u.weights(4) == um.weights(4, 0.5, 2.0, 0.0)
    d = estimation.from_config({"estimator": {"type": "UKF"}})
    assert type(d) is UKF and (d.alpha, d.beta, d.kappa) == (1.0, 0.0, 1.0)
    with pytest.raises(ValueError, match="unknown key"):
        estimation.from_config({"estimator": {"type": "ukf", "Qd": 1.0}})
    e = estimation.from_config({"estimator": {"measured": [0], "Rn": 1e-3}})
    assert type(e) is EKF and e.measured == (0,)
    k = estimation.from_config({"estimator": {"type": "ekf_disturbance", "Qd": 1e-6}})
    assert type(k) is DisturbanceEKF
    with pytest.raises(ValueError, match="unknown key"):
        estimation.from_config({"estimator": {"type": "ekf", "alpha": 1.0}})
    with pytest.raises(ValueError, match="Unknown estimator type"):
        estimation.from_config({"estimator": {"type": "mhe"}})
    with pytest.raises(ValueError, match="Unknown estimator type"):
        EKF.from_config({"estimator": {"type": "ukf"}})
    import yaml
    for name in os.listdir(os.path.join(ROOT, "configs")):
        if name.endswith((".yaml", ".yml")):  # no shipped configuration has the section
            assert estimation.from_config(yaml.safe_load(open(os.path.join(ROOT, "configs", name))) or {}) is None


def _fields(header, struct):
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} %s;" % struct, header, re.S).group(1)
    return re.findall(r"\b(\w+)(?:\[[\w *]+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_structs_match_the_header_and_the_symbols_are_exported():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    assert _fields(header, "phnn_ukf_options") == [f for f, _ in _capi.UkfOptions._fields_]
    assert _fields(header, "phnn_ekf_log") == [f for f, _ in _capi.EkfLog._fields_]  # the step's log is the EKF's
    assert re.search(r"#define PHNN_UKF_MAX_N %d\b" % _capi.PHNN_UKF_MAX_N, header)
    # uint32 + pad, 16 + 4 doubles, four doubles, int32[4];  two pointers, a pointer, int32 + pad
    o, lg = _capi.UkfOptions, _capi.EkfLog
    assert C.sizeof(o) == 8 + 8 * 20 + 8 * 4 + 16
    assert (o.meas_mask.offset, o.Qn.offset, o.Rn.offset, o.gamma.offset, o.wm0.offset, o.wc0.offset, o.wi.offset,
            o.reserved.offset) == (0, 8, 136, 168, 176, 184, 192, 200)
    assert C.sizeof(lg) == 32 and (lg.log_xhat_dev.offset, lg.log_nis_dev.offset, lg.step_dev.offset, lg.step_host.offset) == (0, 8, 16, 24)
    lib = _capi.load_library()
    for name in ("phnn_ukf_workspace_bytes", "phnn_ukf_sigma", "phnn_ukf_moments", "phnn_ukf_step"):
        assert name in _capi.EXPORTED and re.search(r"\b%s\(" % name, header) and hasattr(lib, name)
    assert lib.phnn_version() == 290
