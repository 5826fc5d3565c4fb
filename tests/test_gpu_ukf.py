"""The batched unscented Kalman filter on the device.

  1 k_ukf_sigma        bits == ukf_model.sigma in chi and in the control rows for n in {2, 3, 4}, m in {1, 2}, B in
                       {1, 17, 65}, u strides m and H m, failures mixed into the batch
  2 k_ukf_moments      bits == ukf_model.moments in xm, Pm and the identity, Y dense and read in place from row 1 of a
                       (B S, 2, n) trajectory
  3 phnn_ukf_step      bits == the four calls made by hand (estimation.UKF.step): three models, Euler and RK4, controls
                       outside the bounds, cost given and NULL; one ReLU model
  4 sigma point 0      its image == the prediction phnn_ekf_step forms from the same xhat and u: a rollout does not see
                       its batch-mates
  5 footprint          the three entry points in guarded buffers (tests/footprint.py)
  6 refusals           PHNN_ERR_INVALID_ARG / PHNN_ERR_UNSUPPORTED with no output touched
  7 closed loop        DeviceClosedLoop(estimator=UKF): graphed == eager == run_mpc_batch on the same engine, Adam and
                       Gauss-Newton, and once with track=
"""
import ctypes as C

import numpy as np
import pytest

import ekf_model as em
import footprint as fp
import ukf_model as um
import variant_census as vc
from test_gpu_ekf import DevicePlant, _controller, dev, npy
from test_gpu_footprint import engine as census_engine
from test_gpu_mppi import engine

pytestmark = pytest.mark.gpu
RELU_SPEC = "phnn<n=4,hid=128,fixedG,relu>"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def engine_nm(n, m):
    """A handle with n state and m input components: the two kernels read none of its weights."""
    eng = census_engine(vc.NM_SPEC[(n, m)])
    assert (eng.n, eng.m) == (n, m)
    return eng


def ukf_options(n, mask=0, Qn=None, Rn=None, w=None):
    from phnn_mpc_amd import _capi
    o = _capi.UkfOptions()
    o.meas_mask = mask
    for i in range(n * n):
        o.Qn[i] = 0.0 if Qn is None else float(np.asarray(Qn).reshape(-1)[i])
    for i in range(n):
        o.Rn[i] = 1.0 if Rn is None else float(Rn[i])
    o.gamma, o.wm0, o.wc0, o.wi = um.weights(n) if w is None else w
    return o


def plant_failures(p, B, n):
    """Mixes failures into a seeded problem IN PLACE where the batch is large enough -> their indices."""
    if B < 17:
        return []
    p["P"][2] = np.diag(np.full(n, -50.0))  # indefinite
    p["P"][5][n - 1, 0] = np.inf  # an infinite entry of the lower triangle
    p["xpred"][7, n - 1] = np.nan
    p["P"][9][:] = 0.0  # exactly singular
    p["P"][12][0, n - 1] = np.nan  # the upper triangle is not read: no failure
    return [2, 5, 7, 9]


# ----------------------------------------------------------------------------- 1. the sigma points against the model
@pytest.mark.parametrize("n,m", [(2, 1), (3, 1), (4, 1), (4, 2)])
def test_sigma_equals_the_model_bit_for_bit(torch, n, m):
    eng, S, H = engine_nm(n, m), 2 * n + 1, 3
    for B in (1, 17, 65):
        for w in (um.weights(n), um.weights(n, 0.5, 2.0, 0.0)):
            p = em.seeded_problem(2000 * n + B, B, n, 0)
            failed = plant_failures(p, B, n)
            rng = np.random.default_rng(B)
            u = rng.uniform(-4, 4, size=(B, H, m)).astype(np.float32)
            o = ukf_options(n, w=w)
            for stride, uu in ((H * m, u), (m, u[:, 0])):
                ref = um.sigma(p["xpred"], p["P"], w[0], u[:, 0])
                assert list(np.flatnonzero(ref["fail"])) == failed
                chi, ctrl = eng.ukf_sigma(dev(torch, p["xpred"]), dev(torch, p["P"]), o, u=dev(torch, uu), u_stride=stride)
                assert chi.shape == (B, S, n) and ctrl.shape == (B, S, 1, m)
                assert em.same_floats(npy(chi), ref["chi"]), (B, stride)
                assert np.array_equal(npy(ctrl), ref["ctrl"]), (B, stride)
                assert np.isnan(npy(chi)[failed]).all() and np.isfinite(np.delete(npy(chi), failed, axis=0)).all()
            chi2, none = eng.ukf_sigma(dev(torch, p["xpred"]), dev(torch, p["P"]), o)  # without control rows
            assert none is None and em.same_floats(npy(chi2), ref["chi"])


# ----------------------------------------------------------------------------- 2. the moments against the model
@pytest.mark.parametrize("n", [2, 3, 4])
def test_moments_equal_the_model_bit_for_bit(torch, n):
    eng, S = engine_nm(n, 1), 2 * n + 1
    for B in (1, 17, 65):
        for w in (um.weights(n), um.weights(n, 0.5, 2.0, 0.0)):
            p = em.seeded_problem(3000 * n + B, B, n, 0)
            chi = um.sigma(p["xpred"], p["P"], w[0])["chi"]
            Y = np.einsum("bij,bkj->bki", p["A"].astype(np.float64), chi.astype(np.float64)).astype(np.float32)
            if B >= 17:
                Y[3, 2, 0] = np.nan  # a NaN image: that problem's moments are NaN, its neighbours keep their bits
                Y[8, 0, n - 1] = np.inf
            ref = um.moments(Y, *w[1:])
            o = ukf_options(n, w=w)
            r = eng.ukf_moments(dev(torch, Y), B, o)
            for k in ("xm", "Pm", "eye"):
                assert em.same_floats(npy(r[k]), ref[k]), (B, k)
            assert np.array_equal(npy(r["eye"]), np.broadcast_to(np.eye(n, dtype=np.float32), (B, n, n)))
            if B >= 17:
                assert (~np.isfinite(npy(r["xm"])[[3, 8]])).any(axis=1).all() and np.isfinite(np.delete(npy(r["Pm"]), [3, 8], axis=0)).all()
            # in place from row 1 of a (B S, 2, n) trajectory whose row 0 holds something else; no identity asked for
            traj = np.full((B * S, 2, n), 123.0, np.float32)
            traj[:, 1] = Y.reshape(B * S, n)
            r2 = eng.ukf_moments(dev(torch, traj).reshape(-1)[n:], B, o, Y_stride=2 * n, eye=False)
            assert r2["eye"] is None
            for k in ("xm", "Pm"):
                assert em.same_floats(npy(r2[k]), ref[k]), (B, k, "strided")


# ----------------------------------------------------------------------------- 3. the step against the four calls by hand
STEP_MODELS = {"phnn_cartpole": (0, 1), "canonical_cartpole": (0, 2), "odefunc_pendulum": (0,)}


def _step_by_hand(torch, eng, integ, measured, Bs=(1, 17, 65)):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.estimation import UKF
    n, m, H = eng.n, eng.m, 3
    ukf = UKF(measured=measured, Qn=np.linspace(1e-6, 1e-4, n), Rn=1e-3, P0=0.02)
    o = ukf.options(n)
    cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0)
    for B in Bs:
        rng = np.random.default_rng(50 + B)
        x0 = (0.3 * rng.normal(size=(B, n))).astype(np.float32)
        F = 0.1 * rng.normal(size=(B, n, n))
        P0 = F @ np.swapaxes(F, 1, 2) + 0.02 * np.eye(n)  # a full covariance, another one per problem
        P0 = 0.5 * (P0 + np.swapaxes(P0, 1, 2))
        u = rng.uniform(-4.0, 4.0, size=(B, H, m)).astype(np.float32)  # some of them outside the bounds
        assert B == 1 or ((u[:, 0] < -1.5).any() and (u[:, 0] > 2.0).any())
        y = (x0 + 0.05 * rng.normal(size=(B, n))).astype(np.float32)
        y[:, [i for i in range(n) if i not in ukf.measured]] = np.nan
        if B >= 17:
            P0[4] = -P0[4]  # no Cholesky factor: status 2, NaN, and the neighbours do not see it
        for c in (cost, None):
            xhat, P = dev(torch, x0), dev(torch, P0)
            hand = ukf.step(eng, xhat, P, dev(torch, u[:, 0]), dev(torch, y), c, integ, 0.02, opt=o)
            got = eng.ukf_step(xhat, P, dev(torch, u), H * m, dev(torch, y), c, integ, 0.02, o, nis=True, innov=True)
            assert got["xhat"] is xhat and got["P"] is P
            for k in ("xhat", "P", "nis", "innov", "status"):
                assert em.same_floats(npy(got[k]), npy(hand[k])), (B, k, c is None)
            st = npy(got["status"])
            if B >= 17:
                assert st[4] == 2 and np.isnan(npy(xhat)[4]).all() and np.isnan(npy(P)[4]).all()
                st = np.delete(st, 4)
            assert not st.any() and np.all(np.delete(npy(got["nis"]), 4 if B >= 17 else [], axis=0) > 0)
            assert np.isfinite(np.delete(npy(xhat), 4 if B >= 17 else [], axis=0)).all() and not np.array_equal(npy(xhat), x0)


@pytest.mark.parametrize("model", list(STEP_MODELS))
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_step_equals_the_four_calls_by_hand(torch, model, integ):
    _step_by_hand(torch, engine(model), integ, STEP_MODELS[model])


def test_step_on_a_relu_model_equals_the_calls_by_hand(torch):
    _step_by_hand(torch, census_engine(RELU_SPEC), "euler", (0, 1), Bs=(17,))


# ----------------------------------------------------------------------------- 4. sigma point 0 is the EKF's prediction
@pytest.mark.parametrize("model,integ", [("phnn_cartpole", "euler"), ("phnn_cartpole", "rk4"), ("odefunc_pendulum", "euler")])
def test_sigma_point_0_is_the_prediction_of_the_ekf_step(torch, model, integ):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.estimation import EKF, UKF
    eng = engine(model)
    n, m, B = eng.n, eng.m, 17
    S = 2 * n + 1
    rng = np.random.default_rng(9)
    x0 = (0.3 * rng.normal(size=(B, n))).astype(np.float32)
    u = rng.uniform(-4.0, 4.0, size=(B, m)).astype(np.float32)
    cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0)
    y = dev(torch, np.full((B, n), np.nan, np.float32))
    # nothing measured: the EKF's estimate is its prediction, bit for bit
    blind = EKF(measured=(), Qn=1e-6, P0=0.02)
    xe, Pe = dev(torch, x0), dev(torch, blind.initial(x0)[1])
    eng.ekf_step(xe, Pe, dev(torch, u), m, y, cost, integ, 0.02, blind.options(n))
    ukf = UKF(measured=(), Qn=1e-6, P0=0.02)
    chi, ctrl = eng.ukf_sigma(dev(torch, x0), dev(torch, ukf.initial(x0)[1]), ukf.options(n), u=dev(torch, u))
    bounds = _capi.Cost()
    bounds.has_u_bounds, bounds.u_min, bounds.u_max = cost.has_u_bounds, cost.u_min, cost.u_max
    _, traj = eng.rollout_cost(chi.reshape(B * S, n), ctrl.reshape(B * S, 1, m), bounds, integ, 0.02, want_traj=True)
    img = npy(traj).reshape(B, S, 2, n)
    assert np.array_equal(img[:, 0, 1], npy(xe)), "among 2 n other rollouts of its problem, sigma point 0 lands where the EKF predicts"
    assert not np.array_equal(img[:, 1, 1], img[:, 0, 1])


# ----------------------------------------------------------------------------- 5. footprint
class UkfSigmaOp(fp.Op):
    """phnn_ukf_sigma with the first control of a (B,H,m) sequence."""
    H = 3

    def __init__(self, n, m, B, rng, ctrl=True):
        super().__init__()
        self.name, self.n, self.m, self.B, self.ctrl = f"ukf_sigma n{n} m{m} B{B} ctrl={ctrl}", n, m, B, ctrl
        p = em.seeded_problem(int(rng.integers(1 << 30)), B, n, 0)
        plant_failures(p, B, n)
        f32, S = np.float32, 2 * n + 1
        self.add("xhat", f32, (B, n), fp.IN, p["xpred"])
        self.add("P", np.float64, (B, n, n), fp.IN, p["P"])
        self.add("chi", f32, (B, S, n), fp.OUT)
        if ctrl:
            self.add("u", f32, (B, self.H, m), fp.IN, rng.uniform(-4, 4, size=(B, self.H, m)).astype(f32))
            self.add("ctrl", f32, (B, S, 1, m), fp.OUT)

    def call(self, eng, p):
        o = ukf_options(self.n)
        fp.check_rc(eng, eng.lib.phnn_ukf_sigma(eng.h, p["xhat"], p["P"], p.get("u"), self.H * self.m, self.B, C.byref(o), p["chi"],
                                                p.get("ctrl"), eng._stream()))

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        chi, ctrl = eng.ukf_sigma(t["xhat"], t["P"], ukf_options(self.n), u=t.get("u"), u_stride=self.H * self.m)
        return dict(chi=chi, ctrl=ctrl) if self.ctrl else dict(chi=chi)


class UkfMomentsOp(fp.Op):
    """phnn_ukf_moments on row 1 of a (B S, 2, n) trajectory."""

    def __init__(self, n, B, rng, eye=True):
        super().__init__()
        self.name, self.n, self.B, self.eye = f"ukf_moments n{n} B{B} eye={eye}", n, B, eye
        f32, S = np.float32, 2 * n + 1
        self.add("traj", f32, (B * S, 2, n), fp.IN, rng.normal(size=(B * S, 2, n)).astype(f32))
        self.add("xm", f32, (B, n), fp.OUT)
        self.add("Pm", np.float64, (B, n, n), fp.OUT)
        if eye:
            self.add("eye", f32, (B, n, n), fp.OUT)

    def call(self, eng, p):
        o = ukf_options(self.n)
        Y = C.c_void_p(p["traj"].value + 4 * self.n)
        fp.check_rc(eng, eng.lib.phnn_ukf_moments(eng.h, Y, 2 * self.n, self.B, C.byref(o), p["xm"], p["Pm"], p.get("eye"), eng._stream()))

    def engine(self, eng):
        import torch
        traj = torch.tensor(self.bufs[0].init, device=eng.device)
        r = eng.ukf_moments(traj.reshape(-1)[self.n:], self.B, ukf_options(self.n), Y_stride=2 * self.n, eye=self.eye)
        return {k: v for k, v in r.items() if v is not None}


class UkfStepOp(fp.Op):
    """phnn_ukf_step with the first control of a (B,H,m) sequence, at step 1 of 3."""
    H = 3

    def __init__(self, eng, B, measured, integ, rng, bounded=True, drop=()):
        from phnn_mpc_amd import _capi
        from phnn_mpc_amd.estimation import UKF
        super().__init__()
        n, m = eng.n, eng.m
        self.name, self.n, self.m, self.B, self.integ, self.drop = f"ukf_step B{B} {integ} drop={','.join(drop) or '-'}", n, m, B, integ, set(drop)
        self.ukf = UKF(measured=measured, Qn=1e-5, Rn=1e-3, P0=0.02)
        self.cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0) if bounded else None
        f32, f64 = np.float32, np.float64
        x0 = (0.3 * rng.normal(size=(B, n))).astype(f32)
        y = (x0 + 0.05 * rng.normal(size=(B, n))).astype(f32)
        y[:, [i for i in range(n) if i not in measured]] = np.nan
        nbytes = eng.ukf_workspace_bytes(B)
        assert nbytes > 0
        self.add("xhat", f32, (B, n), fp.INOUT, x0)
        self.add("P", f64, (B, n, n), fp.INOUT, self.ukf.initial(x0)[1])
        self.add("u", f32, (B, self.H, m), fp.IN, rng.uniform(-4, 4, size=(B, self.H, m)).astype(f32))
        self.add("y", f32, (B, n), fp.IN, y)
        self.add("status", np.int32, (B,), fp.OUT)
        self.add("ws", np.uint8, (nbytes,), fp.WS)
        if "nis" not in self.drop:
            self.add("nis", f64, (B,), fp.OUT)
        if "innov" not in self.drop:
            self.add("innov", f64, (B, n), fp.OUT)
        if "log" not in self.drop:
            self.add("log_xhat", f32, (4, B, n), fp.INOUT, np.zeros((4, B, n), f32))
            self.add("log_nis", f64, (3, B), fp.INOUT, np.zeros((3, B)))

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        lg = None
        if "log" not in self.drop:
            lg = _capi.EkfLog()
            lg.log_xhat_dev, lg.log_nis_dev, lg.step_host = p["log_xhat"].value, p["log_nis"].value, 1
        o = self.ukf.options(self.n)
        rc = eng.lib.phnn_ukf_step(eng.h, p["xhat"], p["P"], p["u"], self.H * self.m, p["y"], self.n, self.B,
                                   C.byref(self.cost) if self.cost is not None else None, eng._integ(self.integ), 0.02, C.byref(o),
                                   p.get("nis"), p.get("innov"), p["status"], C.byref(lg) if lg else None, p["ws"], eng._stream())
        fp.check_rc(eng, rc)

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        log = None if "log" in self.drop else dict(log_xhat=t["log_xhat"], log_nis=t["log_nis"], step=1)
        r = eng.ukf_step(t["xhat"], t["P"], t["u"], self.H * self.m, t["y"], self.cost, self.integ, 0.02, self.ukf.options(self.n),
                         nis="nis" not in self.drop, innov="innov" not in self.drop, log=log)
        t.update({k: v for k, v in r.items() if v is not None})
        return {b.name: t[b.name] for b in self.outputs() if b.role != fp.WS}


@pytest.mark.parametrize("n,m", [(2, 1), (3, 1), (4, 2)])
def test_footprint_of_the_two_kernels(torch, n, m):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = engine_nm(n, m)
    rep = Report(f"phnn_ukf_sigma / phnn_ukf_moments n{n} m{m}")
    for B in (17, 65):
        for full in (True, False):
            footprint(rep, torch, eng, UkfSigmaOp(n, m, B, rng_of("ukf_sigma", n, m, B, full), ctrl=full))
            footprint(rep, torch, eng, UkfMomentsOp(n, B, rng_of("ukf_moments", n, B, full), eye=full))
    rep.finish()


@pytest.mark.parametrize("model,integ", [("phnn_cartpole", "euler"), ("canonical_cartpole", "rk4"), ("odefunc_pendulum", "rk4")])
def test_footprint_of_the_step(torch, model, integ):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = engine(model)
    rep = Report(f"phnn_ukf_step {model} {integ}")
    measured = (0,) if eng.n == 2 else (0, 1)
    for B in (17, 65):
        for bounded, drop in ((True, ()), (False, ("nis", "innov", "log"))):
            footprint(rep, torch, eng, UkfStepOp(eng, B, measured, integ, rng_of("ukf_step", model, B, bounded), bounded, drop))
    rep.finish()


# ----------------------------------------------------------------------------- 6. refusals
def test_bad_arguments_are_refused_and_nothing_is_written(torch):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    eng = engine("phnn_cartpole")
    n, B, S = 4, 5, 9
    p = em.seeded_problem(3, B, n, 0b0011)
    x, y, u = dev(torch, p["xpred"]), dev(torch, p["y"]), dev(torch, np.ones((B, 1), np.float32))
    Y = dev(torch, np.ones((B, S, n), np.float32))
    cost = _capi.make_cost(4, 1, np.ones(4), 0.01, None, -1.0, 1.0)

    def fresh():
        f = lambda *s, dt=torch.float32: torch.full(s, 7.0, dtype=dt, device="cuda:0")  # noqa: E731
        return dict(P=dev(torch, p["P"]), xhat=dev(torch, p["xpred"]), status=torch.full((B,), 7, dtype=torch.int32, device="cuda:0"),
                    nis=f(B, dt=torch.float64), chi=f(B, S, n), ctrl=f(B, S, 1, 1), xm=f(B, n), Pm=f(B, n, n, dt=torch.float64),
                    eye=f(B, n, n))

    def untouched(o):
        assert np.array_equal(npy(o["P"]), p["P"]) and em.same_floats(npy(o["xhat"]), p["xpred"])
        for k in ("status", "nis", "chi", "ctrl", "xm", "Pm", "eye"):
            assert np.all(npy(o[k]) == 7), k

    def opts():
        return ukf_options(n, 0b0011, p["Qn"], p["Rn"])

    def bad_options():
        edits = [("mask", lambda o: setattr(o, "meas_mask", 0b10011)), ("Qn nan", lambda o: o.Qn.__setitem__(5, float("nan"))),
                 ("Rn 0", lambda o: o.Rn.__setitem__(0, 0.0)), ("Rn inf", lambda o: o.Rn.__setitem__(1, float("inf"))),
                 ("reserved", lambda o: o.reserved.__setitem__(2, 1))]
        for name in ("gamma", "wi"):
            for v in (0.0, -1.0, float("nan"), float("inf")):
                edits.append((f"{name} {v}", lambda o, name=name, v=v: setattr(o, name, v)))
        for name in ("wm0", "wc0"):
            for v in (float("nan"), float("-inf")):
                edits.append((f"{name} {v}", lambda o, name=name, v=v: setattr(o, name, v)))
        for what, edit in edits:
            o = opts()
            edit(o)
            yield what, o

    # The complete text each edit leaves in phnn_last_error, for the step, the sigma points and the moments alike: the
    # mask, Qn and Rn are reported under the EKF's struct name (k_ekf_update takes them), the rest under the UKF's.
    ekf_text = {"mask": "meas_mask has bits at or above n", "Qn": "Qn is not finite",
                "Rn": "Rn of a measured component is not positive and finite"}
    ukf_text = {"reserved": "reserved must be zero", "gamma": "gamma and wi must be positive and finite",
                "wi": "gamma and wi must be positive and finite", "wm0": "wm0 / wc0 is not finite", "wc0": "wm0 / wc0 is not finite"}
    good = opts()
    good.wm0, good.wc0 = -3.0, -0.5  # negative weights of sigma point 0 are the textbook's small alpha: allowed
    good.Rn[3] = float("nan")  # not measured: not looked at
    o = fresh()
    eng.ukf_step(o["xhat"], o["P"], u, 1, y, cost, "euler", 0.02, good, nis=o["nis"], status=o["status"])
    assert set(npy(o["status"])) <= {0, 2} and np.all(npy(o["nis"]) != 7)
    nolog = dict(log_xhat=torch.zeros(2, B, n, device="cuda:0"), step=-1)
    for what, opt in bad_options():
        o = fresh()
        with pytest.raises(PhnnError, match="error -") as stp:
            eng.ukf_step(o["xhat"], o["P"], u, 1, y, cost, "euler", 0.02, opt, nis=o["nis"], status=o["status"])
        with pytest.raises(PhnnError, match="error -") as sig:
            eng.ukf_sigma(o["xhat"], o["P"], opt, u=u, chi=o["chi"], ctrl=o["ctrl"])
        with pytest.raises(PhnnError, match="error -") as mom:
            eng.ukf_moments(Y, B, opt, xm=o["xm"], Pm=o["Pm"], eye=o["eye"])
        untouched(o)
        key = what.split()[0]
        full = "phnn_ekf_options: " + ekf_text[key] if key in ekf_text else "phnn_ukf_options: " + ukf_text[key]
        assert str(stp.value) == str(sig.value) == str(mom.value) == "phnn_mpc error -1: " + full, what
    o, good = fresh(), opts()
    with pytest.raises(PhnnError, match="step source"):
        eng.ukf_step(o["xhat"], o["P"], u, 1, y, cost, "euler", 0.02, good, nis=o["nis"], status=o["status"], log=nolog)
    with pytest.raises(ValueError, match="Unknown integrator"):
        eng.ukf_step(o["xhat"], o["P"], u, 1, y, cost, 7, 0.02, good, nis=o["nis"], status=o["status"])
    with pytest.raises(PhnnError, match="dt"):
        eng.ukf_step(o["xhat"], o["P"], u, 1, y, cost, "euler", float("nan"), good, nis=o["nis"], status=o["status"])
    upside = _capi.make_cost(4, 1, np.ones(4), 0.01, None, 1.0, -1.0)
    with pytest.raises(PhnnError, match="error -"):
        eng.ukf_step(o["xhat"], o["P"], u, 1, y, upside, "euler", 0.02, good, nis=o["nis"], status=o["status"])
    untouched(o)
    assert np.all(npy(nolog["log_xhat"]) == 0)
    # NULL required buffers, B < 0, B == 0 through the C-ABI
    lib, st = eng.lib, eng._stream()
    a = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ws = torch.zeros(eng.ukf_workspace_bytes(B), dtype=torch.uint8, device="cuda:0")
    g = C.byref(good)
    assert lib.phnn_ukf_sigma(eng.h, a(x), None, a(u), 1, B, g, a(o["chi"]), a(o["ctrl"]), st) == -1
    assert lib.phnn_ukf_sigma(eng.h, a(x), a(o["P"]), None, 1, B, g, a(o["chi"]), a(o["ctrl"]), st) == -1
    assert lib.phnn_ukf_sigma(eng.h, a(x), a(o["P"]), a(u), 1, -1, g, a(o["chi"]), a(o["ctrl"]), st) == -1
    assert lib.phnn_ukf_sigma(eng.h, None, None, None, 1, 0, g, None, None, st) == 0
    assert lib.phnn_ukf_moments(eng.h, a(Y), n, B, g, a(o["xm"]), None, a(o["eye"]), st) == -1
    assert lib.phnn_ukf_moments(eng.h, a(Y), -1, B, g, a(o["xm"]), a(o["Pm"]), a(o["eye"]), st) == -1
    assert lib.phnn_ukf_moments(eng.h, None, n, 0, g, None, None, None, st) == 0
    assert lib.phnn_ukf_step(eng.h, a(o["xhat"]), a(o["P"]), a(u), 1, a(y), n, B, None, 0, 0.02, g, None, None, a(o["status"]), None,
                             None, st) == -1  # no workspace
    assert lib.phnn_ukf_step(eng.h, a(o["xhat"]), a(o["P"]), a(u), 1, None, n, B, None, 0, 0.02, g, None, None, a(o["status"]), None,
                             a(ws), st) == -1  # something is measured and there is no y
    assert lib.phnn_ukf_step(eng.h, a(o["xhat"]), a(o["P"]), a(u), 1, a(y), n, B, None, 0, 0.02, None, None, None, a(o["status"]), None,
                             a(ws), st) == -1  # no options
    assert lib.phnn_ukf_step(eng.h, None, None, None, 1, None, n, 0, None, 0, 0.02, g, None, None, None, None, None, st) == 0
    assert eng.ukf_workspace_bytes(-1) == 0 and eng.ukf_workspace_bytes(0) > 0 and eng.ukf_workspace_bytes(65) >= eng.ukf_workspace_bytes(17)
    torch.cuda.synchronize()
    untouched(o)


# ----------------------------------------------------------------------------- 7. the closed loop
KW = dict(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4)


@pytest.mark.parametrize("which", ["Adam", "GaussNewton"])
def test_closed_loop_with_a_ukf(torch, which):
    from phnn_mpc_amd.closed_loop import PlantScenario, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.estimation import EKF, UKF
    c = _controller(torch, which)
    nb, steps = 8, 5
    rng = np.random.default_rng(20)
    X0 = rng.uniform(-1, 1, size=(nb, 4)) * [0.2, 0.08, 0.1, 0.1]
    sc = PlantScenario(meas_sigma=[0.01, 0.005, 0.05, 0.05], seed=0xE57)
    ukf = UKF(**KW)
    eager, graphed = (run_mpc_batch_device(c, X0, steps, use_graph=g, scenario=sc, estimator=ukf) for g in (False, True))
    assert set(eager) == {"states", "controls", "done_step", "disturbance", "estimates", "nis", "ekf_status"}
    assert eager["estimates"].shape == (steps + 1, nb, 4) and eager["estimates"].dtype == np.float32 and eager["nis"].shape == (steps, nb)
    for k in ("states", "controls", "estimates", "nis", "ekf_status", "done_step"):
        assert em.same_floats(eager[k], graphed[k]), k
    assert np.array_equal(eager["estimates"][0], X0.astype(np.float32)) and np.all(eager["nis"] > 0) and not eager["ekf_status"].any()
    host = run_mpc_batch(DevicePlant(torch, c.engine, sc), c, X0, steps, estimator=ukf)
    for k in ("controls", "estimates", "states", "nis"):
        assert np.array_equal(np.asarray(eager[k], np.float64), np.asarray(host[k], np.float64)), k
    # it is the unscented filter that ran: near the EKF's estimates on this smooth model, and not the same numbers
    ekf = run_mpc_batch_device(c, X0, steps, scenario=sc, estimator=EKF(**KW))
    assert np.array_equal(ekf["controls"][0], eager["controls"][0]) and not np.array_equal(ekf["estimates"][1:], eager["estimates"][1:])
    assert np.abs(ekf["estimates"].astype(np.float64) - eager["estimates"]).max() < 1e-3


def test_closed_loop_with_a_ukf_and_tracking(torch):
    from phnn_mpc_amd.closed_loop import PlantScenario, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.estimation import UKF
    from phnn_mpc_amd.feedback import Tracking
    c = _controller(torch, "Adam")
    nb, steps = 8, 5
    rng = np.random.default_rng(21)
    X0 = rng.uniform(-1, 1, size=(nb, 4)) * [0.2, 0.08, 0.1, 0.1]
    sc = PlantScenario(meas_sigma=[0.01, 0.005, 0.05, 0.05], seed=0xE57)
    ukf, tr = UKF(**KW), Tracking(2)
    eager, graphed = (run_mpc_batch_device(c, X0, steps, use_graph=g, scenario=sc, estimator=ukf, track=tr) for g in (False, True))
    for k in ("states", "controls", "estimates", "nis", "ekf_status", "track_status", "track_dev"):
        assert em.same_floats(eager[k], graphed[k]), k
    host = run_mpc_batch(DevicePlant(torch, c.engine, sc), c, X0, steps, estimator=ukf, track=tr)
    for k in ("controls", "estimates", "states", "nis"):
        assert np.array_equal(np.asarray(eager[k], np.float64), np.asarray(host[k], np.float64)), k
    assert not eager["ekf_status"].any() and np.all(eager["nis"] > 0)
