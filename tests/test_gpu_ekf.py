"""The batched extended Kalman filter on the device.

  1 k_ekf_update       bits == ekf_model.update for n in {2, 3, 4}, every mask kind, B in {1, 17, 65} (one thread, a partial
                       workgroup, a workgroup plus one), dropouts and failures mixed into the batch, optional outputs
                       NULL and given, log rows from a device counter and from step_host
  2 phnn_ekf_step      bits == the four calls made by hand through the existing entry points (estimation.EKF.step)
  3 trusting the model P = 0, Qn = 0: six filter steps reproduce K1's H = 6 trajectory, whatever y holds
  4 footprint          both entry points in guarded buffers (tests/footprint.py)
  5 refusals           PHNN_ERR_INVALID_ARG with no output touched
  6 closed loop        DeviceClosedLoop(estimator=): graphed == eager, and == run_mpc_batch(estimator=) on the same engine
"""
import ctypes as C
import os

import numpy as np
import pytest
import yaml

import ekf_model as em
import footprint as fp
import oracle_lib as ol
from test_gpu_mppi import engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
N3_SPEC = "odefunc<n=3,hid=128,f16x2>"
_N3 = {}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def engine_n(n):
    """A handle with n state components: k_ekf_update reads none of its weights."""
    if n == 4:
        return engine("phnn_cartpole")
    if n == 2:
        return engine("odefunc_pendulum")
    if "eng" not in _N3:
        import variant_census as vc
        from phnn_mpc_amd.engine import RolloutEngine
        s = vc.CENSUS[N3_SPEC]
        _N3["eng"] = RolloutEngine(vc.build_state_dict(N3_SPEC, s), "cuda:0", **vc.engine_kwargs(s))
    return _N3["eng"]


def options(p, n):
    from phnn_mpc_amd import _capi
    o = _capi.EkfOptions()
    o.meas_mask = p["mask"]
    for i in range(n * n):
        o.Qn[i] = float(p["Qn"].reshape(-1)[i])
    for i in range(n):
        o.Rn[i] = float(p["Rn"][i])
    return o


def npy(t):
    return t.detach().cpu().numpy()


def dev(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0")


# ----------------------------------------------------------------------------- 1. the update kernel against the model
@pytest.mark.parametrize("n,name", [(n, name) for n in (2, 3, 4) for name in em.MASKS[n]])
def test_update_equals_the_model_bit_for_bit(torch, n, name):
    eng, mask = engine_n(n), em.MASKS[n][name]
    assert eng.n == n
    for B in (1, 17, 65):
        p = em.seeded_problem(1000 * n + B, B, n, mask)
        where = em.plant_cases(p, np.random.default_rng(B))
        ref = em.update(**p)
        if B > 1:
            assert set(ref["status"][list(where.values())]) == ({1, 2} if mask else {2}) and (ref["status"] == 0).sum() >= B - 4
        o = options(p, n)
        t = {k: dev(torch, p[k]) for k in ("xpred", "A", "y")}
        P = dev(torch, p["P"])
        r = eng.ekf_update(t["xpred"], t["A"], t["y"], P, o)
        assert r["P"] is P
        for k in ("xhat", "P", "nis", "innov", "status"):
            assert em.same_floats(npy(r[k]), ref[k]), (B, k)
        # the optional outputs left NULL; the log rows from a device counter and from step_host
        T = 3
        for src in ("dev", "host"):
            P2 = dev(torch, p["P"])
            lx = torch.full((T + 1, B, n), 7.0, dtype=torch.float32, device="cuda:0")
            ln = torch.full((T, B), 7.0, dtype=torch.float64, device="cuda:0")
            log = dict(log_xhat=lx, log_nis=ln)
            step = 1 if src == "dev" else 2
            log.update(step_dev=torch.tensor([step], dtype=torch.int32, device="cuda:0")) if src == "dev" else log.update(step=step)
            r2 = eng.ekf_update(t["xpred"], t["A"], t["y"], P2, o, nis=False, innov=False, log=log)
            assert r2["nis"] is None and r2["innov"] is None
            for k in ("xhat", "P", "status"):
                assert em.same_floats(npy(r2[k]), ref[k]), (B, src, k)
            lx, ln = npy(lx), npy(ln)
            assert em.same_floats(lx[step + 1], ref["xhat"]) and em.same_floats(ln[step], ref["nis"])
            assert np.all(np.delete(lx, step + 1, axis=0) == 7.0) and np.all(np.delete(ln, step, axis=0) == 7.0)


# ----------------------------------------------------------------------------- 2. the step against the four calls by hand
STEP_MODELS = {"phnn_cartpole": (0, 1), "canonical_cartpole": (0, 2), "odefunc_pendulum": (0,)}


@pytest.mark.parametrize("model", list(STEP_MODELS))
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_step_equals_the_four_calls_by_hand(torch, model, integ):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.estimation import EKF
    eng = engine(model)
    n, m, H = eng.n, eng.m, 3
    ekf = EKF(measured=STEP_MODELS[model], Qn=np.linspace(1e-6, 1e-4, n), Rn=1e-3, P0=0.02)
    o = ekf.options(n)
    cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0)
    for B in (1, 17):
        rng = np.random.default_rng(50 + B)
        x0 = (0.3 * rng.normal(size=(B, n))).astype(np.float32)
        u = rng.uniform(-4.0, 4.0, size=(B, H, m)).astype(np.float32)  # some of them outside the bounds
        assert B == 1 or ((u[:, 0] < -1.5).any() and (u[:, 0] > 2.0).any())
        y = (x0 + 0.05 * rng.normal(size=(B, n))).astype(np.float32)
        y[:, [i for i in range(n) if i not in ekf.measured]] = np.nan
        for c in (cost, None):
            xhat, P = dev(torch, x0), dev(torch, ekf.initial(x0)[1])
            hand = ekf.step(eng, xhat, P, dev(torch, u[:, 0]), dev(torch, y), c, integ, 0.02, opt=o)
            got = eng.ekf_step(xhat, P, dev(torch, u), H * m, dev(torch, y), c, integ, 0.02, o, nis=True, innov=True)
            assert got["xhat"] is xhat and got["P"] is P
            for k in ("xhat", "P", "nis", "innov", "status"):
                assert em.same_floats(npy(got[k]), npy(hand[k])), (B, k, c is None)
            assert not npy(got["status"]).any() and np.all(npy(got["nis"]) > 0)
            assert not np.array_equal(npy(xhat), x0)


# ----------------------------------------------------------------------------- 3. trusting the model reproduces the model
@pytest.mark.parametrize("model,integ", [("phnn_cartpole", "euler"), ("phnn_cartpole", "rk4"), ("odefunc_pendulum", "euler")])
def test_zero_covariance_reproduces_the_rollout(torch, model, integ):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.estimation import EKF
    eng = engine(model)
    n, m, T, B = eng.n, eng.m, 6, 17
    rng = np.random.default_rng(6)
    x0 = (0.3 * rng.normal(size=(B, n))).astype(np.float32)
    u = dev(torch, rng.uniform(-3.0, 3.0, size=(B, T, m)).astype(np.float32))
    cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0)
    _, traj = eng.rollout_cost(dev(torch, x0), u, cost, integ, 0.02, want_traj=True)
    o = EKF(measured=(0,) if n == 2 else (0, 1), Qn=0.0, Rn=1e-4, P0=0.0).options(n)
    xhat, P = dev(torch, x0), torch.zeros(B, n, n, dtype=torch.float64, device="cuda:0")
    ws = {}
    for t in range(T):
        y = (1e3 * rng.normal(size=(B, n))).astype(np.float32)  # garbage, some of it dropped
        y[rng.random(B) < 0.3, 0] = np.nan
        r = eng.ekf_step(xhat, P, u.reshape(-1)[t * m:], T * m, dev(torch, y), cost, integ, 0.02, o, workspace=ws)
        assert em.same_floats(npy(xhat), npy(traj[:, t + 1])), t
        assert not npy(P).any() and set(npy(r["status"])) <= {0, 1}


# ----------------------------------------------------------------------------- 4. footprint
class EkfUpdateOp(fp.Op):
    """phnn_ekf_update at step 1 of 3; drop: the optional outputs left NULL."""

    def __init__(self, n, B, mask, rng, drop=()):
        super().__init__()
        self.name, self.n, self.B, self.drop = f"ekf_update n{n} B{B} mask{mask:04b} drop={','.join(drop) or '-'}", n, B, set(drop)
        self.p = p = em.seeded_problem(int(rng.integers(1 << 30)), B, n, mask)
        em.plant_cases(p, rng)
        f32, f64 = np.float32, np.float64
        self.add("xpred", f32, (B, n), fp.IN, p["xpred"])
        self.add("A", f32, (B, n, n), fp.IN, p["A"])
        self.add("y", f32, (B, n), fp.IN, p["y"])  # NaN at the unmeasured components: never read
        self.add("P", f64, (B, n, n), fp.INOUT, p["P"])
        self.add("xhat", f32, (B, n), fp.OUT)
        self.add("status", np.int32, (B,), fp.OUT)
        if "nis" not in self.drop:
            self.add("nis", f64, (B,), fp.OUT)
        if "innov" not in self.drop:
            self.add("innov", f64, (B, n), fp.OUT)
        if "log" not in self.drop:
            self.add("log_xhat", f32, (4, B, n), fp.INOUT, np.zeros((4, B, n), f32))
            self.add("log_nis", f64, (3, B), fp.INOUT, np.zeros((3, B)))

    def _log(self, p):
        from phnn_mpc_amd import _capi
        if "log" in self.drop:
            return None
        lg = _capi.EkfLog()
        lg.log_xhat_dev, lg.log_nis_dev, lg.step_host = p["log_xhat"], p["log_nis"], 1
        return lg

    def call(self, eng, p):
        lg = self._log({k: v.value for k, v in p.items()})
        o = options(self.p, self.n)
        fp.check_rc(eng, eng.lib.phnn_ekf_update(eng.h, p["xpred"], self.n, p["A"], p["y"], self.n, self.B, C.byref(o), p["P"],
                                                 p["xhat"], p.get("nis"), p.get("innov"), p["status"],
                                                 C.byref(lg) if lg else None, eng._stream()))

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        log = None if "log" in self.drop else dict(log_xhat=t["log_xhat"], log_nis=t["log_nis"], step=1)
        r = eng.ekf_update(t["xpred"], t["A"], t["y"], t["P"], options(self.p, self.n), nis="nis" not in self.drop,
                           innov="innov" not in self.drop, log=log)
        t.update({k: v for k, v in r.items() if v is not None})
        return {b.name: t[b.name] for b in self.outputs()}


class EkfStepOp(fp.Op):
    """phnn_ekf_step with the first control of an (B,H,m) sequence, at step 1 of 3."""
    H = 3

    def __init__(self, eng, B, measured, integ, rng, bounded=True, drop=()):
        from phnn_mpc_amd import _capi
        from phnn_mpc_amd.estimation import EKF
        super().__init__()
        n, m = eng.n, eng.m
        self.name, self.n, self.m, self.B, self.integ, self.drop = f"ekf_step B{B} {integ} drop={','.join(drop) or '-'}", n, m, B, integ, set(drop)
        self.ekf = EKF(measured=measured, Qn=1e-5, Rn=1e-3, P0=0.02)
        self.cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0) if bounded else None
        f32, f64 = np.float32, np.float64
        x0 = (0.3 * rng.normal(size=(B, n))).astype(f32)
        y = (x0 + 0.05 * rng.normal(size=(B, n))).astype(f32)
        y[:, [i for i in range(n) if i not in measured]] = np.nan
        nbytes = eng.ekf_workspace_bytes(B)
        assert nbytes > 0
        self.add("xhat", f32, (B, n), fp.INOUT, x0)
        self.add("P", f64, (B, n, n), fp.INOUT, self.ekf.initial(x0)[1])
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
        o = self.ekf.options(self.n)
        rc = eng.lib.phnn_ekf_step(eng.h, p["xhat"], p["P"], p["u"], self.H * self.m, p["y"], self.n, self.B,
                                   C.byref(self.cost) if self.cost is not None else None, eng._integ(self.integ), 0.02, C.byref(o),
                                   p.get("nis"), p.get("innov"), p["status"], C.byref(lg) if lg else None, p["ws"], eng._stream())
        fp.check_rc(eng, rc)

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        log = None if "log" in self.drop else dict(log_xhat=t["log_xhat"], log_nis=t["log_nis"], step=1)
        r = eng.ekf_step(t["xhat"], t["P"], t["u"], self.H * self.m, t["y"], self.cost, self.integ, 0.02, self.ekf.options(self.n),
                         nis="nis" not in self.drop, innov="innov" not in self.drop, log=log)
        t.update({k: v for k, v in r.items() if v is not None})
        return {b.name: t[b.name] for b in self.outputs() if b.role != fp.WS}


@pytest.mark.parametrize("n", [2, 3, 4])
def test_footprint_of_the_update(torch, n):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = engine_n(n)
    rep = Report(f"phnn_ekf_update n{n}")
    for B in (17, 65):
        for name, drop in (("all", ()), ("single", ("nis", "innov", "log")), ("empty", ("log",))):
            op = EkfUpdateOp(n, B, em.MASKS[n][name], rng_of("ekf_update", n, B, name), drop)
            ff = footprint(rep, torch, eng, op)
            if not drop:  # the call wrote row 2 of the estimates' log and row 1 of the nis log, nothing else of them
                for k, row, width in (("log_xhat", 2, 4 * n * B), ("log_nis", 1, 8 * B)):
                    got = ff[2].written(k, 0)
                    assert got is not None and row * width <= got[0] and got[1] <= (row + 1) * width, (k, got)
    rep.finish()


@pytest.mark.parametrize("model,integ", [("phnn_cartpole", "euler"), ("canonical_cartpole", "rk4"), ("odefunc_pendulum", "rk4")])
def test_footprint_of_the_step(torch, model, integ):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = engine(model)
    rep = Report(f"phnn_ekf_step {model} {integ}")
    measured = (0,) if eng.n == 2 else (0, 1)
    for B in (17, 65):
        for bounded, drop in ((True, ()), (False, ("nis", "innov", "log"))):
            footprint(rep, torch, eng, EkfStepOp(eng, B, measured, integ, rng_of("ekf_step", model, B, bounded), bounded, drop))
    rep.finish()


# ----------------------------------------------------------------------------- 5. refusals
def test_bad_arguments_are_refused_and_nothing_is_written(torch):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    eng = engine("phnn_cartpole")
    n, B = 4, 5
    p = em.seeded_problem(3, B, n, 0b0011)
    t = {k: dev(torch, p[k]) for k in ("xpred", "A", "y")}
    cost = _capi.make_cost(4, 1, np.ones(4), 0.01, None, -1.0, 1.0)

    def fresh():
        return dict(P=dev(torch, p["P"]), xhat=torch.full((B, n), 7.0, device="cuda:0"),
                    status=torch.full((B,), 7, dtype=torch.int32, device="cuda:0"),
                    nis=torch.full((B,), 7.0, dtype=torch.float64, device="cuda:0"))

    def untouched(o):
        assert np.array_equal(npy(o["P"]), p["P"]) and np.all(npy(o["xhat"]) == 7) and np.all(npy(o["status"]) == 7) and np.all(npy(o["nis"]) == 7)

    def bad_options():
        for what, edit in (("mask", lambda o: setattr(o, "meas_mask", 0b10011)), ("Qn nan", lambda o: o.Qn.__setitem__(5, float("nan"))),
                           ("Qn inf", lambda o: o.Qn.__setitem__(15, float("inf"))), ("Rn 0", lambda o: o.Rn.__setitem__(0, 0.0)),
                           ("Rn < 0", lambda o: o.Rn.__setitem__(1, -1.0)), ("Rn nan", lambda o: o.Rn.__setitem__(1, float("nan"))),
                           ("Rn inf", lambda o: o.Rn.__setitem__(0, float("inf"))), ("reserved", lambda o: o.reserved.__setitem__(2, 1))):
            o = options(p, n)
            edit(o)
            yield what, o

    # the complete text each edit leaves in phnn_last_error, for the update and for the step alike
    text = {"mask": "meas_mask has bits at or above n", "Qn": "Qn is not finite",
            "Rn": "Rn of a measured component is not positive and finite", "reserved": "reserved must be zero"}
    good = options(p, n)
    good.Rn[3] = float("nan")  # not measured: not looked at
    o = fresh()
    eng.ekf_update(t["xpred"], t["A"], t["y"], o["P"], good, xhat=o["xhat"], nis=o["nis"], status=o["status"])
    assert not npy(o["status"]).any()
    nolog = dict(log_xhat=torch.zeros(2, B, n, device="cuda:0"), step=-1)
    for what, opt in bad_options():
        o = fresh()
        with pytest.raises(PhnnError, match="error -") as upd:
            eng.ekf_update(t["xpred"], t["A"], t["y"], o["P"], opt, xhat=o["xhat"], nis=o["nis"], status=o["status"])
        with pytest.raises(PhnnError, match="error -") as stp:
            eng.ekf_step(o["xhat"], o["P"], t["xpred"], n, t["y"], cost, "euler", 0.02, opt, nis=o["nis"], status=o["status"])
        untouched(o)
        assert str(upd.value) == str(stp.value) == "phnn_mpc error -1: phnn_ekf_options: " + text[what.split()[0]], what
    o = fresh()
    with pytest.raises(PhnnError, match="step source"):
        eng.ekf_update(t["xpred"], t["A"], t["y"], o["P"], good, xhat=o["xhat"], nis=o["nis"], status=o["status"], log=nolog)
    with pytest.raises(PhnnError, match="step source"):
        eng.ekf_step(o["xhat"], o["P"], t["xpred"], n, t["y"], cost, "euler", 0.02, good, nis=o["nis"], status=o["status"], log=nolog)
    with pytest.raises(ValueError, match="Unknown integrator"):
        eng.ekf_step(o["xhat"], o["P"], t["xpred"], n, t["y"], cost, 7, 0.02, good, nis=o["nis"], status=o["status"])
    with pytest.raises(PhnnError, match="dt"):
        eng.ekf_step(o["xhat"], o["P"], t["xpred"], n, t["y"], cost, "euler", float("nan"), good, nis=o["nis"], status=o["status"])
    untouched(o)
    assert np.all(npy(nolog["log_xhat"]) == 0)
    # NULL required buffers, B < 0, B == 0 through the C-ABI
    lib, st = eng.lib, eng._stream()
    a = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.phnn_ekf_update(eng.h, a(t["xpred"]), n, None, a(t["y"]), n, B, C.byref(good), a(o["P"]), a(o["xhat"]), None, None,
                               a(o["status"]), None, st) == -1
    assert lib.phnn_ekf_update(eng.h, a(t["xpred"]), n, a(t["A"]), a(t["y"]), n, -1, C.byref(good), a(o["P"]), a(o["xhat"]), None,
                               None, a(o["status"]), None, st) == -1
    assert lib.phnn_ekf_update(eng.h, None, n, None, None, n, 0, C.byref(good), None, None, None, None, None, None, st) == 0
    assert lib.phnn_ekf_step(eng.h, a(o["xhat"]), a(o["P"]), a(t["xpred"]), n, a(t["y"]), n, B, None, 0, 0.02, C.byref(good), None,
                             None, a(o["status"]), None, None, st) == -1
    assert lib.phnn_ekf_step(eng.h, None, None, None, n, None, n, 0, None, 0, 0.02, C.byref(good), None, None, None, None, None, st) == 0
    assert eng.ekf_workspace_bytes(-1) == 0 and eng.ekf_workspace_bytes(0) > 0 and eng.ekf_workspace_bytes(65) >= eng.ekf_workspace_bytes(17)
    torch.cuda.synchronize()
    untouched(o)


# ----------------------------------------------------------------------------- 6. the closed loop
class DevicePlant:
    """run_mpc_batch's simulator served by the device plant kernel, so that the host-driven loop sees the states and the
    measurements of the device loop bit for bit (the numpy plant differs by the device's sin / cos)."""

    def __init__(self, torch, eng, scenario, dt=0.02):
        from phnn_mpc_amd import _capi
        self.torch, self.eng, self.plant = torch, eng, _capi.Plant.default(dt)
        self.ex = _capi.PlantEx()
        for i in range(4):
            self.ex.meas_sigma[i] = float(scenario.meas_sigma[i])
        self.ex.seed, self.ex.plant_offset = scenario.seed, scenario.plant_offset
        self.scenario = None

    def reset(self, x0):
        torch = self.torch
        self.state = torch.tensor(np.asarray(x0, np.float64).reshape(-1, 4), device=self.eng.device)
        self.y32 = self.state.to(torch.float32)
        self.done = torch.full((self.state.shape[0],), -1, dtype=torch.int32, device=self.eng.device)
        self.t = 0
        return npy(self.state)

    def step(self, u):
        action = self.torch.tensor(np.asarray(u, np.float32).reshape(-1), device=self.eng.device)
        self.eng.plant_step(self.plant, self.state, action, 1, state_f32=self.y32, done_step=self.done, step=self.t, ex=self.ex)
        self.t += 1
        return npy(self.state), npy(self.done) >= 0

    def measurement(self):
        return npy(self.y32)


def _controller(torch, which):
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(horizon=5, optimizer_steps=3)
    if which == "GaussNewton":
        cfg["mpc"].update(optimizer="GaussNewton", optimizer_steps=2, gn_line_steps=4)
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights("phnn_cartpole").items()})
    c = create_mpc_from_config(m, cfg)
    assert c.optimizer_type == which
    return c


@pytest.mark.parametrize("which", ["Adam", "GaussNewton"])
def test_closed_loop_with_an_estimator(torch, which):
    from phnn_mpc_amd.closed_loop import PlantScenario, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.estimation import EKF
    c = _controller(torch, which)
    nb, steps = 8, 5
    rng = np.random.default_rng(20)
    X0 = rng.uniform(-1, 1, size=(nb, 4)) * [0.2, 0.08, 0.1, 0.1]
    sc = PlantScenario(meas_sigma=[0.01, 0.005, 0.05, 0.05], seed=0xE57)
    ekf = EKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4)
    eager, graphed = (run_mpc_batch_device(c, X0, steps, use_graph=g, scenario=sc, estimator=ekf) for g in (False, True))
    assert set(eager) == {"states", "controls", "done_step", "disturbance", "estimates", "nis", "ekf_status"}
    assert eager["estimates"].shape == (steps + 1, nb, 4) and eager["estimates"].dtype == np.float32 and eager["nis"].shape == (steps, nb)
    for k in ("states", "controls", "estimates", "nis", "ekf_status", "done_step"):
        assert em.same_floats(eager[k], graphed[k]), k
    assert np.array_equal(eager["estimates"][0], X0.astype(np.float32)) and np.all(eager["nis"] > 0) and not eager["ekf_status"].any()
    host = run_mpc_batch(DevicePlant(torch, c.engine, sc), c, X0, steps, estimator=ekf)
    for k in ("controls", "estimates", "states", "nis"):
        assert np.array_equal(np.asarray(eager[k], np.float64), np.asarray(host[k], np.float64)), k
    from phnn_mpc_amd.closed_loop import DeviceClosedLoop
    with pytest.raises(ValueError, match="differs from the controller's"):  # the filter would predict over another interval
        DeviceClosedLoop(c, X0, steps, dt=0.01, estimator=ekf)
    DeviceClosedLoop(c, X0, steps, dt=0.01)  # without an estimator a dt of the plant's own stays allowed
    # the estimator is in the loop: without it the same scenario gives other controls after the first step
    raw = run_mpc_batch_device(c, X0, steps, scenario=sc)
    assert set(raw) == {"states", "controls", "done_step", "disturbance"}
    assert np.array_equal(raw["controls"][0], eager["controls"][0]) and not np.array_equal(raw["controls"][1:], eager["controls"][1:])
