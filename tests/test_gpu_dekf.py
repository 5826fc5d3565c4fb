"""Input-disturbance estimation and offset-free control on the device.

  1 k_dekf_update      bits == dekf_model.update for the four (n, m), every mask kind, B in {1, 17, 65}, dropouts and
                       failures mixed into the batch, optional outputs NULL and given, log rows from a device counter and
                       from step_host
  2 reduction          zero d blocks: the x part == phnn_ekf_update's bits on the device, dhat keeps its bits
  3 phnn_dekf_step     bits == the four calls made by hand (estimation.DisturbanceEKF.step); with dhat = 0 and zero d blocks
                       its x part == phnn_ekf_step's
  4 compensation       phnn_dist_compensate == dekf_model.compensate
  5 footprint          the three entry points in guarded buffers (tests/footprint.py)
  6 refusals           PHNN_ERR_INVALID_ARG / PHNN_ERR_UNSUPPORTED with no output touched
  7 closed loop        DeviceClosedLoop(estimator=DisturbanceEKF): graphed == eager, and == run_mpc_batch on the same engine,
                       without and with track=
"""
import ctypes as C

import numpy as np
import pytest

import dekf_model as dm
import ekf_model as em
import footprint as fp
import variant_census as vc
from test_gpu_ekf import DevicePlant, _controller, dev, npy
from test_gpu_footprint import engine as census_engine
from test_gpu_mppi import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def engine_nm(n, m):
    """A handle with n state and m input components: k_dekf_update reads none of its weights."""
    eng = census_engine(vc.NM_SPEC[(n, m)])
    assert (eng.n, eng.m) == (n, m)
    return eng


def tensors(torch, p):
    return {k: dev(torch, p[k]) for k in ("xpred", "A", "Bm", "y")}


# ----------------------------------------------------------------------------- 1. the update kernel against the model
@pytest.mark.parametrize("n,m,name", [(n, m, name) for n, m in dm.NM for name in em.MASKS[n]])
def test_update_equals_the_model_bit_for_bit(torch, n, m, name):
    eng, mask = engine_nm(n, m), em.MASKS[n][name]
    for B in (1, 17, 65):
        p = dm.seeded_problem(1000 * n + 100 * m + B, B, n, m, mask)
        where = dm.plant_cases(p, np.random.default_rng(B))
        ref = dm.update(**p)
        if B > 1:
            assert set(ref["status"][[where[k] for k in dm.FAILS if k in where]]) == {2} and (ref["status"] == 0).sum() >= B - 6
            assert not mask or ref["status"][where["dropout"]] == 1
        o = dm.dekf_options(p)
        t = tensors(torch, p)
        Pz, dhat = dev(torch, p["Pz"]), dev(torch, p["dhat"])
        r = eng.dekf_update(t["xpred"], t["A"], t["Bm"], t["y"], Pz, dhat, o)
        assert r["P"] is Pz and r["dhat"] is dhat
        for k in ("xhat", "dhat", "P", "nis", "innov", "status"):
            assert dm.same_floats(npy(r[k]), ref[k]), (B, k)
        # the optional outputs left NULL; the log rows from a device counter and from step_host
        T = 3
        for src in ("dev", "host"):
            P2, d2 = dev(torch, p["Pz"]), dev(torch, p["dhat"])
            lx = torch.full((T + 1, B, n), 7.0, dtype=torch.float32, device="cuda:0")
            ld = torch.full((T + 1, B, m), 7.0, dtype=torch.float32, device="cuda:0")
            ln = torch.full((T, B), 7.0, dtype=torch.float64, device="cuda:0")
            log = dict(log_xhat=lx, log_dhat=ld, log_nis=ln)
            step = 1 if src == "dev" else 2
            log.update(step_dev=torch.tensor([step], dtype=torch.int32, device="cuda:0")) if src == "dev" else log.update(step=step)
            r2 = eng.dekf_update(t["xpred"], t["A"], t["Bm"], t["y"], P2, d2, o, nis=False, innov=False, log=log)
            assert r2["nis"] is None and r2["innov"] is None
            for k in ("xhat", "dhat", "P", "status"):
                assert dm.same_floats(npy(r2[k]), ref[k]), (B, src, k)
            lx, ld, ln = npy(lx), npy(ld), npy(ln)
            assert dm.same_floats(lx[step + 1], ref["xhat"]) and dm.same_floats(ld[step + 1], ref["dhat"])
            assert dm.same_floats(ln[step], ref["nis"])
            assert np.all(np.delete(lx, step + 1, axis=0) == 7.0) and np.all(np.delete(ld, step + 1, axis=0) == 7.0)
            assert np.all(np.delete(ln, step, axis=0) == 7.0)


# ----------------------------------------------------------------------------- 2. the reduction to the plain filter
REDUCTION = [(4, 1, (0, 1)), (4, 2, (0, 2)), (2, 1, (0,)), (3, 1, (0, 1, 2)), (4, 1, ())]


def zero_d_blocks(p, n):
    for k in ("Pz", "Qz"):
        p[k][..., n:, :] = 0.0
        p[k][..., :, n:] = 0.0


@pytest.mark.parametrize("n,m,measured", REDUCTION)
def test_zero_d_blocks_reduce_to_the_plain_update(torch, n, m, measured):
    from test_gpu_ekf import options as ekf_options
    eng, mask, B = engine_nm(n, m), em.mask_of(measured), 65
    p = dm.seeded_problem(7 + n + m, B, n, m, mask)
    zero_d_blocks(p, n)
    t = tensors(torch, p)
    Pz, dhat = dev(torch, p["Pz"]), dev(torch, p["dhat"])
    r = eng.dekf_update(t["xpred"], t["A"], t["Bm"], t["y"], Pz, dhat, dm.dekf_options(p))
    plain = dict(mask=mask, Qn=np.ascontiguousarray(p["Qz"][:n, :n]), Rn=p["Rn"])
    P = dev(torch, np.ascontiguousarray(p["Pz"][:, :n, :n]))
    r0 = eng.ekf_update(t["xpred"], t["A"], t["y"], P, ekf_options(plain, n))
    Pz = npy(Pz)
    assert dm.same_floats(npy(r["xhat"]), npy(r0["xhat"])) and dm.same_floats(Pz[:, :n, :n], npy(P))
    assert dm.same_floats(npy(r["nis"]), npy(r0["nis"])) and dm.same_floats(npy(r["innov"]), npy(r0["innov"]))
    assert dm.same_floats(npy(dhat), p["dhat"])
    assert not Pz[:, n:, :].any() and not np.signbit(Pz[:, n:, :]).any() and not npy(r["status"]).any()


# ----------------------------------------------------------------------------- 3. the step against the four calls by hand
def step_engine(model):
    return engine(model) if model in ("phnn_cartpole", "odefunc_pendulum") else census_engine(model)


STEP_MODELS = {"phnn_cartpole": (0, 1), vc.NM_SPEC[(4, 2)]: (0, 2), "odefunc_pendulum": (0,)}


@pytest.mark.parametrize("model", list(STEP_MODELS))
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_step_equals_the_four_calls_by_hand(torch, model, integ):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.estimation import DisturbanceEKF
    eng = step_engine(model)
    n, m, H = eng.n, eng.m, 3
    ekf = DisturbanceEKF(measured=STEP_MODELS[model], Qn=np.linspace(1e-6, 1e-4, n), Rn=1e-3, P0=0.02, Qd=1e-5, Pd0=0.3, d0_hat=0.1)
    o = ekf.options(n, m)
    cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0)
    for B in (1, 17):
        rng = np.random.default_rng(50 + B)
        x0 = (0.3 * rng.normal(size=(B, n))).astype(np.float32)
        u = rng.uniform(-4.0, 4.0, size=(B, H, m)).astype(np.float32)  # some of them outside the bounds
        assert B == 1 or ((u[:, 0] < -1.5).any() and (u[:, 0] > 2.0).any())
        y = (x0 + 0.05 * rng.normal(size=(B, n))).astype(np.float32)
        y[:, [i for i in range(n) if i not in ekf.measured]] = np.nan
        _, d0, Pz0 = ekf.initial(x0, m)
        d0 = (d0 + 0.2 * rng.normal(size=(B, m))).astype(np.float32)
        for c in (cost, None):
            xhat, dhat, Pz = dev(torch, x0), dev(torch, d0), dev(torch, Pz0)
            hand = ekf.step(eng, xhat, dhat, Pz, dev(torch, u[:, 0]), dev(torch, y), c, integ, 0.02, opt=o)
            assert np.array_equal(npy(dhat), d0) and np.array_equal(npy(Pz), Pz0)  # the statement keeps its inputs
            got = eng.dekf_step(xhat, dhat, Pz, dev(torch, u), H * m, dev(torch, y), c, integ, 0.02, o, nis=True, innov=True)
            assert got["xhat"] is xhat and got["dhat"] is dhat and got["P"] is Pz
            for k in ("xhat", "dhat", "P", "nis", "innov", "status"):
                assert dm.same_floats(npy(got[k]), npy(hand[k])), (B, k, c is None)
            assert not npy(got["status"]).any() and np.all(npy(got["nis"]) > 0)
            # one Euler step moves no position by the control, so positions alone tell nothing of d yet; one RK4 step does
            assert not np.array_equal(npy(xhat), x0) and (integ == "euler" or not np.array_equal(npy(dhat), d0))


@pytest.mark.parametrize("model", ["phnn_cartpole", "odefunc_pendulum"])
def test_step_with_no_disturbance_reduces_to_the_plain_step(torch, model):
    """dhat = 0 and zero d blocks: the control row is c(u) + 0 = c(u) (u != -0.0), the model sees what K1's own clamp
    hands it in phnn_ekf_step, A is the same Jacobian: the x part equals phnn_ekf_step's bit for bit."""
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.estimation import EKF, DisturbanceEKF
    eng = step_engine(model)
    n, m, B = eng.n, eng.m, 17
    kw = dict(measured=STEP_MODELS[model], Qn=np.linspace(1e-6, 1e-4, n), Rn=1e-3, P0=0.02)
    ekf, dekf = EKF(**kw), DisturbanceEKF(Qd=0.0, Pd0=0.0, **kw)
    cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0)
    rng = np.random.default_rng(77)
    x0 = (0.3 * rng.normal(size=(B, n))).astype(np.float32)
    u = rng.uniform(-4.0, 4.0, size=(B, m)).astype(np.float32)
    assert not (u == 0).any()
    y = (x0 + 0.05 * rng.normal(size=(B, n))).astype(np.float32)
    for integ in ("euler", "rk4"):
        for c in (cost, None):
            xh, P = dev(torch, x0), dev(torch, ekf.initial(x0)[1])
            r0 = eng.ekf_step(xh, P, dev(torch, u), m, dev(torch, y), c, integ, 0.02, ekf.options(n), nis=True, innov=True)
            _, d0, Pz0 = dekf.initial(x0, m)
            xz, dz, Pz = dev(torch, x0), dev(torch, d0), dev(torch, Pz0)
            r = eng.dekf_step(xz, dz, Pz, dev(torch, u), m, dev(torch, y), c, integ, 0.02, dekf.options(n, m), nis=True, innov=True)
            assert dm.same_floats(npy(xz), npy(xh)) and dm.same_floats(npy(Pz)[:, :n, :n], npy(P)), (integ, c is None)
            assert dm.same_floats(npy(r["nis"]), npy(r0["nis"])) and dm.same_floats(npy(r["innov"]), npy(r0["innov"]))
            assert not npy(dz).any() and not npy(Pz)[:, n:, :].any() and not npy(r["status"]).any()


# ----------------------------------------------------------------------------- 4. the compensation
def compensate_case(rng, B, m, H):
    v = rng.uniform(-4.0, 4.0, size=(B, H, m)).astype(np.float32)
    d = rng.uniform(-1.0, 1.0, size=(B, m)).astype(np.float32)
    if B >= 17:
        d[0, 0], d[1, -1], d[2, 0], d[3] = np.nan, np.inf, -np.inf, 0.0
        v[4, 0, 0], v[1, 0, 0] = np.nan, np.nan
        v[5, 0], v[6, 0] = 3.9, -3.9  # outside the bounds
    return v, d


@pytest.mark.parametrize("m", [1, 2])
def test_compensation_equals_its_restatement(torch, m):
    from phnn_mpc_amd import _capi
    eng = engine_nm(4, m)
    cost = _capi.make_cost(4, m, np.ones(4), 0.01, None, -1.5, 2.0)
    for B in (1, 17, 65):
        for H in (1, 3):  # strides m and H m
            v, d = compensate_case(np.random.default_rng(10 * B + H + m), B, m, H)
            for c in (cost, None):
                ref_u, ref_s = dm.compensate(v[:, 0], d, c)
                u, s = eng.dist_compensate(dev(torch, v), H * m, dev(torch, d), c, status=True)
                assert dm.same_floats(npy(u), ref_u) and np.array_equal(npy(s), ref_s), (B, H, c is None)
                u2, s2 = eng.dist_compensate(dev(torch, v), H * m, dev(torch, d), c)  # the status left NULL
                assert s2 is None and dm.same_floats(npy(u2), ref_u)
                if B >= 17:
                    assert list(ref_s[:5]) == [1, 1, 1, 0, 0] and np.isnan(ref_u[4, 0]) and np.isnan(ref_u[1, 0])
                    assert np.all(np.isfinite(ref_u[[0, 2]])) and (c is None or (np.nanmax(ref_u) <= 2.0 and np.nanmin(ref_u) >= -1.5))


# ----------------------------------------------------------------------------- 5. footprint
class DekfUpdateOp(fp.Op):
    """phnn_dekf_update at step 1 of 3; drop: the optional outputs left NULL."""

    def __init__(self, n, m, B, mask, rng, drop=()):
        super().__init__()
        self.name, self.n, self.m, self.B, self.drop = f"dekf_update n{n} m{m} B{B} mask{mask:04b} drop={','.join(drop) or '-'}", n, m, B, set(drop)
        self.p = p = dm.seeded_problem(int(rng.integers(1 << 30)), B, n, m, mask)
        dm.plant_cases(p, rng)
        f32, f64, nz = np.float32, np.float64, n + m
        self.add("xpred", f32, (B, n), fp.IN, p["xpred"])
        self.add("A", f32, (B, n, n), fp.IN, p["A"])
        self.add("Bm", f32, (B, n, m), fp.IN, p["Bm"])
        self.add("y", f32, (B, n), fp.IN, p["y"])  # NaN at the unmeasured components: never read
        self.add("Pz", f64, (B, nz, nz), fp.INOUT, p["Pz"])
        self.add("dhat", f32, (B, m), fp.INOUT, p["dhat"])
        self.add("xhat", f32, (B, n), fp.OUT)
        self.add("status", np.int32, (B,), fp.OUT)
        if "nis" not in self.drop:
            self.add("nis", f64, (B,), fp.OUT)
        if "innov" not in self.drop:
            self.add("innov", f64, (B, n), fp.OUT)
        if "log" not in self.drop:
            self.add("log_xhat", f32, (4, B, n), fp.INOUT, np.zeros((4, B, n), f32))
            self.add("log_dhat", f32, (4, B, m), fp.INOUT, np.zeros((4, B, m), f32))
            self.add("log_nis", f64, (3, B), fp.INOUT, np.zeros((3, B)))

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        lg = None
        if "log" not in self.drop:
            lg = _capi.DekfLog()
            lg.log_xhat_dev, lg.log_dhat_dev, lg.log_nis_dev, lg.step_host = p["log_xhat"].value, p["log_dhat"].value, p["log_nis"].value, 1
        o = dm.dekf_options(self.p)
        fp.check_rc(eng, eng.lib.phnn_dekf_update(eng.h, p["xpred"], self.n, p["A"], p["Bm"], p["y"], self.n, self.B, C.byref(o),
                                                  p["Pz"], p["xhat"], p["dhat"], p.get("nis"), p.get("innov"), p["status"],
                                                  C.byref(lg) if lg else None, eng._stream()))

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        log = None if "log" in self.drop else dict(log_xhat=t["log_xhat"], log_dhat=t["log_dhat"], log_nis=t["log_nis"], step=1)
        r = eng.dekf_update(t["xpred"], t["A"], t["Bm"], t["y"], t["Pz"], t["dhat"], dm.dekf_options(self.p),
                            nis="nis" not in self.drop, innov="innov" not in self.drop, log=log)
        t.update({k: v for k, v in r.items() if v is not None and k != "P"})
        return {b.name: t[b.name] for b in self.outputs()}


class DekfStepOp(fp.Op):
    """phnn_dekf_step with the first control of an (B,H,m) sequence, at step 1 of 3."""
    H = 3

    def __init__(self, eng, B, measured, integ, rng, bounded=True, drop=()):
        from phnn_mpc_amd import _capi
        from phnn_mpc_amd.estimation import DisturbanceEKF
        super().__init__()
        n, m = eng.n, eng.m
        self.name, self.n, self.m, self.B, self.integ, self.drop = f"dekf_step B{B} {integ} drop={','.join(drop) or '-'}", n, m, B, integ, set(drop)
        self.ekf = DisturbanceEKF(measured=measured, Qn=1e-5, Rn=1e-3, P0=0.02, Qd=1e-6, Pd0=0.2)
        self.cost = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.5, 2.0) if bounded else None
        f32, f64, nz = np.float32, np.float64, n + m
        x0 = (0.3 * rng.normal(size=(B, n))).astype(f32)
        y = (x0 + 0.05 * rng.normal(size=(B, n))).astype(f32)
        y[:, [i for i in range(n) if i not in measured]] = np.nan
        nbytes = eng.dekf_workspace_bytes(B)
        assert nbytes > 0
        self.add("xhat", f32, (B, n), fp.INOUT, x0)
        self.add("dhat", f32, (B, m), fp.INOUT, (0.2 * rng.normal(size=(B, m))).astype(f32))
        self.add("Pz", f64, (B, nz, nz), fp.INOUT, self.ekf.initial(x0, m)[2])
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
            self.add("log_dhat", f32, (4, B, m), fp.INOUT, np.zeros((4, B, m), f32))
            self.add("log_nis", f64, (3, B), fp.INOUT, np.zeros((3, B)))

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        lg = None
        if "log" not in self.drop:
            lg = _capi.DekfLog()
            lg.log_xhat_dev, lg.log_dhat_dev, lg.log_nis_dev, lg.step_host = p["log_xhat"].value, p["log_dhat"].value, p["log_nis"].value, 1
        o = self.ekf.options(self.n, self.m)
        rc = eng.lib.phnn_dekf_step(eng.h, p["xhat"], p["dhat"], p["Pz"], p["u"], self.H * self.m, p["y"], self.n, self.B,
                                    C.byref(self.cost) if self.cost is not None else None, eng._integ(self.integ), 0.02, C.byref(o),
                                    p.get("nis"), p.get("innov"), p["status"], C.byref(lg) if lg else None, p["ws"], eng._stream())
        fp.check_rc(eng, rc)

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        log = None if "log" in self.drop else dict(log_xhat=t["log_xhat"], log_dhat=t["log_dhat"], log_nis=t["log_nis"], step=1)
        r = eng.dekf_step(t["xhat"], t["dhat"], t["Pz"], t["u"], self.H * self.m, t["y"], self.cost, self.integ, 0.02,
                          self.ekf.options(self.n, self.m), nis="nis" not in self.drop, innov="innov" not in self.drop, log=log)
        t.update({k: v for k, v in r.items() if v is not None and k != "P"})
        return {b.name: t[b.name] for b in self.outputs() if b.role != fp.WS}


class CompensateOp(fp.Op):
    """phnn_dist_compensate on the first control of an (B,H,m) sequence."""
    H = 3

    def __init__(self, m, B, rng, bounded=True, drop=()):
        from phnn_mpc_amd import _capi
        super().__init__()
        self.name, self.m, self.B, self.drop = f"dist_compensate m{m} B{B} drop={','.join(drop) or '-'}", m, B, set(drop)
        self.cost = _capi.make_cost(4, m, np.ones(4), 0.01, None, -1.5, 2.0) if bounded else None
        v, d = compensate_case(rng, B, m, self.H)
        self.add("v", np.float32, (B, self.H, m), fp.IN, v)
        self.add("dhat", np.float32, (B, m), fp.IN, d)
        self.add("u_cmd", np.float32, (B, m), fp.OUT)
        if "status" not in self.drop:
            self.add("status", np.int32, (B,), fp.OUT)

    def call(self, eng, p):
        fp.check_rc(eng, eng.lib.phnn_dist_compensate(eng.h, p["v"], self.H * self.m, p["dhat"], self.B,
                                                      C.byref(self.cost) if self.cost is not None else None, p["u_cmd"],
                                                      p.get("status"), eng._stream()))

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        u, s = eng.dist_compensate(t["v"], self.H * self.m, t["dhat"], self.cost, status="status" not in self.drop or None)
        t.update(u_cmd=u, **({} if s is None else {"status": s}))
        return {b.name: t[b.name] for b in self.outputs()}


@pytest.mark.parametrize("n,m", dm.NM)
def test_footprint_of_the_update(torch, n, m):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = engine_nm(n, m)
    rep = Report(f"phnn_dekf_update n{n} m{m}")
    for B in (17, 65):
        for name, drop in (("all", ()), ("single", ("nis", "innov", "log")), ("empty", ("log",))):
            op = DekfUpdateOp(n, m, B, em.MASKS[n][name], rng_of("dekf_update", n, m, B, name), drop)
            ff = footprint(rep, torch, eng, op)
            if not drop:  # the call wrote row 2 of both float32 logs and row 1 of the nis log, nothing else of them
                for k, row, width in (("log_xhat", 2, 4 * n * B), ("log_dhat", 2, 4 * m * B), ("log_nis", 1, 8 * B)):
                    got = ff[2].written(k, 0)
                    assert got is not None and row * width <= got[0] and got[1] <= (row + 1) * width, (k, got)
    rep.finish()


@pytest.mark.parametrize("model,integ", [("phnn_cartpole", "euler"), (vc.NM_SPEC[(4, 2)], "rk4"), ("odefunc_pendulum", "rk4")])
def test_footprint_of_the_step(torch, model, integ):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = step_engine(model)
    rep = Report(f"phnn_dekf_step {model} {integ}")
    for B in (17, 65):
        for bounded, drop in ((True, ()), (False, ("nis", "innov", "log"))):
            footprint(rep, torch, eng, DekfStepOp(eng, B, STEP_MODELS[model], integ, rng_of("dekf_step", model, B, bounded), bounded, drop))
    rep.finish()


@pytest.mark.parametrize("m", [1, 2])
def test_footprint_of_the_compensation(torch, m):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = engine_nm(4, m)
    rep = Report(f"phnn_dist_compensate m{m}")
    for B in (17, 65):
        for bounded, drop in ((True, ()), (False, ("status",))):
            footprint(rep, torch, eng, CompensateOp(m, B, rng_of("dist_compensate", m, B, bounded), bounded, drop))
    rep.finish()


# ----------------------------------------------------------------------------- 6. refusals
def test_bad_arguments_are_refused_and_nothing_is_written(torch):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    eng = engine("phnn_cartpole")
    n, m, B = 4, 1, 5
    p = dm.seeded_problem(3, B, n, m, 0b0011)
    t = tensors(torch, p)
    cost = _capi.make_cost(4, 1, np.ones(4), 0.01, None, -1.0, 1.0)
    upside = _capi.make_cost(4, 1, np.ones(4), 0.01, None, 1.0, -1.0)

    def fresh():
        return dict(Pz=dev(torch, p["Pz"]), dhat=dev(torch, p["dhat"]), xhat=torch.full((B, n), 7.0, device="cuda:0"),
                    status=torch.full((B,), 7, dtype=torch.int32, device="cuda:0"),
                    nis=torch.full((B,), 7.0, dtype=torch.float64, device="cuda:0"))

    def untouched(o):
        assert np.array_equal(npy(o["Pz"]), p["Pz"]) and np.array_equal(npy(o["dhat"]), p["dhat"]) and np.all(npy(o["xhat"]) == 7)
        assert np.all(npy(o["status"]) == 7) and np.all(npy(o["nis"]) == 7)

    def update(o, opt, **kw):
        return eng.dekf_update(t["xpred"], t["A"], t["Bm"], t["y"], o["Pz"], o["dhat"], opt, xhat=o["xhat"], nis=o["nis"],
                               status=o["status"], **kw)

    def step(o, opt, c=cost, integ="euler", dt=0.02, **kw):
        return eng.dekf_step(o["xhat"], o["dhat"], o["Pz"], t["xpred"][:, :m].contiguous(), m, t["y"], c, integ, dt, opt,
                             nis=o["nis"], status=o["status"], **kw)

    def bad_options():
        for what, edit in (("mask", lambda o: setattr(o, "meas_mask", 0b10011)), ("Qz nan", lambda o: o.Qz.__setitem__(5, float("nan"))),
                           ("Qz inf", lambda o: o.Qz.__setitem__(24, float("inf"))), ("Rn 0", lambda o: o.Rn.__setitem__(0, 0.0)),
                           ("Rn < 0", lambda o: o.Rn.__setitem__(1, -1.0)), ("Rn nan", lambda o: o.Rn.__setitem__(1, float("nan"))),
                           ("Rn inf", lambda o: o.Rn.__setitem__(0, float("inf"))), ("reserved", lambda o: o.reserved.__setitem__(2, 1))):
            o = dm.dekf_options(p)
            edit(o)
            yield what, o

    # the complete text each edit leaves in phnn_last_error, for the update and for the step alike
    text = {"mask": "meas_mask has bits at or above n", "Qz": "Qz is not finite",
            "Rn": "Rn of a measured component is not positive and finite", "reserved": "reserved must be zero"}
    good = dm.dekf_options(p)
    good.Rn[3] = float("nan")  # not measured: not looked at
    good.Qz[25] = float("nan")  # past the (5,5) entries: not looked at
    o = fresh()
    update(o, good)
    assert not npy(o["status"]).any()
    nolog = dict(log_dhat=torch.zeros(2, B, m, device="cuda:0"), step=-1)
    for what, opt in bad_options():
        o = fresh()
        with pytest.raises(PhnnError, match="error -") as upd:
            update(o, opt)
        with pytest.raises(PhnnError, match="error -") as stp:
            step(o, opt)
        untouched(o)
        assert str(upd.value) == str(stp.value) == "phnn_mpc error -1: phnn_dekf_options: " + text[what.split()[0]], what
    o = fresh()
    with pytest.raises(PhnnError, match="step source"):
        update(o, good, log=nolog)
    with pytest.raises(PhnnError, match="step source"):
        step(o, good, log=nolog)
    with pytest.raises(ValueError, match="Unknown integrator"):
        step(o, good, integ=7)
    with pytest.raises(PhnnError, match="dt"):
        step(o, good, dt=float("nan"))
    with pytest.raises(PhnnError, match="u_min > u_max"):
        step(o, good, c=upside)
    ucmd = torch.full((B, m), 7.0, device="cuda:0")
    with pytest.raises(PhnnError, match="u_min > u_max"):
        eng.dist_compensate(t["xpred"], n, o["dhat"], upside, u_cmd=ucmd)
    untouched(o)
    assert np.all(npy(nolog["log_dhat"]) == 0) and np.all(npy(ucmd) == 7)
    # NULL required buffers, B < 0, B == 0 through the C-ABI
    lib, st = eng.lib, eng._stream()
    a = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    upd = lambda *args: lib.phnn_dekf_update(eng.h, *args, st)  # noqa: E731
    assert upd(a(t["xpred"]), n, a(t["A"]), None, a(t["y"]), n, B, C.byref(good), a(o["Pz"]), a(o["xhat"]), a(o["dhat"]), None, None,
               a(o["status"]), None) == -1
    assert upd(a(t["xpred"]), n, a(t["A"]), a(t["Bm"]), a(t["y"]), n, B, C.byref(good), a(o["Pz"]), a(o["xhat"]), None, None, None,
               a(o["status"]), None) == -1
    assert upd(a(t["xpred"]), n, a(t["A"]), a(t["Bm"]), a(t["y"]), n, -1, C.byref(good), a(o["Pz"]), a(o["xhat"]), a(o["dhat"]), None,
               None, a(o["status"]), None) == -1
    assert upd(None, n, None, None, None, n, 0, C.byref(good), None, None, None, None, None, None, None) == 0
    assert lib.phnn_dekf_step(eng.h, a(o["xhat"]), a(o["dhat"]), a(o["Pz"]), a(t["xpred"]), n, a(t["y"]), n, B, None, 0, 0.02,
                              C.byref(good), None, None, a(o["status"]), None, None, st) == -1  # no workspace
    assert lib.phnn_dekf_step(eng.h, None, None, None, None, n, None, n, 0, None, 0, 0.02, C.byref(good), None, None, None, None, None,
                              st) == 0
    assert lib.phnn_dist_compensate(eng.h, a(t["xpred"]), n, None, B, None, a(ucmd), None, st) == -1
    assert lib.phnn_dist_compensate(eng.h, a(t["xpred"]), n, a(o["dhat"]), -1, None, a(ucmd), None, st) == -1
    assert lib.phnn_dist_compensate(eng.h, None, n, None, 0, None, None, None, st) == 0
    assert eng.dekf_workspace_bytes(-1) == 0 and eng.dekf_workspace_bytes(0) > 0 and eng.dekf_workspace_bytes(65) >= eng.dekf_workspace_bytes(17)
    torch.cuda.synchronize()
    untouched(o)
    assert np.all(npy(ucmd) == 7)


@pytest.mark.parametrize("m", [3, 4])
def test_an_input_dimension_without_a_kernel_is_unsupported(torch, m):
    from phnn_mpc_amd.estimation import DisturbanceEKF
    eng = engine_nm(4, m)
    assert eng.dekf_workspace_bytes(17) == 0
    B, n, nz = 5, 4, 4 + m
    o = DisturbanceEKF(measured=(0, 1)).options(4, 2)  # any valid options: the (n, m) of the handle is what is refused
    z = lambda *s, dt=None: torch.full(s, 7.0, dtype=dt or torch.float32, device="cuda:0")  # noqa: E731
    Pz, xhat, dhat, status = z(B, nz, nz, dt=torch.float64), z(B, n), z(B, m), torch.full((B,), 7, dtype=torch.int32, device="cuda:0")
    a = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    lib, st = eng.lib, eng._stream()
    UNSUPPORTED = -2
    assert lib.phnn_dekf_update(eng.h, a(xhat), n, a(z(B, n, n)), a(z(B, n, m)), a(xhat), n, B, C.byref(o), a(Pz), a(xhat), a(dhat),
                                None, None, a(status), None, st) == UNSUPPORTED
    assert lib.phnn_dekf_step(eng.h, a(xhat), a(dhat), a(Pz), a(dhat), m, a(xhat), n, B, None, 0, 0.02, C.byref(o), None, None,
                              a(status), None, a(z(4096)), st) == UNSUPPORTED
    torch.cuda.synchronize()
    assert all(np.all(npy(x) == 7) for x in (Pz, xhat, dhat, status))


# ----------------------------------------------------------------------------- 7. the closed loop
class BiasedDevicePlant(DevicePlant):
    """test_gpu_ekf.DevicePlant with the scenario's per-plant force bias, as DeviceClosedLoop hands it to the plant."""

    def __init__(self, torch, eng, scenario, nb, dt=0.02):
        super().__init__(torch, eng, scenario, dt)
        self.bias = torch.tensor(scenario.bias_array(nb), dtype=torch.float32, device=eng.device)
        self.ex.force_bias_dev = self.bias.data_ptr()


@pytest.mark.parametrize("which", ["Adam", "GaussNewton"])
@pytest.mark.parametrize("compensate", [True, False])
def test_closed_loop_with_a_disturbance_estimator(torch, which, compensate):
    from phnn_mpc_amd.closed_loop import PlantScenario, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.estimation import DisturbanceEKF
    c = _controller(torch, which)
    nb, steps = 8, 5
    rng = np.random.default_rng(20)
    X0 = rng.uniform(-1, 1, size=(nb, 4)) * [0.2, 0.08, 0.1, 0.1]
    sc = PlantScenario(force_bias=np.linspace(-2.0, 2.0, nb), meas_sigma=[0.01, 0.005, 0.05, 0.05], seed=0xE57)
    ekf = DisturbanceEKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4, Pd0=4.0, compensate=compensate)
    eager, graphed = (run_mpc_batch_device(c, X0, steps, use_graph=g, scenario=sc, estimator=ekf) for g in (False, True))
    assert set(eager) == {"states", "controls", "done_step", "disturbance", "estimates", "disturbances", "nis", "ekf_status"}
    assert eager["disturbances"].shape == (steps + 1, nb, 1) and eager["disturbances"].dtype == np.float32
    assert eager["estimates"].shape == (steps + 1, nb, 4) and eager["nis"].shape == (steps, nb)
    for k in ("states", "controls", "estimates", "disturbances", "nis", "ekf_status", "done_step"):
        assert dm.same_floats(eager[k], graphed[k]), k
    # positions measured: dhat moves once the disturbance has reached them, from the second step at the latest
    assert not eager["disturbances"][0].any() and eager["disturbances"][2:].all() and np.all(eager["nis"] > 0) and not eager["ekf_status"].any()
    host = run_mpc_batch(BiasedDevicePlant(torch, c.engine, sc, nb), c, X0, steps, estimator=ekf)
    for k in ("controls", "estimates", "disturbances", "states", "nis"):
        assert np.array_equal(np.asarray(eager[k], np.float64), np.asarray(host[k], np.float64)), k
    # the applied control: the plain loop's on the same estimates without compensation, dhat taken off it with
    plain = run_mpc_batch_device(c, X0, 1, use_graph=False, scenario=sc)
    assert np.array_equal(plain["controls"][0], eager["controls"][0])  # dhat = 0 at the first step
    if compensate:
        off = run_mpc_batch_device(c, X0, steps, scenario=sc, estimator=DisturbanceEKF(
            measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4, Pd0=4.0, compensate=False))
        assert np.array_equal(off["controls"][0], eager["controls"][0]) and not np.array_equal(off["controls"][1:], eager["controls"][1:])


def test_closed_loop_with_tracking_compensates_the_tracking_law(torch):
    """track= with a compensating DisturbanceEKF: v is the tracking law's output, the plant and the filter read u_cmd;
    both captured graphs (solve step, tracking step) == eager == run_mpc_batch on the same engine."""
    from phnn_mpc_amd.closed_loop import PlantScenario, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.estimation import DisturbanceEKF
    from phnn_mpc_amd.feedback import Tracking
    c = _controller(torch, "Adam")
    nb, steps = 8, 5
    rng = np.random.default_rng(21)
    X0 = rng.uniform(-1, 1, size=(nb, 4)) * [0.2, 0.08, 0.1, 0.1]
    sc = PlantScenario(force_bias=np.linspace(-2.0, 2.0, nb), meas_sigma=[0.01, 0.005, 0.05, 0.05], seed=0xE57)
    ekf = DisturbanceEKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4, Pd0=4.0)
    tr = Tracking(2)
    eager, graphed = (run_mpc_batch_device(c, X0, steps, use_graph=g, scenario=sc, estimator=ekf, track=tr) for g in (False, True))
    for k in ("states", "controls", "estimates", "disturbances", "nis", "ekf_status", "track_status", "track_dev"):
        assert dm.same_floats(eager[k], graphed[k]), k
    host = run_mpc_batch(BiasedDevicePlant(torch, c.engine, sc, nb), c, X0, steps, estimator=ekf, track=tr)
    for k in ("controls", "estimates", "disturbances", "states", "nis"):
        assert np.array_equal(np.asarray(eager[k], np.float64), np.asarray(host[k], np.float64)), k
    assert eager["disturbances"][2:].all() and not eager["ekf_status"].any()
