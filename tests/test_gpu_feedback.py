"""Tracking the plan between solves on the device.

  1 k_feedback_control   bits == feedback_model.control for every reachable (n, m) (variant_census.NM_PAIRS), B in {1, 17, 65}
                         (one thread, a partial workgroup, a workgroup plus one), H in {1, 2, 7}, the first and the last row
                         of the plan, the step from the host and from a device counter, with and without bounds, the
                         status 1 and 2 cases and a NaN control mixed into the batch, optional outputs NULL and given, log
                         rows at the step index
  2 phnn_feedback_plan   bits == the three public calls made by hand (feedback.Tracking.plan)
  3 footprint            both entry points in guarded buffers (tests/footprint.py)
  4 refusals             PHNN_ERR_INVALID_ARG with no output touched
  5 graph                both calls captured and replayed against the eager run
  6 closed loop          DeviceClosedLoop(track=): solve_every = 1 == the loop without tracking; solve_every = 3 graphed ==
                         eager == run_mpc_batch(track=) on the same engine
"""
import ctypes as C
import os

import numpy as np
import pytest
import yaml

import feedback_model as fm
import footprint as fp
import oracle_lib as ol
import variant_census as vc
from test_gpu_footprint import Report, footprint, rng_of
from test_gpu_footprint import engine as census_engine
from test_gpu_mppi import engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")

# (n, m) -> a census spec with those dimensions (k_feedback_control reads n and m from the handle, nothing else): every
# pair a handle can have
MODEL_OF = vc.NM_SPEC
BOUNDS = (-0.25, 0.4)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def npy(t):
    return t.detach().cpu().numpy()


def dev(torch, a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda:0")


def bounds_cost(n, m, bounds):
    from phnn_mpc_amd import _capi
    if bounds is None:
        return None
    return _capi.make_cost(n, m, np.ones(n), np.ones(m) if m > 1 else 1.0, None, bounds[0], bounds[1])


def control_case(seed, B, H, n, m, j):
    """A seeded plan with the state off its row j, and (where the batch is large enough) the special cases mixed in ->
    (x, u, traj, K, {case: problem})."""
    p = fm.lq_plan(seed, B, H, n, m)
    rng = np.random.default_rng(seed)
    x = (p["traj"][:, j] + 0.1 * rng.normal(size=(B, n))).astype(np.float32)
    u, traj, K = p["u"].copy(), p["traj"].copy(), p["K"].copy()
    where = {}
    if B >= 17:
        slots = [int(b) for b in rng.permutation(B)]
        where = {k: slots.pop() for k in ("nan_K", "inf_K", "nan_x", "nan_traj", "nan_u", "on_plan", "inf_x")}
        K[where["nan_K"], j, m - 1, 0] = np.nan
        K[where["inf_K"], j, 0, n - 1] = -np.inf
        x[where["nan_x"], n - 1] = np.nan
        x[where["inf_x"], 0] = np.inf
        traj[where["nan_traj"], j, 0] = np.nan
        u[where["nan_u"], j, 0] = np.nan
        x[where["on_plan"]] = traj[where["on_plan"], j]
        u[where["on_plan"], j, 0] = -0.0
    return x, u, traj, K, where


# ----------------------------------------------------------------------------- 1. the kernel against the model
@pytest.mark.parametrize("n,m", list(MODEL_OF))
def test_control_equals_the_model_bit_for_bit(torch, n, m):
    eng = census_engine(MODEL_OF[(n, m)])
    assert (eng.n, eng.m) == (n, m)
    seen = set()
    for B in (1, 17, 65):
        for H in (1, 2, 7):
            for j in sorted({0, H - 1}):
                x, u, traj, K, where = control_case(1000 * n + 100 * m + 10 * H + j + B, B, H, n, m, j)
                t = [dev(torch, a) for a in (x, u, traj, K)]
                for bounds in (None, BOUNDS):
                    ref = fm.control(x, u, traj, K, j, bounds)
                    seen |= set(ref["status"].tolist())
                    if where:
                        assert [int(ref["status"][where[k]]) for k in ("nan_K", "inf_K", "nan_x", "inf_x", "nan_traj", "nan_u", "on_plan")] == [1, 1, 2, 2, 2, 0, 0]
                        assert np.isnan(ref["u"][where["nan_u"], 0]) and (ref["status"] == 0).sum() >= B - 5
                        assert ref["u"][where["on_plan"], 0].view(np.uint32) == 0x80000000
                    cost = bounds_cost(n, m, bounds)
                    step = H + j  # solve_every = H: row j, the log row is the step itself
                    T = 2 * H
                    for src in ("host", "dev"):
                        kw = dict(step=step) if src == "host" else dict(step_dev=torch.tensor([step], dtype=torch.int32, device="cuda:0"))
                        r = eng.feedback_control(*t, cost, H, **kw)
                        for k in ("u", "status", "dev"):
                            assert fm.same_floats(npy(r[k]), ref[k]), (B, H, j, bounds, src, k)
                        ok = ~np.isnan(ref["u"])  # the signs, of zeros too
                        assert np.array_equal(npy(r["u"]).view(np.uint32)[ok] >> 31, ref["u"].view(np.uint32)[ok] >> 31)
                        # the optional outputs left NULL, the log rows given: row `step` and no other
                        ls = torch.full((T, B), 7, dtype=torch.int32, device="cuda:0")
                        ld = torch.full((T, B), 7.0, dtype=torch.float64, device="cuda:0")
                        r2 = eng.feedback_control(*t, cost, H, status=False, dev=False, log_status=ls, log_dev=ld, **kw)
                        assert r2["status"] is None and r2["dev"] is None and fm.same_floats(npy(r2["u"]), ref["u"])
                        ls, ld = npy(ls), npy(ld)
                        assert np.array_equal(ls[step], ref["status"]) and fm.same_floats(ld[step], ref["dev"])
                        assert np.all(np.delete(ls, step, axis=0) == 7) and np.all(np.delete(ld, step, axis=0) == 7.0)
    assert seen == {0, 1, 2}


# ----------------------------------------------------------------------------- 2. the plan against the three calls by hand
@pytest.mark.parametrize("model", ["phnn_cartpole", "canonical_cartpole", "odefunc_pendulum"])
@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_plan_equals_the_three_calls_by_hand(torch, model, integ):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.feedback import Tracking
    eng = engine(model)
    n, m, H = eng.n, eng.m, 6
    costs = {"R > 0": _capi.make_cost(n, m, np.linspace(1.0, 3.0, n), np.full(m, 0.01) if m > 1 else 0.01, None, -1.5, 2.0),
             "R = 0": _capi.make_cost(n, m, np.ones(n), np.zeros(m) if m > 1 else 0.0, None, -1.5, 2.0)}
    for B in (1, 17):
        rng = np.random.default_rng(70 + B)
        x0 = (0.3 * rng.normal(size=(B, n))).astype(np.float32)
        u = rng.uniform(-4.0, 4.0, size=(B, H, m)).astype(np.float32)  # some of them outside the bounds
        if B > 1:
            assert (u < -1.5).any() and (u > 2.0).any()
            x0[3, 0] = np.nan  # its trajectory and its Jacobians are NaN: the recursion fails at its first pivots
        for name, cost in costs.items():
            for mu in (0.0, 1e-3):
                xd, ud = dev(torch, x0), dev(torch, u)
                hand = Tracking(2, mu=mu).plan(eng, xd, ud, cost, integ, 0.02)
                _, traj = eng.rollout_cost(xd, ud, cost, integ, 0.02, want_traj=True)
                A, Bm, _ = eng.rollout_linearize(xd, ud, cost, integ, 0.02, traj=traj)
                lq = eng.tvlqr(A, Bm, cost, mu=mu)
                got = eng.feedback_plan(xd, ud, cost, integ, 0.02, mu=mu)
                for k, ref in (("traj", traj), ("K", lq["K"]), ("status", lq["status"])):
                    assert fm.same_floats(npy(got[k]), npy(ref)) and fm.same_floats(npy(hand[k]), npy(ref)), (B, name, mu, k)
                assert np.array_equal(npy(xd), x0, equal_nan=True) and np.array_equal(npy(ud), u), "the inputs are not written"
                status = npy(got["status"])
                if B > 1:
                    # at the last step, or one further down where that step's control is clamped (its column of B is an
                    # exact zero, so the NaN arrives through P)
                    assert status[3] in (H - 1, H) and np.isnan(npy(got["K"])[3, :status[3]]).all()
                    if name == "R > 0":
                        assert not np.delete(status, 3).any() and np.isfinite(np.delete(npy(got["K"]), 3, axis=0)).all()
                elif name == "R > 0":
                    assert not status.any()


# ----------------------------------------------------------------------------- 3. footprint
class FeedbackControlOp(fp.Op):
    """phnn_feedback_control at step 4 of 6 with solve_every = 3 (row 1 of the plan); drop: optional outputs left NULL."""
    H, K_EVERY, STEP, T = 4, 3, 4, 6

    def __init__(self, n, m, B, rng, bounded=True, drop=()):
        super().__init__()
        self.name, self.n, self.m, self.B, self.drop = f"feedback_control n{n} m{m} B{B} drop={','.join(drop) or '-'}", n, m, B, set(drop)
        x, u, traj, K, _ = control_case(int(rng.integers(1 << 30)), B, self.H, n, m, self.STEP % self.K_EVERY)
        self.cost = bounds_cost(n, m, BOUNDS if bounded else None)
        f32, f64 = np.float32, np.float64
        self.add("x", f32, (B, n), fp.IN, x)
        self.add("u", f32, (B, self.H, m), fp.IN, u)
        self.add("traj", f32, (B, self.H + 1, n), fp.IN, traj)
        self.add("K", f64, (B, self.H, m, n), fp.IN, K)
        self.add("u_out", f32, (B, m), fp.OUT)
        if "status" not in self.drop:
            self.add("status", np.int32, (B,), fp.OUT)
        if "dev" not in self.drop:
            self.add("dev", f64, (B,), fp.OUT)
        if "log" not in self.drop:
            self.add("log_status", np.int32, (self.T, B), fp.INOUT, np.zeros((self.T, B), np.int32))
            self.add("log_dev", f64, (self.T, B), fp.INOUT, np.zeros((self.T, B)))

    def call(self, eng, p):
        rc = eng.lib.phnn_feedback_control(eng.h, p["x"], p["u"], p["traj"], p["K"], self.B, self.H,
                                           C.byref(self.cost) if self.cost is not None else None, self.K_EVERY, None, self.STEP,
                                           p["u_out"], p.get("status"), p.get("dev"), p.get("log_status"), p.get("log_dev"),
                                           eng._stream())
        fp.check_rc(eng, rc)

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        r = eng.feedback_control(t["x"], t["u"], t["traj"], t["K"], self.cost, self.K_EVERY, step=self.STEP,
                                 status="status" not in self.drop, dev="dev" not in self.drop, log_status=t.get("log_status"),
                                 log_dev=t.get("log_dev"))
        t.update(u_out=r["u"], **{k: r[k] for k in ("status", "dev") if r[k] is not None})
        return {b.name: t[b.name] for b in self.outputs()}


class FeedbackPlanOp(fp.Op):
    """phnn_feedback_plan with a workspace of exactly the reported size."""
    H = 5

    def __init__(self, eng, B, integ, rng):
        from phnn_mpc_amd import _capi
        super().__init__()
        n, m = eng.n, eng.m
        self.name, self.n, self.m, self.B, self.integ = f"feedback_plan B{B} {integ}", n, m, B, integ
        self.cost = _capi.make_cost(n, m, np.linspace(1.0, 3.0, n), np.full(m, 0.01) if m > 1 else 0.01, None, -1.5, 2.0)
        self.nbytes = eng.feedback_workspace_bytes(B, self.H)
        assert self.nbytes > 0
        f32 = np.float32
        self.add("x0", f32, (B, n), fp.IN, (0.3 * rng.normal(size=(B, n))).astype(f32))
        self.add("u", f32, (B, self.H, m), fp.IN, rng.uniform(-4, 4, size=(B, self.H, m)).astype(f32))
        self.add("traj", f32, (B, self.H + 1, n), fp.OUT)
        self.add("K", np.float64, (B, self.H, m, n), fp.OUT)
        self.add("status", np.int32, (B,), fp.OUT)
        self.add("ws", np.uint8, (self.nbytes,), fp.WS)

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        opt = _capi.TvlqrOptions()
        opt.mu = 1e-6
        rc = eng.lib.phnn_feedback_plan(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), eng._integ(self.integ), 0.02,
                                        C.byref(opt), p["ws"], self.nbytes, p["traj"], p["K"], p["status"], eng._stream())
        fp.check_rc(eng, rc)

    def engine(self, eng):
        import torch
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        r = eng.feedback_plan(t["x0"], t["u"], self.cost, self.integ, 0.02, mu=1e-6)
        return {k: r[k] for k in ("traj", "K", "status")}


@pytest.mark.parametrize("n,m", [(2, 1), (3, 1), (4, 1), (4, 4)])
def test_footprint_of_the_control(torch, n, m):
    eng = census_engine(MODEL_OF[(n, m)])
    rep = Report(f"phnn_feedback_control n{n} m{m}")
    for B in (17, 65):
        for bounded, drop in ((True, ()), (False, ("status", "dev", "log")), (True, ("log",))):
            op = FeedbackControlOp(n, m, B, rng_of("feedback_control", n, m, B, bounded), bounded, drop)
            ff = footprint(rep, torch, eng, op)
            if not drop:  # the call wrote row 4 of both logs, nothing else of them
                for k, width in (("log_status", 4 * B), ("log_dev", 8 * B)):
                    got = ff[2].written(k, 0)
                    assert got is not None and op.STEP * width <= got[0] and got[1] <= (op.STEP + 1) * width, (k, got)
    rep.finish()


@pytest.mark.parametrize("model,integ", [("phnn_cartpole", "euler"), ("canonical_cartpole", "rk4"), ("odefunc_pendulum", "rk4")])
def test_footprint_of_the_plan(torch, model, integ):
    eng = engine(model)
    rep = Report(f"phnn_feedback_plan {model} {integ}")
    for B in (17, 65):
        footprint(rep, torch, eng, FeedbackPlanOp(eng, B, integ, rng_of("feedback_plan", model, B)))
    rep.finish()
    # the size query: zero for what it refuses, non-decreasing in B and H
    wb = eng.feedback_workspace_bytes
    assert wb(-1, 5) == 0 and wb(5, 0) == 0 and wb(0, 1) > 0
    sizes = [[wb(B, H) for H in (1, 2, 7, 20)] for B in (1, 17, 65, 4096)]
    assert all(r == sorted(r) for r in sizes) and all(list(c) == sorted(c) for c in zip(*sizes))
    n, m = eng.n, eng.m
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    assert wb(65, 7) == up(65 * 7 * n * n * 4) + up(65 * 7 * n * m * 4) + up(65 * 4) + up(65 * n * n * 8)


# ----------------------------------------------------------------------------- 4. refusals
def test_bad_arguments_are_refused_and_nothing_is_written(torch):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    eng = engine("phnn_cartpole")
    n, m, B, H = 4, 1, 5, 4
    x, u, traj, K, _ = control_case(5, B, H, n, m, 1)
    t = [dev(torch, a) for a in (x, u, traj, K)]
    cost = bounds_cost(n, m, BOUNDS)
    upside = bounds_cost(n, m, (1.0, -1.0))

    def fresh():
        return dict(u_out=torch.full((B, m), 7.0, device="cuda:0"), status=torch.full((B,), 7, dtype=torch.int32, device="cuda:0"),
                    dev=torch.full((B,), 7.0, dtype=torch.float64, device="cuda:0"),
                    log_status=torch.full((3, B), 7, dtype=torch.int32, device="cuda:0"),
                    log_dev=torch.full((3, B), 7.0, dtype=torch.float64, device="cuda:0"))

    def untouched(o):
        for k, v in o.items():
            assert np.all(npy(v) == 7), k

    o = fresh()
    for what, kw in (("solve_every", dict(cost=cost, solve_every=0)), ("solve_every", dict(cost=cost, solve_every=H + 1)),
                     ("step source", dict(cost=cost, solve_every=2, step=-1)), ("u_min > u_max", dict(cost=upside, solve_every=2))):
        kw.setdefault("step", 1)
        with pytest.raises(PhnnError, match=what):
            eng.feedback_control(*t, kw.pop("cost"), kw.pop("solve_every"), **kw, **o)
    untouched(o)
    lib, st = eng.lib, eng._stream()
    a = lambda v: C.c_void_p(v.data_ptr())  # noqa: E731
    tail = lambda: (a(o["status"]), a(o["dev"]), a(o["log_status"]), a(o["log_dev"]), st)  # noqa: E731
    for missing in range(5):  # each required buffer NULL in turn
        ptrs = [a(v) for v in t] + [a(o["u_out"])]
        ptrs[missing] = None
        assert lib.phnn_feedback_control(eng.h, *ptrs[:4], B, H, C.byref(cost), 2, None, 1, ptrs[4], *tail()) == -1
    assert lib.phnn_feedback_control(eng.h, *[a(v) for v in t], -1, H, C.byref(cost), 2, None, 1, a(o["u_out"]), *tail()) == -1
    assert lib.phnn_feedback_control(eng.h, *[a(v) for v in t], B, 0, C.byref(cost), 1, None, 1, a(o["u_out"]), *tail()) == -1
    assert lib.phnn_feedback_control(eng.h, None, None, None, None, 0, H, None, 2, None, 1, None, None, None, None, None, st) == 0
    torch.cuda.synchronize()
    untouched(o)
    # the plan
    xd, ud = t[0], t[1]
    ws = torch.empty(eng.feedback_workspace_bytes(B, H), dtype=torch.uint8, device="cuda:0")
    out = dict(traj=torch.full((B, H + 1, n), 7.0, device="cuda:0"), K=torch.full((B, H, m, n), 7.0, dtype=torch.float64, device="cuda:0"),
               status=torch.full((B,), 7, dtype=torch.int32, device="cuda:0"))
    full = _capi.make_cost(n, m, np.ones(n), 0.01, None, -1.0, 1.0)
    flipped = _capi.make_cost(n, m, np.ones(n), 0.01, None, 1.0, -1.0)
    with pytest.raises(PhnnError, match="u_min > u_max"):
        eng.feedback_plan(xd, ud, flipped, "euler", 0.02, **out)
    with pytest.raises(PhnnError, match="mu"):
        eng.feedback_plan(xd, ud, full, "euler", 0.02, mu=-1.0, **out)
    with pytest.raises(PhnnError, match="dt"):
        eng.feedback_plan(xd, ud, full, "euler", float("inf"), **out)
    with pytest.raises(ValueError, match="Unknown integrator"):
        eng.feedback_plan(xd, ud, full, "heun", 0.02, **out)
    opt = _capi.TvlqrOptions()

    def plan(x0=a(xd), uu=a(ud), nb=B, hh=H, c=C.byref(full), integ=0, o_=C.byref(opt), w=a(ws), size=ws.numel(), tr=a(out["traj"]),
             kk=a(out["K"]), s=a(out["status"])):
        return lib.phnn_feedback_plan(eng.h, x0, uu, nb, hh, c, integ, 0.02, o_, w, size, tr, kk, s, st)

    for kw in (dict(x0=None), dict(uu=None), dict(c=None), dict(w=None), dict(tr=None), dict(kk=None), dict(s=None), dict(nb=-1),
               dict(hh=0), dict(integ=2), dict(size=ws.numel() - 1)):
        assert plan(**kw) == -1, kw
    opt.reserved[1] = 1
    assert plan() == -1
    opt.reserved[1] = 0
    assert plan(x0=None, uu=None, nb=0, w=None, size=0, tr=None, kk=None, s=None) == 0
    torch.cuda.synchronize()
    untouched(out)
    assert plan() == 0 and plan(o_=None) == 0  # and with everything in place it runs; opt NULL = {0}
    torch.cuda.synchronize()
    assert not npy(out["status"]).any() and np.isfinite(npy(out["K"])).all()


# ----------------------------------------------------------------------------- 5. graph replay
def test_graph_replay_equals_the_eager_calls(torch):
    from phnn_mpc_amd import _capi
    eng = engine("phnn_cartpole")
    n, m, B, H, ke = 4, 1, 17, 6, 3
    rng = np.random.default_rng(9)
    cost = _capi.make_cost(n, m, [10.0, 100.0, 1.0, 10.0], 0.01, None, -2.0, 2.0)
    x0 = dev(torch, (0.2 * rng.normal(size=(B, n))).astype(np.float32))
    u = dev(torch, rng.uniform(-3, 3, size=(B, H, m)).astype(np.float32))
    x = dev(torch, (npy(x0) + 0.05 * rng.normal(size=(B, n))).astype(np.float32))
    step = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ws, out = {}, torch.zeros(B, m, device="cuda:0")
    st, dv = torch.zeros(B, dtype=torch.int32, device="cuda:0"), torch.zeros(B, dtype=torch.float64, device="cuda:0")

    def both():
        pl = eng.feedback_plan(x0, u, cost, "euler", 0.02, workspace=ws)
        eng.feedback_control(x, u, pl["traj"], pl["K"], cost, ke, step_dev=step, u_out=out, status=st, dev=dv)
        return pl

    eager = []
    for s in range(4):
        step.fill_(s)
        pl = both()
        eager.append([npy(v).copy() for v in (pl["traj"], pl["K"], pl["status"], out, st, dv)])
    from phnn_mpc_amd.solver import capture
    step.fill_(0)
    graph, pl = capture(eng.device, both)
    for s in range(4):
        for v in (pl["traj"], pl["K"], out, dv):
            v.fill_(7.0)
        step.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip((pl["traj"], pl["K"], pl["status"], out, st, dv), eager[s]):
            assert fm.same_floats(npy(got), ref), s
    assert not np.array_equal(eager[0][3], eager[1][3]), "the counter moves the plan row under the replayed graph"


# ----------------------------------------------------------------------------- 6. the closed loop
class DevicePlant:
    """run_mpc_batch's simulator served by the device plant kernel, so that the host-driven loop sees the states and the
    measurements of the device loop bit for bit (the numpy plant differs by the device's sin / cos)."""

    def __init__(self, torch, eng, scenario, dt=0.02):
        from phnn_mpc_amd import _capi
        self.torch, self.eng, self.plant, self.dt = torch, eng, _capi.Plant.default(dt), dt
        self.ex = _capi.PlantEx()
        self.ex.force_sigma = scenario.force_sigma
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
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import MPCControllerCanonical
    if which == "canonical":
        m = pHNN_Canonical(CFG)
        m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights("canonical_cartpole").items()})
        return MPCControllerCanonical(m.use_device("cuda:0"), horizon=5, dt=0.02, optimizer_steps=3)
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(horizon=5, optimizer_steps=3)
    if which == "GaussNewton":
        cfg["mpc"].update(optimizer="GaussNewton", optimizer_steps=2, gn_line_steps=4)
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights("phnn_cartpole").items()})
    c = create_mpc_from_config(m, cfg)
    assert c.optimizer_type == which
    return c


NB, STEPS = 8, 7


def _x0():
    return np.random.default_rng(20).uniform(-1, 1, size=(NB, 4)) * [0.2, 0.08, 0.1, 0.1]


@pytest.mark.parametrize("which", ["Adam", "GaussNewton", "canonical"])
def test_solve_every_1_is_the_loop_without_tracking(torch, which):
    from phnn_mpc_amd.closed_loop import PlantScenario, run_mpc_batch_device
    from phnn_mpc_amd.feedback import Tracking
    c = _controller(torch, which)
    sc = PlantScenario(force_sigma=0.5, meas_sigma=0.002, seed=0xFB)
    for graph in (False, True):
        plain = run_mpc_batch_device(c, _x0(), STEPS, use_graph=graph, scenario=sc)
        tracked = run_mpc_batch_device(c, _x0(), STEPS, use_graph=graph, scenario=sc, track=Tracking(1))
        assert set(tracked) == set(plain) | {"track_status", "track_dev"}
        for k in ("states", "controls", "done_step", "disturbance"):
            assert np.array_equal(plain[k], tracked[k]), (graph, k)
        assert tracked["track_status"].shape == (STEPS, NB) and not tracked["track_status"].any() and not tracked["track_dev"].any()
    assert run_mpc_batch_device(c, _x0(), 2, track=Tracking(1, log=False))["track_dev"] is None


@pytest.mark.parametrize("which,estimated", [("Adam", False), ("Adam", True), ("canonical", False)])
def test_solve_every_3_graphed_eager_and_host_loops_agree(torch, which, estimated):
    from phnn_mpc_amd.closed_loop import DeviceClosedLoop, PlantScenario, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.estimation import EKF
    from phnn_mpc_amd.feedback import Tracking
    c = _controller(torch, which)
    sc = PlantScenario(force_sigma=0.5, meas_sigma=[0.01, 0.005, 0.05, 0.05] if estimated else 0.0, seed=0xFB)
    kw = dict(estimator=EKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4)) if estimated else {}
    tr = Tracking(3)
    eager, graphed = (run_mpc_batch_device(c, _x0(), STEPS, use_graph=g, scenario=sc, track=tr, **kw) for g in (False, True))
    keys = ("states", "controls", "done_step", "disturbance", "track_status", "track_dev") + (("estimates", "nis") if estimated else ())
    for k in keys:
        assert fm.same_floats(eager[k], graphed[k]), k
    host = run_mpc_batch(DevicePlant(torch, c.engine, sc), c, _x0(), STEPS, track=tr, **kw)
    for k in ("controls", "states", "track_status", "track_dev") + (("estimates", "nis") if estimated else ()):
        assert np.array_equal(np.asarray(eager[k], np.float64), np.asarray(host[k], np.float64)), k
    # every plan held, and the deviation is zero exactly on the solve steps
    assert not eager["track_status"].any()
    assert not eager["track_dev"][0::3].any() and np.all(eager["track_dev"][1::3] > 0) and np.all(eager["track_dev"][2::3] > 0)
    # the solve runs every third step only: the loop without tracking gives other controls from step 1 on
    plain = run_mpc_batch_device(c, _x0(), STEPS, scenario=sc, **kw)
    assert np.array_equal(plain["controls"][0], eager["controls"][0]) and not np.array_equal(plain["controls"][1:], eager["controls"][1:])
    with pytest.raises(ValueError, match="horizon"):
        DeviceClosedLoop(c, _x0(), STEPS, track=Tracking(6))
    with pytest.raises(ValueError, match="differs from the controller's"):
        DeviceClosedLoop(c, _x0(), STEPS, dt=0.01, track=tr)
