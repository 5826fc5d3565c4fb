"""phnn_tvlqr on the GPU, and the properties the three linearisation entry points share:

  1 bitwise      k_tvlqr == tests/tvlqr_model.py bit for bit (NaN at the same positions, the same status) on the CPU
                 tests' seeded inputs, B in {1, 65, 300} x H in {1, 6, 50} x every reachable (n, m) (variant_census.NM_PAIRS), on (A, Bm)
                 downloaded from phnn_rollout_linearize of the headline spec, and on the failure cases; P_all = NULL gives
                 the same K and P0
  2 arguments    one bad argument at a time through the three entry points: PHNN_ERR_INVALID_ARG, outputs untouched,
                 phnn_last_error names the cause
  3 footprint    the three entry points on guarded buffers of exactly the documented sizes (tests/footprint.py)
  4 graph        K1 -> linearise -> tvlqr captured on one stream, replayed twice, against the eager run
  5 controllers  feedback_gains of both controllers == the three engine calls made by hand"""
import ctypes as C
import os

import numpy as np
import pytest

import footprint as fp
import linearize_cases as lc
import oracle_lib as ol
import tvlqr_model as tm
import variant_census as vc
from test_gpu_footprint import Report, engine, footprint, rng_of
from test_tvlqr_model import FAILURES, failure_case

pytestmark = pytest.mark.gpu

# (n, m) -> a census spec with those dimensions (phnn_tvlqr reads n and m from the handle, nothing else): every pair a
# handle can have
MODEL_OF = vc.NM_SPEC
INVALID = -1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def npf(t):
    return t.detach().cpu().numpy()


def cost_of(n, m, Q, R):
    from phnn_mpc_amd import _capi
    return _capi.make_cost(n, m, Q, R)


def check_equal(what, out, ref, want_P=True):
    assert np.array_equal(npf(out["status"]), ref["status"]), (what, npf(out["status"]), ref["status"])
    for k in ("K", "P0") + (("P",) if want_P else ()):
        assert tm.same_floats(npf(out[k]), ref[k]), (what, k)


# ----------------------------------------------------------------------------- 1. bitwise
@pytest.mark.parametrize("H", [1, 6, 50])
@pytest.mark.parametrize("n,m", list(MODEL_OF))
def test_kernel_equals_the_stated_order_model(torch, n, m, H):
    eng = engine(MODEL_OF[(n, m)])
    for B in (1, 65, 300):
        A, Bm, Q, R = tm.seeded_problem(1000 * n + 100 * m + H, B, H, n, m)
        cost = cost_of(n, m, Q, R)
        Lxx, Luu = tm.cost_matrices_of(cost, n, m)
        for mu in (0.0, 0.125):
            ref = tm.tvlqr(A, Bm, Lxx, Luu, mu)
            assert not ref["status"].any()
            out = eng.tvlqr(A, Bm, cost, mu=mu, want_P=True)
            check_equal((n, m, H, B, mu), out, ref)
            lean = eng.tvlqr(A, Bm, cost, mu=mu)  # P_all = NULL
            assert lean["P"] is None
            assert torch.equal(lean["K"], out["K"]) and torch.equal(lean["P0"], out["P0"]) and torch.equal(lean["status"], out["status"])


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_kernel_on_a_linearised_rollout(torch, integ):
    """(A, Bm) downloaded from phnn_rollout_linearize of the headline spec, non-symmetric Q and bounds: some columns of
    Bm are exactly zero."""
    sid = lc.HEADLINE
    s, eng = vc.CENSUS[sid], engine(sid)
    rng = np.random.default_rng(21)
    B, H = 65, 50
    x0 = 0.3 * vc.states(rng, 4, B)
    u = vc.controls(rng, B, H, 1)
    cost = vc.cost_of(s, rng)
    A, Bm, _ = eng.rollout_linearize(x0, u, cost, integ, 0.02)
    assert bool(torch.isfinite(A).all()) and bool((Bm == 0).any())
    ref = tm.tvlqr(npf(A), npf(Bm), *tm.cost_matrices_of(cost, 4, 1))
    out = eng.tvlqr(A, Bm, cost, want_P=True)
    check_equal(integ, out, ref)
    assert not ref["status"].any() and np.isfinite(ref["K"]).all()


@pytest.mark.parametrize("kind,n,m,H,t", FAILURES + [("zero_B_mu", 2, 1, 6, 3), ("zero_B_mu", 4, 3, 6, 0)])
def test_failure_cases(torch, kind, n, m, H, t):
    eng = engine(MODEL_OF[(n, m)])
    A, Bm, Lxx, Luu, mu, status = failure_case(kind, n, m, H, t)
    # the cost whose Q + Q^T, R + R^T are the case's matrices: halves are exact
    cost = cost_of(n, m, (0.5 * Lxx).astype(np.float32), (0.5 * Luu).astype(np.float32))
    assert np.array_equal(tm.cost_matrices_of(cost, n, m)[0], Lxx) and np.array_equal(tm.cost_matrices_of(cost, n, m)[1], Luu)
    ref = tm.tvlqr(A, Bm, Lxx, Luu, mu)
    if kind != "negative_R":
        assert ref["status"][1] == status
    out = eng.tvlqr(A, Bm, cost, mu=mu, want_P=True)
    check_equal((kind, n, m, H, t), out, ref)
    lean = eng.tvlqr(A, Bm, cost, mu=mu)
    check_equal((kind, n, m, H, t, "P_all = NULL"), lean, ref, want_P=False)


# ----------------------------------------------------------------------------- 2. arguments
def _buffers(torch, B, H, n, m):
    f = dict(dtype=torch.float32, device="cuda:0")
    d = dict(dtype=torch.float64, device="cuda:0")
    return dict(x=torch.zeros(B, n, **f), u1=torch.zeros(B, m, **f), u=torch.zeros(B, H, m, **f), traj=torch.zeros(B, H + 1, n, **f),
                A1=torch.full((B, n, n), 7.0, **f), B1=torch.full((B, n, m), 7.0, **f),
                A=torch.full((B, H, n, n), 7.0, **f), Bm=torch.full((B, H, n, m), 7.0, **f),
                K=torch.full((B, H, m, n), 7.0, **d), P0=torch.full((B, n, n), 7.0, **d), P=torch.full((B, H + 1, n, n), 7.0, **d),
                status=torch.full((B,), 7, dtype=torch.int32, device="cuda:0"))


def test_bad_arguments(torch):
    from phnn_mpc_amd import _capi
    sid = lc.HEADLINE
    s, eng = vc.CENSUS[sid], engine(sid)
    lib, h, st = eng.lib, eng.h, eng._stream()
    assert lib.phnn_version() >= 270
    B, H, n, m = 5, 3, 4, 1
    t = _buffers(torch, B, H, n, m)
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    cost = vc.cost_of(s, np.random.default_rng(0))
    bad_cost = vc.cost_of(s, np.random.default_rng(0))
    bad_cost.u_min, bad_cost.u_max = 1.0, -1.0
    cref = C.byref(cost)

    def opt(mu=0.0, reserved=0):
        o = _capi.TvlqrOptions()
        o.mu, o.reserved[2] = mu, reserved
        return C.byref(o)

    def jac(x=p["x"], u=p["u1"], nb=B, A=p["A1"], Bm=p["B1"]):
        return lib.phnn_model_jacobian(h, x, u, nb, A, Bm, st)

    def lin(u=p["u"], nb=B, hh=H, c=cref, integ=0, dt=0.02, traj=p["traj"], A=p["A"], Bm=p["Bm"]):
        return lib.phnn_rollout_linearize(h, u, nb, hh, c, integ, dt, traj, A, Bm, st)

    def lqr(A=p["A"], Bm=p["Bm"], nb=B, hh=H, c=cref, o=None, K=p["K"], P0=p["P0"], P=p["P"], status=p["status"]):
        return lib.phnn_tvlqr(h, A, Bm, nb, hh, c, o, K, P0, P, status, st)

    cases = [
        (lambda: jac(x=None), "NULL"), (lambda: jac(u=None), "NULL"), (lambda: jac(A=None), "NULL"),
        (lambda: jac(Bm=None), "NULL"), (lambda: jac(nb=-1), "negative batch"),
        (lambda: lin(u=None), "NULL"), (lambda: lin(traj=None), "NULL"), (lambda: lin(A=None), "NULL"),
        (lambda: lin(Bm=None), "NULL"), (lambda: lin(nb=-1), "negative batch"), (lambda: lin(hh=0), "horizon < 1"),
        (lambda: lin(integ=2), "integrator"), (lambda: lin(integ=-1), "integrator"),
        (lambda: lin(dt=float("nan")), "dt"), (lambda: lin(dt=float("inf")), "dt"),
        (lambda: lin(c=C.byref(bad_cost)), "u_min > u_max"),
        (lambda: lqr(A=None), "NULL"), (lambda: lqr(Bm=None), "NULL"), (lambda: lqr(K=None), "NULL"),
        (lambda: lqr(P0=None), "NULL"), (lambda: lqr(status=None), "NULL"), (lambda: lqr(c=None), "cost is NULL"),
        (lambda: lqr(nb=-1), "negative batch"), (lambda: lqr(hh=0), "horizon < 1"),
        (lambda: lqr(o=opt(mu=-1e-9)), "mu"), (lambda: lqr(o=opt(mu=float("nan"))), "mu"),
        (lambda: lqr(o=opt(mu=float("inf"))), "mu"), (lambda: lqr(o=opt(reserved=1)), "reserved"),
    ]
    for k, (call, why) in enumerate(cases):
        rc = call()
        msg = lib.phnn_last_error(h).decode()
        assert rc == INVALID, (k, rc, msg)
        assert why in msg, (k, why, msg)
    torch.cuda.synchronize()
    for k in ("A1", "B1", "A", "Bm", "K", "P0", "P", "status"):
        assert bool((t[k] == 7).all()), k  # nothing was launched
    # B == 0: PHNN_OK, nothing launched, NULL buffers allowed
    assert jac(x=None, u=None, nb=0, A=None, Bm=None) == 0
    assert lin(u=None, nb=0, traj=None, A=None, Bm=None) == 0
    assert lqr(A=None, Bm=None, nb=0, K=None, P0=None, P=None, status=None) == 0
    # and the valid calls: options NULL == mu 0, cost NULL == no clamp
    assert jac() == 0 and lin() == 0 and lin(c=None) == 0 and lqr() == 0 and lqr(o=opt()) == 0 and lqr(P=None) == 0
    torch.cuda.synchronize()
    assert not bool((t["A"] == 7).any()) and not bool((t["K"] == 7).any()) and not bool((t["status"] == 7).any())


# ----------------------------------------------------------------------------- 3. footprint
class JacobianOp(fp.Op):
    """phnn_model_jacobian: x (B,n), u (B,m) -> A (B,n,n), Bm (B,n,m)."""

    def __init__(self, x, u):
        super().__init__()
        B, n = x.shape
        m = u.shape[1]
        self.name, self.B = f"jacobian B{B}", B
        f = np.float32
        self.add("x", f, (B, n), fp.IN, x)
        self.add("u", f, (B, m), fp.IN, u)
        self.add("A", f, (B, n, n), fp.OUT)
        self.add("Bm", f, (B, n, m), fp.OUT)

    def call(self, eng, p):
        fp.check_rc(eng, eng.lib.phnn_model_jacobian(eng.h, p["x"], p["u"], self.B, p["A"], p["Bm"], eng._stream()))

    def engine(self, eng):
        A, Bm = eng.jacobian(self.input("x"), self.input("u"))
        return {"A": A, "Bm": Bm}


class GainsOp(fp.Op):
    """K1 -> phnn_rollout_linearize -> phnn_tvlqr on shared buffers (P_all given or NULL).  The float64 outputs and the
    status are accessed by element, so they take the row-slice skew like every other tensor; A and traj are tensors of
    state rows, whose row slices keep their 16-byte alignment."""

    def __init__(self, cost, x0, U, integ, dt, with_P=True):
        super().__init__()
        B, H, m = U.shape
        n = x0.shape[1]
        self.name = f"gains B{B} H{H} m{m} integ{integ} P={int(with_P)}"
        self.cost, self.integ, self.dt, self.B, self.H, self.with_P = cost, integ, dt, B, H, with_P
        f, d = np.float32, np.float64
        self.add("x0", f, (B, n), fp.IN, x0)
        self.add("u", f, (B, H, m), fp.IN, U)
        self.add("cost", f, (B,), fp.OUT)
        self.add("traj", f, (B, H + 1, n), fp.OUT)
        self.add("A", f, (B, H, n, n), fp.OUT)
        self.add("Bm", f, (B, H, n, m), fp.OUT)
        self.add("K", d, (B, H, m, n), fp.OUT)
        self.add("P0", d, (B, n, n), fp.OUT)
        if with_P:
            self.add("P", d, (B, H + 1, n, n), fp.OUT)
        self.add("status", np.int32, (B,), fp.OUT)

    def call(self, eng, p):
        lib, h, st = eng.lib, eng.h, eng._stream()
        B, H, c, integ, dt = self.B, self.H, C.byref(self.cost), self.integ, float(self.dt)
        fp.check_rc(eng, lib.phnn_rollout_fwd(h, p["x0"], p["u"], B, H, c, integ, dt, p["cost"], p["traj"], None, st))
        fp.check_rc(eng, lib.phnn_rollout_linearize(h, p["u"], B, H, c, integ, dt, p["traj"], p["A"], p["Bm"], st))
        fp.check_rc(eng, lib.phnn_tvlqr(h, p["A"], p["Bm"], B, H, c, None, p["K"], p["P0"], p.get("P"), p["status"], st))

    def engine(self, eng):
        A, Bm, traj = eng.rollout_linearize(self.input("x0"), self.input("u"), self.cost, {0: "euler", 1: "rk4"}[self.integ], self.dt)
        r = eng.tvlqr(A, Bm, self.cost, want_P=self.with_P)
        out = {"traj": traj, "A": A, "Bm": Bm, "K": r["K"], "P0": r["P0"], "status": r["status"]}
        if self.with_P:
            out["P"] = r["P"]
        return out


FOOTPRINT_SPECS = [lc.HEADLINE, "phnn<n=2,hid=64,Gnet>", "canonical<m=3,hid=128,f16x2>", "odefunc<n=3,hid=128,f16x2>"]


@pytest.mark.parametrize("sid", FOOTPRINT_SPECS)
def test_footprint(torch, sid):
    """Nothing outside the outputs is written, the inputs are unchanged, the outputs are fully written (0xFF fill == 0x00
    fill) and do not depend on what lies around the inputs, at a row-slice skew and with ragged B."""
    s, eng = vc.CENSUS[sid], engine(sid)
    rep = Report(f"linearise {sid}")
    for B in (1, 17, 37):
        rng = rng_of("lin", sid, B)
        x, u = vc.states(rng, s["n"], B), rng.uniform(vc.U_MIN, vc.U_MAX, size=(B, s["m"])).astype(np.float32)
        footprint(rep, torch, eng, JacobianOp(x, u))
        for H in (1, 6):
            x0, U, cost = 0.3 * vc.states(rng, s["n"], B), vc.controls(rng, B, H, s["m"]), vc.cost_of(s, rng)
            for integ in (0, 1):
                footprint(rep, torch, eng, GainsOp(cost, x0, U, integ, vc.dt_of(s), with_P=(integ == 0)))
    rep.finish()


# ----------------------------------------------------------------------------- 4. graph
def test_graph_replay_equals_eager(torch):
    sid = lc.HEADLINE
    s, eng = vc.CENSUS[sid], engine(sid)
    rng = np.random.default_rng(31)
    B, H = 37, 6
    cost = vc.cost_of(s, rng)
    x0 = torch.as_tensor(0.3 * vc.states(rng, 4, B), device="cuda:0")
    u = torch.as_tensor(vc.controls(rng, B, H, 1), device="cuda:0")

    def run():
        A, Bm, traj = eng.rollout_linearize(x0, u, cost, "rk4", 0.02)
        r = eng.tvlqr(A, Bm, cost, mu=0.01, want_P=True)
        return [A, Bm, traj, r["K"], r["P0"], r["P"], r["status"]]

    eager = [t.clone() for t in run()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # one stream, one branch: K1 -> linearise -> tvlqr
        outs = run()
    for _ in range(2):
        for t in outs:
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert fp.same_bytes(torch, fp.as_bytes(torch, a), fp.as_bytes(torch, b))
    # new inputs in the captured buffers are picked up by the next replay
    x0.mul_(0.5)
    fresh = [t.clone() for t in run()]
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, fresh):
        assert fp.same_bytes(torch, fp.as_bytes(torch, a), fp.as_bytes(torch, b))


# ----------------------------------------------------------------------------- 5. controllers
CFG = os.path.join(vc.ROOT, "configs", "cartpole_mpc.yaml")


def _controller(torch, which):
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import MPCController
    from phnn_mpc_amd.mpc_controller_canonical import MPCControllerCanonical
    cls, name = (pHNN, "phnn_cartpole") if which == "phnn" else (pHNN_Canonical, "canonical_cartpole")
    w = ol.load_weights(name)
    model = cls(CFG)
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    model.use_device("cuda:0")
    if which == "phnn":
        return MPCController(phnn_model=model, horizon=12, dt=0.02, Q=[10.0, 200.0, 1.0, 10.0], R=0.01, u_min=-10.0, u_max=10.0), 1
    ctl = MPCControllerCanonical(model, horizon=12, dt=0.02)
    return ctl, ctl.input_dim


@pytest.mark.parametrize("which", ["phnn", "canonical"])
def test_feedback_gains_equal_the_three_engine_calls(torch, which):
    ctl, m = _controller(torch, which)
    eng = ctl.engine
    rng = np.random.default_rng(41)
    B, H = 19, ctl.horizon
    x0 = (rng.uniform(-1, 1, size=(B, 4)) * [0.5, 0.2, 0.3, 0.3]).astype(np.float32)
    u = rng.uniform(-12, 12, size=(B, H, m)).astype(np.float32)  # some outside the controller's bounds
    out = ctl.feedback_gains(x0, u, mu=1e-3)
    cost = ctl._cost()
    _, traj = eng.rollout_cost(x0, u, cost, ctl.integrator, ctl.dt, want_traj=True)
    A, Bm, _ = eng.rollout_linearize(x0, u, cost, ctl.integrator, ctl.dt, traj=traj)
    ref = eng.tvlqr(A, Bm, cost, mu=1e-3, want_P=True)
    for k, t in (("traj", traj), ("A", A), ("Bm", Bm), ("K", ref["K"]), ("P0", ref["P0"]), ("P", ref["P"]), ("status", ref["status"])):
        assert fp.same_bytes(torch, fp.as_bytes(torch, out[k]), fp.as_bytes(torch, t)), k
    assert not bool(out["status"].any()) and bool(torch.isfinite(out["K"]).all())
    assert bool((out["Bm"] == 0).all(dim=2).any())  # a clamped control: its column of B_t is zero
