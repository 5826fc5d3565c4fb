"""k_lbfgs pinned bit for bit: engine.solve_lbfgs == the float32 model of the kernel (lbfgs_kernel_model.py) fed the
same K1 / K2 evaluations (engine.rollout_cost_grad on the same engine, integrator and reference), for every kernel width
E4 = 1 .. 4, every residue of N = H*m mod 4, models with m = 1 .. 4, Euler and RK4.  No tolerances: u_last, costs,
n_iter and func_evals are compared as bits.

  shapes    the table below: N = 1 ... 256, pHNN / canonical / ODEFunc models, per-problem references, a warm start
            with controls outside the clamp
  paths     a full wrapped history of 100 pairs, dropped updates (ys <= 1e-10), every forced break reason at N = 21,
            B = 4099 (many workgroups, a partial last one)
  limit     N = 257 is refused with PHNN_ERR_UNSUPPORTED and leaves u alone; the controller raises
  layout    phnn_lbfgs_workspace_bytes == the layout of DESIGN.md section 11 at ragged N

Every case asserts that it reached what it is there for (E4, N mod 4, a wrap, a dropped update, the break reason).  On a
mismatch the first differing problem, field and the model's break reasons are reported; outer_steps = k runs exactly the
first k outer steps, so a smaller outer_steps narrows a mismatch down to its step.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from lbfgs_kernel_model import kernel_e4, kernel_schedule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
PHNN_ERR_UNSUPPORTED = -2
STATE_BYTES = 48  # sizeof(LbfgsState)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def weights(model):
    if model in ("phnn_cartpole", "odefunc_cartpole"):
        return ol.load_weights(model)
    fname = "golden_m2.npz" if model.endswith("m2_fix") else "golden_m34.npz"
    return ol.load_named_golden(fname)[1][model]


_ENGINES = {}


def engine(model):
    from phnn_mpc_amd.engine import RolloutEngine
    if model not in _ENGINES:
        _ENGINES[model] = RolloutEngine(weights(model), "cuda:0")
    return _ENGINES[model]


def make_cost(eng, u_lim=10.0):
    from phnn_mpc_amd import _capi
    R = [0.01 * (1 + i) for i in range(eng.m)]
    return _capi.make_cost(eng.n, eng.m, [10.0, 100.0, 1.0, 10.0], R, [0.0] * 4, -u_lim, u_lim)


def states(B, seed, scale=(0.5, 0.1, 0.3, 0.3)):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, size=(B, 4)) * np.array(scale)).astype(np.float32)


def check(torch, eng, x0, u0, cost, integrator="euler", x_ref=None, **kw):
    """solve_lbfgs == kernel_schedule bit for bit; -> the model's result."""
    B, H, m = u0.shape
    N = H * m
    ws = {}

    def ev(u, rows):
        assert list(rows) == list(range(B))  # the schedule evaluates every problem in every slot
        rk = {} if x_ref is None else {"x_ref": x_ref}
        c, g = eng.rollout_cost_grad(x0, u.to(eng.device).reshape(B, H, m), cost, integrator, 0.02, workspace=ws, **rk)
        return c.cpu().clone(), g.reshape(B, N).cpu().clone()

    model = kernel_schedule(ev, u0.reshape(B, N).cpu(), **kw)
    rk = {} if x_ref is None else {"x_ref": x_ref}
    dev = eng.solve_lbfgs(x0, u0, cost, integrator, 0.02, **kw, **rk)
    got = {"u_last": dev["u_last"].reshape(B, N).cpu(), "costs": dev["costs"].cpu(), "n_iter": dev["n_iter"].cpu(),
           "func_evals": dev["func_evals"].cpu()}
    for k in ("u_last", "costs", "n_iter", "func_evals"):
        a = got[k].contiguous().view(torch.int32)
        b = model[k].contiguous().view(torch.int32)
        if not torch.equal(a, b):
            diff = (a != b).reshape(a.shape[0], -1) if k != "costs" else (a != b).T
            p = int(diff.any(dim=1).nonzero()[0, 0])
            raise AssertionError(f"{k} differs first at problem {p} of {B} (N = {N}, E4 = {kernel_e4(N)}): device "
                                 f"{got[k][p] if k != 'costs' else got[k][:, p]} vs model "
                                 f"{model[k][p] if k != 'costs' else model[k][:, p]}; model n_iter "
                                 f"{int(model['n_iter'][p])}, reasons {dict(model['reasons'])}")
    assert torch.isfinite(model["u_last"]).all() and torch.isfinite(model["costs"]).all()
    return model


# model, m, H, E4, integrator, B, solve options, extra
TABLE = [
    ("phnn_cartpole", 1, 1, 1, "euler", 1, dict(lr=0.5, outer_steps=2, max_iter=10), None),
    ("phnn_cartpole", 1, 7, 1, "euler", 5, dict(lr=0.5, outer_steps=2, max_iter=10, history_size=1), "wrap"),
    ("phnn_cartpole", 1, 64, 1, "euler", 6, dict(lr=0.5, outer_steps=2, max_iter=10), None),
    ("phnn_cartpole", 1, 65, 2, "euler", 6, dict(lr=0.5, outer_steps=2, max_iter=10, history_size=2), "wrap"),
    ("phnn_m2_fix", 2, 63, 2, "rk4", 5, dict(lr=0.5, outer_steps=2, max_iter=8), None),
    ("phnn_m3_fix", 3, 43, 3, "euler", 5, dict(lr=0.5, outer_steps=2, max_iter=8), None),
    ("canonical_m3", 3, 57, 3, "rk4", 5, dict(lr=0.5, outer_steps=2, max_iter=8), None),
    ("phnn_m4_gnet", 4, 48, 3, "euler", 5, dict(lr=0.5, outer_steps=2, max_iter=8), "x_ref"),
    ("phnn_cartpole", 1, 193, 4, "euler", 5, dict(lr=0.5, outer_steps=2, max_iter=8), "warm"),
    ("odefunc_cartpole", 1, 255, 4, "euler", 5, dict(lr=0.5, outer_steps=2, max_iter=8), None),
    ("phnn_m4_gnet", 4, 64, 4, "euler", 5, dict(lr=0.5, outer_steps=2, max_iter=8), None),
]
# E4 and N mod 4 are properties of the shape: lbfgs_launch picks k_lbfgs<E4> deterministically from Np = 4*ceil(N/4)
# (kernel_e4 restates that choice), so the table's shapes are what makes each width and residue run on the device.
# Together the rows cover E4 = 1 .. 4 and every N mod 4 (asserted below).


def test_table_covers_every_width_and_residue():
    shapes = {(kernel_e4(r[1] * r[2]), r[1] * r[2] % 4) for r in TABLE}
    assert {e for e, _ in shapes} == {1, 2, 3, 4} and {r for _, r in shapes} == {0, 1, 2, 3}
    assert {r for e, r in shapes if e in (3, 4)} == {0, 1, 3}  # the two widths that had never run, ragged and not
    assert max(r[1] * r[2] for r in TABLE) == 256


@pytest.mark.parametrize("model,m,H,E4,integrator,B,kw,extra", TABLE,
                         ids=[f"{r[0]}-H{r[2]}-N{r[1] * r[2]}" for r in TABLE])
def test_device_equals_kernel_model(torch, model, m, H, E4, integrator, B, kw, extra):
    eng = engine(model)
    assert eng.m == m
    N = H * m
    assert kernel_e4(N) == E4
    x0 = torch.tensor(states(B, N), device=eng.device)
    cost = make_cost(eng)
    u0 = torch.zeros(B, H, m, device=eng.device)
    x_ref = None
    if extra == "warm":  # a warm start with some controls outside the clamp [-10, 10]
        g = torch.Generator().manual_seed(H)
        u0 = (4.0 * torch.randn(B, H, m, generator=g)).to(eng.device)
        u0[:, ::7] = 12.5 * torch.sign(u0[:, ::7] + 1e-3)
        assert (u0.abs() > 10.0).any() and (u0.abs() < 10.0).any()
    if extra == "x_ref":  # a time-varying reference per problem
        t = torch.linspace(0.0, 1.0, H + 1)
        amp = torch.tensor(states(B, N + 1, scale=(0.3, 0.05, 0.1, 0.1)))
        x_ref = (amp[:, None, :] * t[None, :, None]).contiguous().to(eng.device)
    r = check(torch, eng, x0, u0, cost, integrator, x_ref=x_ref, **kw)
    assert r["reasons"]["push"] > 0 and int(r["n_iter"].min()) >= 2, r["reasons"]
    if extra == "wrap":
        assert int(r["pushes"].max()) > kw["history_size"], r["pushes"]


def _small(B=5, H=7, seed=11):
    eng = engine("phnn_cartpole")
    import torch
    x0 = torch.tensor(states(B, seed), device=eng.device)
    return eng, x0, torch.zeros(B, H, 1, device=eng.device), make_cost(eng)


def test_full_wrapped_history(torch):
    eng, x0, u0, cost = _small()
    r = check(torch, eng, x0, u0, cost, lr=0.05, outer_steps=6, max_iter=20, tolerance_grad=0.0, tolerance_change=0.0)
    assert int(r["pushes"].max()) > 100, (r["pushes"], r["reasons"])


def test_dropped_history_updates(torch):
    eng, x0, u0, cost = _small(seed=12)
    r = check(torch, eng, x0, u0, cost, lr=1e-6, outer_steps=2, max_iter=6, tolerance_change=0.0)
    assert r["reasons"]["skip_update"] > 0, r["reasons"]


@pytest.mark.parametrize("forced,kw", [
    ("opt_cond_start", dict(tolerance_grad=1e6)),
    ("max_eval", dict(max_eval=3)),
    ("gtd", dict(tolerance_change=1e4)),
    ("lack_of_progress", None),
    ("max_iter", dict(max_iter=5, tolerance_change=0.0, tolerance_grad=0.0)),
])
def test_forced_break_paths_ragged(torch, forced, kw):
    eng, x0, u0, cost = _small(B=13, H=21, seed=3)
    assert 21 % 4 == 1
    if forced == "lack_of_progress":  # the smallest tolerance_change that stops some step() on |d t| or the loss change
        ws = {}

        def ev(u, rows):
            c, g = eng.rollout_cost_grad(x0, u.to(eng.device).reshape(13, 21, 1), cost, "euler", 0.02, workspace=ws)
            return c.cpu().clone(), g.reshape(13, 21).cpu().clone()

        for tc in (1e-3, 1e-2, 1e-1, 1.0):
            reasons = kernel_schedule(ev, u0.reshape(13, 21).cpu(), lr=0.5, outer_steps=3, tolerance_change=tc)["reasons"]
            if reasons["small_step"] + reasons["loss_change"] > 0:
                break
        kw = dict(tolerance_change=tc)
    r = check(torch, eng, x0, u0, cost, lr=0.5, outer_steps=3, **kw)
    if forced == "lack_of_progress":
        assert r["reasons"]["small_step"] + r["reasons"]["loss_change"] > 0, r["reasons"]
    else:
        assert r["reasons"][forced] > 0, r["reasons"]


def test_ragged_large_batch(torch):
    B = 4099  # 256 workgroups of 16 problems and a last one with 3
    eng, x0, u0, cost = _small(B=B, H=7, seed=13)
    x0 = torch.tensor(states(B, 13, scale=(1.0, 0.3, 0.5, 0.5)), device=eng.device)
    r = check(torch, eng, x0, u0, cost, lr=0.5, outer_steps=2, max_iter=10, history_size=5, tolerance_change=1e-6)
    assert len(set(r["n_iter"].tolist())) > 1 and r["reasons"]["push"] > 0, r["reasons"]


# ------------------------------------------------------------------ the limit N = H*m <= 256
@pytest.mark.parametrize("model,H", [("phnn_cartpole", 257), ("phnn_m4_gnet", 65)])
def test_limit_is_refused_and_leaves_u(torch, model, H):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    eng = engine(model)
    assert H * eng.m > 256 and kernel_e4(H * eng.m) == 0
    B, lib, cost = 3, eng.lib, make_cost(eng)
    f = dict(dtype=torch.float32, device=eng.device)
    x0 = torch.tensor(states(B, 14), device=eng.device)
    u = torch.full((B, H, eng.m), 0.25, **f)
    grad, cst, traj = torch.empty(B, H, eng.m, **f), torch.empty(B, **f), torch.empty(B, H + 1, eng.n, **f)
    nbytes = eng.lbfgs_workspace_bytes(B, H, 4)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)
    o = _capi.LbfgsOptions()
    o.outer_steps, o.max_iter, o.max_eval, o.history_size, o.lr = 1, 5, 0, 4, 1.0
    o.tolerance_grad, o.tolerance_change = 1e-7, 1e-9
    rc = lib.phnn_solve_lbfgs(eng.h, x0.data_ptr(), u.data_ptr(), B, H, C.byref(cost), None, 0, 0.02, C.byref(o),
                              grad.data_ptr(), cst.data_ptr(), traj.data_ptr(), None, ws.data_ptr(), nbytes, None, None,
                              None, None)
    assert rc == PHNN_ERR_UNSUPPORTED, rc
    assert b"256" in lib.phnn_last_error(eng.h)
    torch.cuda.synchronize()
    assert torch.equal(u, torch.full_like(u, 0.25))
    with pytest.raises(PhnnError, match="256"):  # the wrapper raises (it solves on a clone of u)
        eng.solve_lbfgs(x0, u, cost, outer_steps=1)


def test_controller_with_too_long_a_horizon_raises(torch):
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import MPCController
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights("phnn_cartpole").items()})
    c = MPCController(phnn_model=m, horizon=257, dt=0.02, Q=[10.0, 200.0, 1.0, 10.0], R=0.01,
                      target_state=[0.0] * 4, u_min=-15.0, u_max=15.0, optimizer_type="LBFGS", lr=0.5, max_iterations=1)
    with pytest.raises(RuntimeError, match="256"):
        c.solve_batch(states(2, 15))


# ------------------------------------------------------------------ workspace layout
def _layout_bytes(B, N, hs):
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    Np = 4 * ((N + 3) // 4)
    ro = al(B * STATE_BYTES)
    alpha = al(ro + B * hs * 4)
    d = al(alpha + B * hs * 4)
    pg = al(d + B * Np * 4)
    hist = al(pg + B * Np * 4)
    return al(hist + B * hs * 2 * Np * 4)


@pytest.mark.parametrize("model,B,H,hs", [("phnn_cartpole", 3, 7, 5), ("phnn_cartpole", 17, 1, 1),
                                          ("phnn_m3_fix", 5, 43, 100), ("canonical_m3", 1, 57, 3),
                                          ("phnn_m2_fix", 4099, 63, 2)])
def test_workspace_bytes_match_the_documented_layout(torch, model, B, H, hs):
    eng = engine(model)
    N = H * eng.m
    assert N % 4 != 0  # ragged: Np > N
    assert eng.lbfgs_workspace_bytes(B, H, hs) == _layout_bytes(B, N, hs), (model, B, H, hs)
