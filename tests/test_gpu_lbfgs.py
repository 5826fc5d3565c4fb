"""Batched L-BFGS solve on the device (phnn_solve_lbfgs, kernel k_lbfgs; engine.solve_lbfgs, MPCController with
optimizer_type='LBFGS' through solve_batch / compute_control_batch / DeviceClosedLoop).

  G13         compute_control_batch reproduces the reference's own L-BFGS output (golden_controllers.npz lbfgs_u0)
  host torch  B = 37 problems == 37 host torch.optim.LBFGS runs on the engine's cost / gradient, to rounding
  restatement == the CPU restatement of the slot schedule (lbfgs_reference.py) on the same engine: pHNN H = 20,
              an m = 2 model at H = 50, a wrapped history, and every forced break reason (counters exactly)
  invariance  a problem alone == the same problem anywhere in a B = 4096 batch, split-tile == whole-tile, bitwise
  tracking    per-problem setpoints through x_ref == separate solves with x_target set to each, bitwise
  graph/loop  graph replay == eager; DeviceClosedLoop with an L-BFGS controller == run_mpc_batch; x_ref loop runs
  arguments   PHNN_ERR_INVALID_ARG for bad options / buffers; outer_steps = 0 leaves u and the counters alone

These check torch's semantics and the host path.  The kernel's own arithmetic is pinned bit for bit, against a float32
model of k_lbfgs, at every kernel width, ragged N and m = 1 .. 4, in tests/test_gpu_lbfgs_kernel.py.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from lbfgs_reference import lbfgs_schedule, torch_lbfgs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
G13 = dict(horizon=20, dt=0.02, Q=[10.0, 200.0, 1.0, 10.0], R=0.01, target_state=[0.0, 0.0, 0.0, 0.0], u_min=-15.0,
           u_max=15.0, optimizer_type="LBFGS", lr=0.5, max_iterations=3)
TOLERANCE_BREAKS = {"opt_cond_start", "opt_cond", "small_step", "loss_change", "gtd"}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def ctl():
    with np.load(os.path.join(ol.GOLDEN, "golden_controllers.npz")) as z:
        return {k: z[k] for k in z.files}


_ENGINES = {}


def engine(split="auto"):
    from phnn_mpc_amd.engine import RolloutEngine
    if split not in _ENGINES:
        _ENGINES[split] = RolloutEngine(ol.load_weights("phnn_cartpole"), "cuda:0", split=split)
    return _ENGINES[split]


def g13_cost():
    from phnn_mpc_amd import _capi
    return _capi.make_cost(4, 1, G13["Q"], G13["R"], G13["target_state"], G13["u_min"], G13["u_max"])


def controller(torch, **kw):
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import MPCController
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights("phnn_cartpole").items()})
    return MPCController(phnn_model=m, **{**G13, **kw})


def states(B, seed, scale=(0.5, 0.1, 0.3, 0.3)):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, size=(B, 4)) * np.array(scale)).astype(np.float32)


def gpu_evaluate(torch, eng, x0, cost, H, m=1, x_ref=None):
    """evaluate(u (k, H*m) CPU, rows) for lbfgs_reference: the engine's K1 / K2 on the rows' problems, batched."""
    def ev(u, rows):
        idx = torch.tensor(list(rows), device=eng.device)
        kw = {} if x_ref is None else {"x_ref": x_ref[idx]}
        c, g = eng.rollout_cost_grad(x0[idx], u.to(eng.device).reshape(-1, H, m), cost, "euler", 0.02, **kw)
        return c.cpu().clone(), g.reshape(u.shape[0], -1).cpu().clone()
    return ev


def solve(eng, x0, cost, H, m=1, **kw):
    import torch
    u0 = torch.zeros(x0.shape[0], H, m, device=eng.device)
    return eng.solve_lbfgs(x0, u0, cost, "euler", 0.02, **kw)


def close_to(torch, dev, ref, N, tol=5e-4):
    u = dev["u_last"].reshape(-1, N).cpu()
    scale = max(1.0, float(ref["u_last"].abs().max()))
    assert float((u - ref["u_last"]).abs().max()) <= tol * scale, float((u - ref["u_last"]).abs().max())
    c = dev["costs"].cpu()
    assert torch.allclose(c, ref["costs"], rtol=1e-4, atol=1e-6), (c - ref["costs"]).abs().max()


def test_g13_through_the_batched_path(torch, ctl):
    c = controller(torch)
    u0 = c.compute_control_batch(ctl["mpc_x0"][None])
    assert u0.shape == (1, 1) and abs(u0[0, 0] - ctl["lbfgs_u0"][0]) < 5e-4 * max(1.0, abs(ctl["lbfgs_u0"][0])), (u0, ctl["lbfgs_u0"])


def test_versus_host_torch_lbfgs(torch):
    eng, cost, H, B = engine(), g13_cost(), 20, 37
    x0 = torch.tensor(states(B, 1), device=eng.device)
    ev = gpu_evaluate(torch, eng, x0, cost, H)
    host = torch_lbfgs(ev, torch.zeros(B, H), lr=0.5, outer_steps=3)
    dev = solve(eng, x0, cost, H, lr=0.5, outer_steps=3)
    close_to(torch, dev, host, H)
    fin_d = eng.rollout_cost(x0, dev["u_last"], cost).cpu()
    fin_h = eng.rollout_cost(x0, host["u_last"].reshape(B, H, 1).to(eng.device), cost).cpu()
    assert torch.allclose(fin_d, fin_h, rtol=1e-4), (fin_d / fin_h - 1).abs().max()
    # counters: equal unless a tolerance break (decided by rounding) happened somewhere on the host path
    reasons = lbfgs_schedule(ev, torch.zeros(B, H), lr=0.5, outer_steps=3)["reasons"]
    if not TOLERANCE_BREAKS & set(reasons):
        assert torch.equal(dev["n_iter"].cpu(), host["n_iter"]) and torch.equal(dev["func_evals"].cpu(), host["func_evals"])


@pytest.mark.parametrize("case", ["g13", "wrap", "m2"])
def test_versus_restatement(torch, case):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import RolloutEngine
    if case == "m2":
        g, w = ol.load_m2_golden()
        eng = RolloutEngine(w["phnn_m2_fix"], "cuda:0")
        m, H, B = 2, 50, 9
        cost = _capi.make_cost(4, 2, [10.0, 100.0, 1.0, 10.0], [0.01, 0.02], [0.0] * 4, -10.0, 10.0)
        kw = dict(lr=0.5, outer_steps=1, max_iter=8)  # few iterations: L-BFGS amplifies rounding differences
    else:
        eng, m, H, B, cost = engine(), 1, 20, 11, g13_cost()
        kw = dict(lr=0.5, outer_steps=3) if case == "g13" else dict(lr=0.05, outer_steps=2, max_iter=40, max_eval=60,
                                                                     history_size=3, tolerance_change=0.0)
    x0 = torch.tensor(states(B, 2), device=eng.device)
    ref = lbfgs_schedule(gpu_evaluate(torch, eng, x0, cost, H, m), torch.zeros(B, H * m), **kw)
    dev = solve(eng, x0, cost, H, m, **kw)
    close_to(torch, dev, ref, H * m)
    if not TOLERANCE_BREAKS & set(ref["reasons"]):
        assert torch.equal(dev["n_iter"].cpu(), ref["n_iter"]) and torch.equal(dev["func_evals"].cpu(), ref["func_evals"])
    if case == "wrap":
        assert ref["reasons"]["push"] > 3 * B


@pytest.mark.parametrize("forced,kw", [
    ("opt_cond_start", dict(tolerance_grad=1e6)),
    ("max_eval", dict(max_eval=3)),
    ("gtd", dict(tolerance_change=1e4)),
    ("lack_of_progress", None),
    ("max_iter", dict(max_iter=5, tolerance_change=0.0, tolerance_grad=0.0)),
])
def test_forced_break_paths(torch, forced, kw):
    eng, cost, H, B = engine(), g13_cost(), 20, 13
    x0 = torch.tensor(states(B, 3), device=eng.device)
    ev = gpu_evaluate(torch, eng, x0, cost, H)
    if forced == "lack_of_progress":  # the smallest tolerance_change that stops some step() on |d t| or on the loss change
        for tc in (1e-3, 1e-2, 1e-1, 1.0):
            ref = lbfgs_schedule(ev, torch.zeros(B, H), lr=0.5, outer_steps=3, tolerance_change=tc)
            if ref["reasons"]["small_step"] + ref["reasons"]["loss_change"] > 0:
                break
        kw = dict(tolerance_change=tc)
    args = dict(lr=0.5, outer_steps=3, **kw)
    ref = lbfgs_schedule(ev, torch.zeros(B, H), **args)
    if forced == "lack_of_progress":
        assert ref["reasons"]["small_step"] + ref["reasons"]["loss_change"] > 0, ref["reasons"]
    else:
        assert ref["reasons"][forced] > 0, ref["reasons"]
    dev = solve(eng, x0, cost, H, **args)
    assert torch.equal(dev["n_iter"].cpu(), ref["n_iter"]), (dev["n_iter"], ref["n_iter"])
    assert torch.equal(dev["func_evals"].cpu(), ref["func_evals"]), (dev["func_evals"], ref["func_evals"])
    close_to(torch, dev, ref, H)


def test_bitwise_invariance_batch_position_and_split(torch):
    cost, H, B = g13_cost(), 20, 4096
    X = states(B, 4)
    outs = {}
    for split in ("auto", "never"):
        eng = engine(split)
        outs[split] = solve(eng, torch.tensor(X, device=eng.device), cost, H, lr=0.5, outer_steps=3)
    for k in ("u_last", "costs", "n_iter", "func_evals"):
        assert torch.equal(outs["auto"][k], outs["never"][k]), k
    eng = engine()
    for b in (0, 1, 777, B - 1):
        one = solve(eng, torch.tensor(X[b:b + 1], device=eng.device), cost, H, lr=0.5, outer_steps=3)
        for k in ("u_last", "func_evals", "n_iter"):
            assert torch.equal(one[k][0], outs["auto"][k][b]), (k, b)
        assert torch.equal(one["costs"][:, 0], outs["auto"]["costs"][:, b])


def test_tracking_setpoints_bitwise(torch):
    from phnn_mpc_amd import _capi
    eng, H, B = engine(), 20, 6
    x0 = torch.tensor(states(B, 5), device=eng.device)
    targets = torch.tensor(states(B, 6, scale=(0.3, 0.05, 0.1, 0.1)), device=eng.device)
    tr = solve(eng, x0, g13_cost(), H, lr=0.5, outer_steps=3, x_ref=targets[:, None, :])
    for b in range(B):
        c = _capi.make_cost(4, 1, G13["Q"], G13["R"], targets[b].cpu().numpy(), G13["u_min"], G13["u_max"])
        one = solve(eng, x0[b:b + 1], c, H, lr=0.5, outer_steps=3)
        for k in ("u_last", "n_iter", "func_evals"):
            assert torch.equal(one[k][0], tr[k][b]), (k, b)


def test_graph_equals_eager(torch):
    from phnn_mpc_amd.solver import GraphedLBFGS
    eng, cost, H, B = engine(), g13_cost(), 20, 37
    x0 = torch.tensor(states(B, 7), device=eng.device)
    u0 = torch.zeros(B, H, 1, device=eng.device)
    kw = dict(lr=0.5, outer_steps=3)
    eager = eng.solve_lbfgs(x0, u0, cost, "euler", 0.02, **kw)
    gs = GraphedLBFGS(eng)
    for _ in range(2):
        gr = gs(x0, u0, cost, "euler", 0.02, **kw)
        for k in ("u_last", "costs", "n_iter", "func_evals"):
            assert torch.equal(gr[k], eager[k]), k
    c = controller(torch)
    c.use_graph = True
    assert np.array_equal(c.compute_control_batch(states(5, 8)), controller(torch).compute_control_batch(states(5, 8)))


def test_device_closed_loop_equals_host_loop(torch):
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch, run_mpc_batch_device
    c = controller(torch)
    X0 = states(64, 9).astype(np.float64)
    host = run_mpc_batch(BatchedCartPole(0.02), c, X0, 10)
    dev = run_mpc_batch_device(c, X0, 10, use_graph=True)
    assert np.array_equal(dev["controls"], host["controls"])
    assert np.allclose(dev["states"], host["states"], rtol=0, atol=1e-12)
    assert np.array_equal(dev["done_step"], host["done_step"])


def test_device_closed_loop_with_reference_runs(torch):
    from phnn_mpc_amd.closed_loop import run_mpc_batch_device
    c = controller(torch)
    B, T = 16, 6
    ref = np.zeros((B, T + c.horizon + 1, 4), np.float32)
    ref[:, :, 0] = np.linspace(0.0, 0.2, ref.shape[1])[None, :]
    out = run_mpc_batch_device(c, states(B, 10).astype(np.float64), T, x_ref=torch.tensor(ref, device="cuda:0"))
    assert out["controls"].shape == (T, B, 1) and np.all(np.isfinite(out["controls"]))
    plain = run_mpc_batch_device(c, states(B, 10).astype(np.float64), T)
    assert not np.array_equal(out["controls"], plain["controls"])


def test_argument_checks(torch):
    from phnn_mpc_amd import _capi
    eng, cost = engine(), g13_cost()
    lib = eng.lib
    B, H = 4, 5
    x0 = torch.zeros(B, 4, device=eng.device)
    u = torch.ones(B, H, 1, device=eng.device)
    out = eng.solve_lbfgs(x0, u, cost, "euler", 0.02, outer_steps=0)
    assert torch.equal(out["u_last"], u) and out["n_iter"].tolist() == [0] * B and out["func_evals"].tolist() == [0] * B
    assert eng.solve_lbfgs(x0[:0], u[:0], cost, outer_steps=2)["u_last"].shape == (0, H, 1)

    f = dict(dtype=torch.float32, device=eng.device)
    grad, cst, traj = torch.empty(B, H, 1, **f), torch.empty(B, **f), torch.empty(B, H + 1, 4, **f)
    nbytes = eng.lbfgs_workspace_bytes(B, H, 100)
    assert nbytes > B * 100 * 2 * H * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device=eng.device)

    def call(opt, ws_size=nbytes, grad_p=grad.data_ptr()):
        return lib.phnn_solve_lbfgs(eng.h, x0.data_ptr(), u.data_ptr(), B, H, C.byref(cost), None, 0, 0.02, C.byref(opt),
                                    grad_p, cst.data_ptr(), traj.data_ptr(), None, ws.data_ptr(), ws_size, None, None,
                                    None, None)

    def opts(**kw):
        o = _capi.LbfgsOptions()
        o.outer_steps, o.max_iter, o.max_eval, o.history_size, o.lr = 1, 20, 0, 100, 1.0
        o.tolerance_grad, o.tolerance_change = 1e-7, 1e-9
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    for bad in (dict(history_size=0), dict(max_iter=0), dict(lr=float("nan")), dict(lr=float("inf")), dict(outer_steps=-1),
                dict(max_eval=-1)):
        assert call(opts(**bad)) == -1, bad
        assert lib.phnn_last_error(eng.h)
    assert call(opts(), ws_size=nbytes - 1) == -1
    assert b"too small" in lib.phnn_last_error(eng.h)
    assert call(opts(), grad_p=None) == -1
    assert lib.phnn_solve_lbfgs(eng.h, x0.data_ptr(), u.data_ptr(), B, H, C.byref(cost), None, 0, 0.02, None,
                                grad.data_ptr(), cst.data_ptr(), traj.data_ptr(), None, ws.data_ptr(), nbytes, None, None,
                                None, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(u, torch.ones_like(u))  # nothing ran
