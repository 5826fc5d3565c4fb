"""The MPPI solve on the device (engine.mppi_sample / mppi_update / solve_mppi, kernels k_sample and k_mppi_update).

  primitives  mppi_sample vs the float64 model (tests/mppi_model.py); mppi_update vs the float64 model fed the device's
              own samples and K1 costs.  Device log / sqrt / sincospi / exp are not bit-specified, so the allowance is
              ALLOW = 8 x the distance of the model's float32 form from its float64 form on the same inputs (largest
              entry of the tensor) plus one float32 ulp of the largest entry; best_u and costs are exact copies and
              compared as bits.
  oracle      one iteration end to end: the device's samples costed by the float64 CPU oracle, float64 update of those
              costs vs the device's update, within  2 * 1e-5 * max_k |S64| / lambda * max_k |v|  (the cost tolerance
              pushed through the softmin: |dp|_1 <= 2 max |dS| / lambda) + the allowance above, per problem and
              iteration, each iteration restarted from the device's nominal.
  bitwise     solve_mppi == solver.mppi_solve over the primitives; repeat == first; B problems at once == each alone
              with its problem_offset (B = 37 and 4096: split-tile and whole-tile K1); graph == eager; seed / epoch
              change the samples; per-problem x_ref == separate solves with that x_target; the device closed loop ==
              the host loop.
  saturated   u_init = 2 u_max: Adam returns u_init bit for bit, MPPI ends strictly below cost(clamp(u_init));
              iters = 0 returns best_cost = +inf, best_u = 0, u_last = clamp(u_init).
Shapes cover the pHNN, canonical and ODEFunc goldens, an m = 2 model, Euler and RK4, B = 1 / 37 / 4096, K = 2 / 30 / 64,
every k_mppi_update width (1 .. 4 float4 per lane) and every N = H*m mod 4.
"""
import numpy as np
import pytest
import yaml

import mppi_model as mm
import oracle_lib as ol
from test_mppi_model import CFG, SAT, SEED, X0, saturated_case

pytestmark = pytest.mark.gpu
ALLOW = 8  # the K = 8 rule of tests/test_gpu_trained.py for GPU-vs-float32-floor comparisons

# (model, integrator, B, K, H): N = H*m -> (float4 per lane, N mod 4) = 20:(1,0) 77:(2,1) 150:(3,2) 255:(4,3) 50:(1,2)
CASES = [("phnn_cartpole", "euler", 37, 64, 20), ("phnn_cartpole", "rk4", 1, 30, 77),
         ("canonical_cartpole", "euler", 37, 30, 150), ("odefunc_cartpole", "rk4", 37, 2, 255),
         ("phnn_m2_fix", "euler", 37, 64, 25), ("phnn_cartpole", "euler", 4096, 30, 20)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def weights(model):
    return ol.load_named_golden("golden_m2.npz")[1][model] if model == "phnn_m2_fix" else ol.load_weights(model)


_ENGINES = {}


def engine(model):
    from phnn_mpc_amd.engine import RolloutEngine
    if model not in _ENGINES:
        _ENGINES[model] = RolloutEngine(weights(model), "cuda:0")
    return _ENGINES[model]


def make_cost(eng, u_lim=10.0, x_target=(0.0, 0.0, 0.0, 0.0)):
    from phnn_mpc_amd import _capi
    return _capi.make_cost(eng.n, eng.m, [10.0, 100.0, 1.0, 10.0], [0.01 * (1 + i) for i in range(eng.m)], list(x_target),
                           -u_lim, u_lim)


def states(B, seed, scale=(0.5, 0.1, 0.3, 0.3)):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, size=(B, 4)) * np.array(scale)).astype(np.float32)


def nominal(B, H, m, seed, lim=12.0):
    """Nominal controls, some of them past the +-10 clamp."""
    return np.random.default_rng(seed).uniform(-lim, lim, size=(B, H, m)).astype(np.float32)


def ulp(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def sigma_of(m):
    return tuple(2.0 + 0.5 * i for i in range(m))


def allowance(f32, f64):
    """ALLOW x the float32 form's distance from the float64 form + one ulp of the largest entry."""
    return ALLOW * float(np.abs(f32.astype(np.float64) - f64).max()) + ulp(f64)


def npy(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------- 7. primitives against the model
@pytest.mark.parametrize("model, integ, B, K, H", CASES)
def test_primitives_against_the_float64_model(torch, model, integ, B, K, H):
    eng = engine(model)
    m, N = eng.m, H * eng.m
    cost = make_cost(eng)
    x0 = torch.tensor(states(B, 1), device="cuda")
    u = torch.tensor(np.clip(nominal(B, H, m, 2), -10, 10), device="cuda")
    sig, lam, it, ep, off = sigma_of(m), 25.0, 3, 11, 1000
    v, x0r = eng.mppi_sample(x0, u, cost, K, sig, SEED, it, epoch=ep, problem_offset=off)
    s = eng.rollout_cost(x0r, v, cost, integ, 0.02)
    un = npy(u).reshape(B, N)
    vd = npy(v).reshape(B * K, N)
    args = (un, sig, m, SEED, ep, it, off, K, -10.0, 10.0)
    v64, v32 = mm.sample(*args, np.float64), mm.sample(*args, np.float32)
    tol = allowance(v32, v64)
    err = float(np.abs(vd - v64).max())
    print(f"\n{model} {integ} B={B} K={K} N={N}: sample |dev - f64| = {err:.3e}, f32 model floor = "
          f"{np.abs(v32 - v64).max():.3e}, allowance = {tol:.3e}, ratio dev/floor = {err / max(np.abs(v32 - v64).max(), 1e-30):.2f}")
    assert err <= tol
    assert np.array_equal(vd.reshape(B, K, N)[:, 0], un)  # sample 0 is the nominal, exactly
    assert np.array_equal(npy(x0r), np.repeat(npy(x0), K, axis=0))
    assert np.abs(vd).max() <= 10.0 and (np.abs(vd) == 10.0).any()  # the clamp is active somewhere

    costs_row = torch.empty(B, device="cuda")
    best_cost = torch.full((B,), float("inf"), device="cuda")
    best_u = torch.zeros(B, H, m, device="cuda")
    un2 = u.clone()
    eng.mppi_update(un2, v, s, lam, cost, costs_row=costs_row, best_cost=best_cost, best_u=best_u)
    sd = npy(s)
    assert np.all(np.isfinite(sd))
    r64, r32 = mm.update(un, vd, sd, lam, np.float64, -10.0, 10.0), mm.update(un, vd, sd, lam, np.float32, -10.0, 10.0)
    tol = allowance(r32["u"], r64["u"])
    err = float(np.abs(npy(un2).reshape(B, N) - r64["u"]).max())
    floor = float(np.abs(r32["u"] - r64["u"]).max())
    print(f"  update |dev - f64| = {err:.3e}, f32 model floor = {floor:.3e}, allowance = {tol:.3e}, ratio dev/floor = "
          f"{err / max(floor, 1e-30):.2f}")
    assert err <= tol
    assert np.array_equal(npy(costs_row), sd.reshape(B, K)[:, 0])
    assert np.array_equal(r64["kmin"], sd.reshape(B, K).argmin(axis=1))
    assert np.array_equal(npy(best_cost), sd.reshape(B, K).min(axis=1))
    assert np.array_equal(npy(best_u).reshape(B, N), vd.reshape(B, K, N)[np.arange(B), r64["kmin"]])
    # a second update with worse costs leaves the best alone; non-finite costs are ignored, all non-finite keeps u
    s2 = s.clone().reshape(B, K)
    s2[:, 1] = float("nan")
    s2[0, :] = float("inf")
    before = un2.clone()
    eng.mppi_update(un2, v, (s2 + 1.0).reshape(-1), lam, cost, best_cost=best_cost, best_u=best_u)
    assert np.array_equal(npy(best_cost), sd.reshape(B, K).min(axis=1))
    assert torch.equal(un2[0], before[0]) and bool(torch.isfinite(un2).all())


# ----------------------------------------------------------------------------- 8. one iteration against the float64 oracle
@pytest.mark.parametrize("model, integ, B, K, H", [("phnn_cartpole", "euler", 37, 64, 20),
                                                    ("canonical_cartpole", "rk4", 37, 30, 20),
                                                    ("odefunc_cartpole", "euler", 1, 64, 50),
                                                    ("phnn_m2_fix", "rk4", 37, 30, 25)])
def test_iterations_against_the_float64_oracle(torch, model, integ, B, K, H):
    eng = engine(model)
    m, N = eng.m, H * eng.m
    cost = make_cost(eng)
    o64 = ol.OracleModel(weights(model), "f64")
    x0 = torch.tensor(states(B, 3), device="cuda")
    u = torch.zeros(B, H, m, device="cuda")
    sig, lam = sigma_of(m), 25.0
    for it in range(3):
        un = npy(u).reshape(B, N).copy()  # the device's nominal: every iteration is checked from it
        v, x0r = eng.mppi_sample(x0, u, cost, K, sig, SEED, it)
        s = eng.rollout_cost(x0r, v, cost, integ, 0.02)
        eng.mppi_update(u, v, s, lam, cost)
        vd = npy(v).reshape(B * K, N)
        s64 = o64.rollout(npy(x0r), vd.reshape(B * K, H, m), cost, integ, 0.02, grad=False, traj=False, nthreads=8)["cost"]
        r64 = mm.update(un, vd, s64, lam, np.float64, -10.0, 10.0)
        r32 = mm.update(un, vd, npy(s), lam, np.float32, -10.0, 10.0)
        r64dev = mm.update(un, vd, npy(s), lam, np.float64, -10.0, 10.0)
        allow7 = ALLOW * np.abs(r32["u"] - r64dev["u"]).max(axis=1) + ulp(r64["u"])
        bound = 2 * 1e-5 * np.abs(s64.reshape(B, K)).max(axis=1) / lam * np.abs(vd.reshape(B, K, N)).max(axis=(1, 2)) + allow7
        err = np.abs(npy(u).reshape(B, N) - r64["u"]).max(axis=1)
        print(f"\n{model} {integ} it={it}: max |u_dev - u_64| = {err.max():.3e}, bound (min over problems) = "
              f"{bound.min():.3e}, worst err/bound = {(err / bound).max():.3f}, max |S_dev/S_64 - 1| = "
              f"{np.abs(npy(s) / s64 - 1).max():.2e}")
        assert np.all(err <= bound)


# ----------------------------------------------------------------------------- 9. bitwise
def same(torch, a, b):
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("model, integ, B, K, H", CASES)
def test_library_loop_equals_python_loop_and_repeats(torch, model, integ, B, K, H):
    from phnn_mpc_amd.solver import mppi_solve
    eng = engine(model)
    cost = make_cost(eng)
    x0 = torch.tensor(states(B, 4), device="cuda")
    u0 = torch.tensor(nominal(B, H, eng.m, 5), device="cuda")  # past the clamp in places
    kw = dict(iters=3, samples=K, lam=25.0, sigma=sigma_of(eng.m), seed=SEED, epoch=2, problem_offset=7)
    a = eng.solve_mppi(x0, u0, cost, integ, 0.02, **kw)
    b = mppi_solve(eng, x0, u0, cost, integ, 0.02, **kw)
    same(torch, a, b)
    same(torch, a, eng.solve_mppi(x0, u0, cost, integ, 0.02, **kw))
    assert bool((a["u_last"].abs() <= 10.0).all()) and bool(torch.isfinite(a["best_cost"]).all())
    assert bool((a["best_cost"] <= a["costs"].min(dim=0).values).all())
    for k2, v2 in (("seed", SEED + 1), ("epoch", 3)):
        c = eng.solve_mppi(x0, u0, cost, integ, 0.02, **{**kw, k2: v2})
        assert not torch.equal(a["u_last"], c["u_last"]), k2
    ep = torch.tensor([2], dtype=torch.int32, device="cuda")  # the epoch read from the device
    same(torch, a, eng.solve_mppi(x0, u0, cost, integ, 0.02, **{**kw, "epoch": ep}))


@pytest.mark.parametrize("B, K", [(37, 64), (4096, 30)])
def test_batch_equals_problems_solved_alone(torch, B, K):
    """B = 37, K = 64: 148 tiles, the split-tile K1; B = 4096, K = 30: 7680 tiles, the whole-tile K1; one problem alone:
    at most 4 tiles, split-tile."""
    eng = engine("phnn_cartpole")
    H, cost = 20, make_cost(eng)
    x0 = torch.tensor(states(B, 6), device="cuda")
    u0 = torch.tensor(nominal(B, H, 1, 7), device="cuda")
    kw = dict(iters=2, samples=K, lam=25.0, sigma=2.0, seed=SEED, epoch=5)
    full = eng.solve_mppi(x0, u0, cost, "euler", 0.02, problem_offset=100, **kw)
    alone = {k: torch.empty_like(v) for k, v in full.items()}
    ws = {}
    for b in range(B):
        one = eng.solve_mppi(x0[b:b + 1], u0[b:b + 1], cost, "euler", 0.02, problem_offset=100 + b, workspace=ws, **kw)
        for k in full:
            (alone[k][:, b:b + 1] if k == "costs" else alone[k][b:b + 1]).copy_(one[k])
    same(torch, full, alone)
    half = eng.solve_mppi(x0[B // 2:], u0[B // 2:], cost, "euler", 0.02, problem_offset=100 + B // 2, **kw)
    assert torch.equal(half["u_last"], full["u_last"][B // 2:]) and torch.equal(half["best_u"], full["best_u"][B // 2:])


def test_graph_equals_eager(torch):
    from phnn_mpc_amd.solver import GraphedMPPI, _mppi_eager, mppi_solver_for
    eng = engine("canonical_cartpole")
    cost = make_cost(eng)
    B, H, K = 37, 20, 30
    g = mppi_solver_for(eng, True)
    assert isinstance(g, GraphedMPPI) and mppi_solver_for(eng, True, g) is g and mppi_solver_for(eng, False) is _mppi_eager
    ep = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(iters=3, samples=K, lam=25.0, sigma=(2.0,), seed=SEED)
    for trial in range(3):  # the second and third calls replay the graph with new inputs and a new epoch
        x0 = torch.tensor(states(B, 8 + trial), device="cuda")
        u0 = torch.tensor(nominal(B, H, 1, 9 + trial), device="cuda")
        ep.fill_(trial)
        graph = g(eng, x0, u0, cost, "euler", 0.02, epoch=ep, **kw)
        same(torch, _mppi_eager(eng, x0, u0, cost, "euler", 0.02, epoch=trial, **kw), graph)
        captured = g.graph
    assert g.graph is captured


def test_per_problem_setpoints_equal_separate_solves(torch):
    eng = engine("phnn_cartpole")
    B, H, K = 5, 20, 30
    rng = np.random.default_rng(10)
    setp = (rng.uniform(-1, 1, size=(B, 1, 4)) * [0.5, 0.05, 0.0, 0.0]).astype(np.float32)
    x0 = torch.tensor(states(B, 11), device="cuda")
    u0 = torch.zeros(B, H, 1, device="cuda")
    kw = dict(iters=3, samples=K, lam=25.0, sigma=2.0, seed=SEED)
    tracked = eng.solve_mppi(x0, u0, make_cost(eng), "euler", 0.02, x_ref=torch.tensor(setp, device="cuda"), **kw)
    for b in range(B):
        one = eng.solve_mppi(x0[b:b + 1], u0[b:b + 1], make_cost(eng, x_target=setp[b, 0]), "euler", 0.02, problem_offset=b, **kw)
        assert torch.equal(one["u_last"][0], tracked["u_last"][b]) and torch.equal(one["best_cost"][0], tracked["best_cost"][b])
        assert torch.equal(one["costs"][:, 0], tracked["costs"][:, b])
    # one setpoint shared by all problems goes straight through (batch stride 0)
    shared = eng.solve_mppi(x0, u0, make_cost(eng), "euler", 0.02, x_ref=torch.tensor(setp[2, 0], device="cuda"), **kw)
    same(torch, shared, eng.solve_mppi(x0, u0, make_cost(eng, x_target=setp[2, 0]), "euler", 0.02, **kw))


def _load(cls, name, torch):
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights(name).items()})
    return m


def test_device_closed_loop_equals_host_loop(torch):
    """256 plants x 100 control steps: DeviceClosedLoop (graph and eager; the step counter is the noise epoch) == the
    run_mpc_batch host loop (the loop index is): controls bit for bit, states to 1e-12 (the closed-loop contract)."""
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(optimizer="MPPI", samples=32, lam=20.0, sigma=3.0, seed=SEED, optimizer_steps=2)
    rng = np.random.default_rng(12)
    X = rng.uniform(-1, 1, size=(256, 4)) * [0.2, 0.08, 0.1, 0.1]
    T = 100
    for c in (create_mpc_from_config(_load(pHNN, "phnn_cartpole", torch), cfg),
              create_mpc_controller(_load(pHNN_Canonical, "canonical_cartpole", torch), cfg)):
        host = run_mpc_batch(BatchedCartPole(0.02), c, X, T)
        assert len(np.unique(host["controls"][:, 0, 0])) > T // 4  # fresh noise at every step
        for use_graph in (False, True):
            dev = run_mpc_batch_device(c, X, T, use_graph=use_graph)
            assert np.array_equal(dev["controls"], host["controls"])
            assert np.allclose(dev["states"], host["states"], rtol=0, atol=1e-12)
            assert np.array_equal(dev["done_step"], host["done_step"])
    # the controller's own graph switch: same controls, one capture for all epochs
    c = create_mpc_from_config(_load(pHNN, "phnn_cartpole", torch), cfg)
    eager = [c.compute_control_batch(X[:8].astype(np.float32), epoch=e) for e in range(3)]
    c.use_graph = True
    for e in range(3):
        assert np.array_equal(eager[e], c.compute_control_batch(X[:8].astype(np.float32), epoch=e))
        captured = c._graphed_mppi.graph if e == 0 else captured
    assert c._graphed_mppi.graph is captured


# ----------------------------------------------------------------------------- 10. the saturated start, iters = 0, errors
def test_saturated_start_on_the_device(torch):
    """tests/test_mppi_model.py::test_saturated_start_adam_is_stuck_mppi_is_not on the device (same case, same
    parameters): Adam's last iterate is u_init bit for bit, MPPI's best_cost is strictly below cost(clamp(u_init))."""
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    c = create_mpc_from_config(_load(pHNN, "phnn_cartpole", torch), yaml.safe_load(open(CFG)))
    eng, cost = c.engine, c._cost()
    u_init, adam, mppi, c_sat = saturated_case(eng, cost)
    assert torch.equal(adam["u_last"], u_init)
    print("\ncost(clamp(u_init)) = %.6e, MPPI best_cost = %.6e, nominal costs %s" % (
        float(c_sat), float(mppi["best_cost"]), mppi["costs"][:, 0].tolist()))
    assert float(mppi["costs"][0, 0]) == float(c_sat)
    assert float(mppi["best_cost"]) < float(c_sat)
    same(torch, mppi, eng.solve_mppi(torch.tensor(X0[None], device="cuda"), u_init, cost, "euler", 0.02, seed=SEED, **SAT))
    # iters = 0: nothing uninitialised comes back
    out = eng.solve_mppi(torch.tensor(X0[None], device="cuda"), u_init, cost, "euler", 0.02, seed=SEED, **{**SAT, "iters": 0})
    assert bool(torch.isinf(out["best_cost"]).all()) and bool((out["best_cost"] > 0).all()) and bool((out["best_u"] == 0).all())
    assert torch.equal(out["u_last"], torch.clamp(u_init, -15.0, 15.0)) and out["costs"].shape == (0, 1)


def test_argument_errors_and_limits(torch):
    from phnn_mpc_amd.engine import PhnnError
    eng = engine("phnn_cartpole")
    cost = make_cost(eng)
    x0 = torch.tensor(states(2, 13), device="cuda")
    u0 = torch.zeros(2, 20, 1, device="cuda")
    ok = dict(iters=1, samples=4, lam=1.0, sigma=1.0, seed=0)
    for bad in (dict(samples=1), dict(lam=0.0), dict(lam=float("inf")), dict(lam=float("nan")), dict(sigma=-1.0),
                dict(sigma=float("inf")), dict(iters=-1), dict(problem_offset=-1), dict(problem_offset=2 ** 48)):
        with pytest.raises(PhnnError, match="error -1"):
            eng.solve_mppi(x0, u0, cost, "euler", 0.02, **{**ok, **bad})
    with pytest.raises(PhnnError, match="error -2"):  # H * m > 256
        eng.solve_mppi(x0, torch.zeros(2, 257, 1, device="cuda"), cost, "euler", 0.02, **ok)
    with pytest.raises(ValueError):
        eng.solve_mppi(x0, u0, cost, "euler", 0.02, **{**ok, "sigma": (1.0, 2.0)})
    assert eng.mppi_workspace_bytes(2, 20, 1) == 0
    a256 = lambda x: (x + 255) // 256 * 256
    assert eng.mppi_workspace_bytes(3, 21, 5) == a256(4 * 15 * 21) + a256(4 * 15 * 4) + a256(4 * 15)
    # a too small workspace is refused by the library
    import ctypes as C
    from phnn_mpc_amd import _capi
    opt, _ = eng._mppi_options(1, 4, 1.0, 1.0, 0, 0, 0)
    buf = torch.empty(256, dtype=torch.uint8, device="cuda")
    bc, bu = torch.empty(2, device="cuda"), torch.empty(2, 20, 1, device="cuda")
    rc = eng.lib.phnn_solve_mppi(eng.h, x0.data_ptr(), u0.clone().data_ptr(), 2, 20, C.byref(cost), None, 0, 0.02, C.byref(opt),
                                 buf.data_ptr(), buf.numel(), None, bc.data_ptr(), bu.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == -1 and b"workspace" in eng.lib.phnn_last_error(eng.h)
    assert eng.lib.phnn_version() >= 250
    B0 = eng.solve_mppi(x0[:0], u0[:0], cost, "euler", 0.02, **ok)  # an empty batch
    assert B0["u_last"].shape == (0, 20, 1) and B0["best_cost"].shape == (0,)
