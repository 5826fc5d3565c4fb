"""The CEM solve on the device (engine.cem_sample / cem_update / solve_cem, kernels k_sample and k_cem_update).

  update      k_cem_update has no transcendental: its mean, sigma, best sample and cost record must equal the float32
              form of tests/cem_model.py BIT FOR BIT -- on the device's own samples and K1 costs for every shape, and on
              the synthetic edge costs of tests/test_cem_model.py (ties across the elite boundary, -0 / +0, non-finite
              costs, fewer finite costs than E, none) uploaded as they are.
  sample      k_sample vs the float64 model with test_gpu_mppi's allowance (device log / sqrt / sincospi are not
              bit-specified): 8 x the float32 form's distance from the float64 form + one ulp.
  bitwise     solve_cem == solver.cem_solve over the primitives; repeat == first; B problems at once == each alone with
              its problem_offset (B = 37: split-tile K1, B = 300 x K = 30: 563 tiles, whole-tile K1); graph == eager;
              seed / epoch change the samples; per-problem x_ref == separate solves; the device closed loop == the host
              loop.
  saturated   u_init = 2 u_max: Adam returns u_init bit for bit, CEM's final mean and best sample end strictly below
              cost(clamp(u_init)); iters = 0 returns best_cost = +inf, best_u = 0, u_last = clamp(u_init), sigma_init.
Shapes: test_gpu_mppi's, its B = 4096 case replaced by B = 300, K = 30: every k_cem_update width (1 .. 4 float4 per
lane), every N = H*m mod 4, K = 2 / 30 / 64 (15 and 17 in the synthetic test).
"""
import numpy as np
import pytest
import yaml

import cem_model as cm
import oracle_lib as ol
from test_cem_model import CFG, SAT, SEED, X0, saturated_case, synthetic_costs
from test_gpu_mppi import allowance, engine, make_cost, nominal, npy, states

pytestmark = pytest.mark.gpu

# (model, integrator, B, K, H): N = H*m -> (float4 per lane, N mod 4) = 20:(1,0) 77:(2,1) 150:(3,2) 255:(4,3) 50:(1,2)
CASES = [("phnn_cartpole", "euler", 37, 64, 20), ("phnn_cartpole", "rk4", 1, 30, 77),
         ("canonical_cartpole", "euler", 37, 30, 150), ("odefunc_cartpole", "rk4", 37, 2, 255),
         ("phnn_m2_fix", "euler", 37, 64, 25), ("phnn_cartpole", "euler", 300, 30, 20)]
REFITS = [(0.0, 0.0), (0.25, 0.05)]  # (alpha, sigma_min)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def spread(B, N, seed):
    """A per-element standard deviation in [0, 3], about one entry in eight exactly 0."""
    rng = np.random.default_rng(seed)
    sig = rng.uniform(0, 3, size=(B, N)).astype(np.float32)
    sig[rng.uniform(size=(B, N)) < 0.125] = 0.0
    return sig


def on_device(torch, a, misalign=False):
    """a -> contiguous float32 device tensor; misalign: its base 4 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if not misalign:
        return torch.tensor(a, device="cuda")
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.tensor(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def check_update(torch, eng, cost, u, sig, v, s, E, alpha, smin, misalign=False, lim=10.0, tag="", bits=bits):
    """One k_cem_update launch on numpy inputs against the float32 model, everything as bits (`bits`: float32 array ->
    uint32; a caller that feeds NaN inputs passes one that gives every NaN one pattern, a NaN's sign and payload being no
    part of the model)."""
    B, N = u.shape
    H = N // eng.m
    K = s.size // B
    shape = (B, H, eng.m)
    ud, sd = on_device(torch, u.reshape(shape), misalign), on_device(torch, sig.reshape(shape), misalign)
    vd, cd = on_device(torch, v.reshape(B * K, H, eng.m)), on_device(torch, s.reshape(-1))
    costs_row = torch.full((B,), -7.0, device="cuda")
    prev = np.where(np.arange(B) % 3 == 2, np.float32(-1e30), np.float32(np.inf)).astype(np.float32)  # some cannot be beaten
    best_cost = on_device(torch, prev)
    best_u = torch.zeros(shape, device="cuda")
    eng.cem_update(ud, sd, vd, cd, E, alpha, smin, cost, costs_row=costs_row, best_cost=best_cost, best_u=best_u)
    want = cm.update(u, sig, v, s, E, alpha, smin, np.float32, -lim, lim)
    wc, wu = prev.copy(), np.zeros((B, N), np.float32)
    cm.track_best(wc, wu, v, want)
    got_u, got_sig = npy(ud).reshape(B, N), npy(sd).reshape(B, N)
    assert np.array_equal(bits(got_u), bits(want["u"])), (tag, "mean", float(np.abs(got_u - want["u"]).max()))
    assert np.array_equal(bits(got_sig), bits(want["sig"])), (tag, "sigma", float(np.abs(got_sig - want["sig"]).max()))
    assert np.array_equal(bits(npy(costs_row)), bits(s.reshape(B, K)[:, 0])), tag
    assert np.array_equal(bits(npy(best_cost)), bits(wc)), tag
    assert np.array_equal(bits(npy(best_u).reshape(B, N)), bits(wu)), tag
    return want


# ----------------------------------------------------------------------------- 1. k_cem_update, bit for bit
@pytest.mark.parametrize("model, integ, B, K, H", CASES)
def test_update_equals_the_float32_model_on_device_samples(torch, model, integ, B, K, H):
    eng = engine(model)
    m, N = eng.m, H * eng.m
    cost = make_cost(eng)
    x0 = torch.tensor(states(B, 1), device="cuda")
    u = np.clip(nominal(B, H, m, 2), -10, 10).reshape(B, N)
    sig = spread(B, N, 3)
    v, x0r = eng.cem_sample(x0, on_device(torch, u.reshape(B, H, m)), on_device(torch, sig.reshape(B, H, m)), cost, K, SEED, 2,
                            epoch=11, problem_offset=1000)
    s = npy(eng.rollout_cost(x0r, v, cost, integ, 0.02))
    vd = npy(v).reshape(B * K, N)
    assert np.all(np.isfinite(s))
    for E in sorted({1, min(8, K), K}):
        for alpha, smin in REFITS:
            for misalign in ((False, True) if N % 4 == 0 and B <= 37 else (False,)):
                r = check_update(torch, eng, cost, u, sig, vd, s, E, alpha, smin, misalign, tag=(E, alpha, smin, misalign))
                assert np.all(r["n_elite"] == E)
    if K >= 8:  # costs of one problem made non-finite: kept bit for bit, and the others do not notice
        s2 = s.copy().reshape(B, K)
        s2[0, :] = np.nan
        s2[B - 1, 1::2] = np.inf
        check_update(torch, eng, cost, u, sig, vd, s2.reshape(-1), min(8, K), 0.25, 0.05, tag="non-finite rows")


@pytest.mark.parametrize("K", [2, 15, 17, 30, 64])
def test_update_equals_the_float32_model_on_synthetic_costs(torch, K):
    """The edge inputs of tests/test_cem_model.py::synthetic_costs as three problems each (the costs as given, reversed,
    and rotated by one), N = 20 (16-byte rows, aligned and misaligned bases) and N = 255 (four float4 per lane, ragged)."""
    rng = np.random.default_rng(K)
    for model, H in (("phnn_cartpole", 20), ("odefunc_cartpole", 255)):
        eng = engine(model)
        cost = make_cost(eng)
        N = H * eng.m
        for name, (s1, E) in synthetic_costs(K).items():
            s = np.stack([s1, s1[::-1], np.roll(s1, 1)]).astype(np.float32)
            u = rng.uniform(-10, 10, size=(3, N)).astype(np.float32)
            sig = spread(3, N, K + 1)
            v = rng.uniform(-10, 10, size=(3 * K, N)).astype(np.float32)
            for alpha, smin in REFITS:
                for misalign in ((False, True) if N % 4 == 0 else (False,)):
                    r = check_update(torch, eng, cost, u, sig, v, s.reshape(-1), E, alpha, smin, misalign,
                                     tag=(name, K, N, alpha, misalign))
            fin = np.isfinite(s).sum(axis=1)
            assert np.array_equal(r["n_elite"], np.minimum(E, fin))
            for b in range(3):  # the model's elites are the rule's (the CPU test pins the rule itself)
                assert sorted(cm.elite_order(s[b], E)) == list(np.nonzero(r["elite"][b])[0])


# ----------------------------------------------------------------------------- 2. k_sample against the float64 model
@pytest.mark.parametrize("model, integ, B, K, H", CASES)
def test_sample_against_the_float64_model(torch, model, integ, B, K, H):
    eng = engine(model)
    m, N = eng.m, H * eng.m
    cost = make_cost(eng)
    x0 = torch.tensor(states(B, 1), device="cuda")
    u = np.clip(nominal(B, H, m, 2), -10, 10).reshape(B, N)
    sig = spread(B, N, 3)
    it, ep, off = 3, 11, 1000
    for misalign in ((False, True) if N % 4 == 0 and B <= 37 else (False,)):
        v, x0r = eng.cem_sample(x0, on_device(torch, u.reshape(B, H, m), misalign), on_device(torch, sig.reshape(B, H, m), misalign),
                                cost, K, SEED, it, epoch=ep, problem_offset=off)
        vd = npy(v).reshape(B * K, N)
        args = (u, sig, SEED, ep, it, off, K, -10.0, 10.0)
        v64, v32 = cm.sample(*args, np.float64), cm.sample(*args, np.float32)
        tol = allowance(v32, v64)
        err = float(np.abs(vd - v64).max())
        print(f"\n{model} {integ} B={B} K={K} N={N}: sample |dev - f64| = {err:.3e}, f32 model floor = "
              f"{np.abs(v32 - v64).max():.3e}, allowance = {tol:.3e}")
        assert err <= tol
        assert np.array_equal(bits(vd.reshape(B, K, N)[:, 0]), bits(u))  # sample 0 is the mean, exactly
        assert np.array_equal(npy(x0r), np.repeat(npy(x0), K, axis=0))
        assert np.abs(vd).max() <= 10.0 and (np.abs(vd) == 10.0).any()  # the clamp is active somewhere
        z = np.broadcast_to((sig == 0)[:, None, :], (B, K, N))  # no noise where sigma is 0
        assert z.any() and np.array_equal(vd.reshape(B, K, N)[z], np.broadcast_to(u[:, None, :], (B, K, N))[z])


# ----------------------------------------------------------------------------- 3. bitwise
def same(torch, a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), k


def options(K, **kw):
    return dict(dict(iters=3, samples=K, elites=min(8, K), alpha=0.25, sigma=2.0, sigma_min=0.05, seed=SEED), **kw)


@pytest.mark.parametrize("model, integ, B, K, H", CASES)
def test_library_loop_equals_python_loop_and_repeats(torch, model, integ, B, K, H):
    from phnn_mpc_amd.solver import cem_solve
    eng = engine(model)
    cost = make_cost(eng)
    x0 = torch.tensor(states(B, 4), device="cuda")
    u0 = torch.tensor(nominal(B, H, eng.m, 5), device="cuda")  # past the clamp in places
    kw = options(K, sigma=tuple(2.0 + 0.5 * i for i in range(eng.m)), epoch=2, problem_offset=7)
    a = eng.solve_cem(x0, u0, cost, integ, 0.02, **kw)
    b = cem_solve(eng, x0, u0, cost, integ, 0.02, **kw)
    same(torch, a, b)
    same(torch, a, eng.solve_cem(x0, u0, cost, integ, 0.02, **kw))
    assert bool((a["u_last"].abs() <= 10.0).all()) and bool(torch.isfinite(a["best_cost"]).all())
    assert bool((a["best_cost"] <= a["costs"].min(dim=0).values).all())
    assert bool((a["sigma_last"] >= np.float32(0.05)).all()) and bool(torch.isfinite(a["sigma_last"]).all())
    for k2, v2 in (("seed", SEED + 1), ("epoch", 3)):
        c = eng.solve_cem(x0, u0, cost, integ, 0.02, **{**kw, k2: v2})
        assert not torch.equal(a["u_last"], c["u_last"]), k2
    ep = torch.tensor([2], dtype=torch.int32, device="cuda")  # the epoch read from the device
    same(torch, a, eng.solve_cem(x0, u0, cost, integ, 0.02, **{**kw, "epoch": ep}))


@pytest.mark.parametrize("B, K", [(37, 64), (300, 30)])
def test_batch_equals_problems_solved_alone(torch, B, K):
    """B = 37, K = 64: 148 tiles, the split-tile K1; B = 300, K = 30: 563 tiles, the whole-tile K1; one problem alone:
    at most 4 tiles, split-tile."""
    eng = engine("phnn_cartpole")
    H, cost = 20, make_cost(eng)
    x0 = torch.tensor(states(B, 6), device="cuda")
    u0 = torch.tensor(nominal(B, H, 1, 7), device="cuda")
    kw = options(K, iters=2, epoch=5)
    full = eng.solve_cem(x0, u0, cost, "euler", 0.02, problem_offset=100, **kw)
    alone = {k: torch.empty_like(v) for k, v in full.items()}
    ws = {}
    for b in range(B):
        one = eng.solve_cem(x0[b:b + 1], u0[b:b + 1], cost, "euler", 0.02, problem_offset=100 + b, workspace=ws, **kw)
        for k in full:
            (alone[k][:, b:b + 1] if k == "costs" else alone[k][b:b + 1]).copy_(one[k])
    same(torch, full, alone)
    half = eng.solve_cem(x0[B // 2:], u0[B // 2:], cost, "euler", 0.02, problem_offset=100 + B // 2, **kw)
    assert torch.equal(half["u_last"], full["u_last"][B // 2:]) and torch.equal(half["sigma_last"], full["sigma_last"][B // 2:])


def test_graph_equals_eager(torch):
    from phnn_mpc_amd.solver import GraphedCEM, _cem_eager, cem_solver_for
    eng = engine("canonical_cartpole")
    cost = make_cost(eng)
    B, H, K = 37, 20, 30
    g = cem_solver_for(eng, True)
    assert isinstance(g, GraphedCEM) and cem_solver_for(eng, True, g) is g and cem_solver_for(eng, False) is _cem_eager
    ep = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = options(K, sigma=(2.0,))
    for trial in range(3):  # the second and third calls replay the graph with new inputs and a new epoch
        x0 = torch.tensor(states(B, 8 + trial), device="cuda")
        u0 = torch.tensor(nominal(B, H, 1, 9 + trial), device="cuda")
        ep.fill_(trial)
        graph = g(eng, x0, u0, cost, "euler", 0.02, epoch=ep, **kw)
        same(torch, _cem_eager(eng, x0, u0, cost, "euler", 0.02, epoch=trial, **kw), graph)
        captured = g.graph
    assert g.graph is captured


def test_per_problem_setpoints_equal_separate_solves(torch):
    eng = engine("phnn_cartpole")
    B, H, K = 5, 20, 30
    rng = np.random.default_rng(10)
    setp = (rng.uniform(-1, 1, size=(B, 1, 4)) * [0.5, 0.05, 0.0, 0.0]).astype(np.float32)
    x0 = torch.tensor(states(B, 11), device="cuda")
    u0 = torch.zeros(B, H, 1, device="cuda")
    kw = options(K)
    tracked = eng.solve_cem(x0, u0, make_cost(eng), "euler", 0.02, x_ref=torch.tensor(setp, device="cuda"), **kw)
    for b in range(B):
        one = eng.solve_cem(x0[b:b + 1], u0[b:b + 1], make_cost(eng, x_target=setp[b, 0]), "euler", 0.02, problem_offset=b, **kw)
        assert torch.equal(one["u_last"][0], tracked["u_last"][b]) and torch.equal(one["best_cost"][0], tracked["best_cost"][b])
        assert torch.equal(one["costs"][:, 0], tracked["costs"][:, b]) and torch.equal(one["sigma_last"][0], tracked["sigma_last"][b])
    # one setpoint shared by all problems goes straight through (batch stride 0)
    shared = eng.solve_cem(x0, u0, make_cost(eng), "euler", 0.02, x_ref=torch.tensor(setp[2, 0], device="cuda"), **kw)
    same(torch, shared, eng.solve_cem(x0, u0, make_cost(eng, x_target=setp[2, 0]), "euler", 0.02, **kw))


def _load(cls, name, torch):
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights(name).items()})
    return m


def test_device_closed_loop_equals_host_loop(torch):
    """256 plants x 30 control steps: DeviceClosedLoop (graph and eager; the step counter is the noise epoch) == the
    run_mpc_batch host loop (the loop index is): controls bit for bit, states to 1e-12 (the closed-loop contract)."""
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(optimizer="CrossEntropy", samples=32, elites=6, alpha=0.25, sigma=3.0, sigma_min=0.05, seed=SEED,
                      optimizer_steps=2)
    rng = np.random.default_rng(12)
    X = rng.uniform(-1, 1, size=(256, 4)) * [0.2, 0.08, 0.1, 0.1]
    T = 30
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
        captured = c._graphed_cem.graph if e == 0 else captured
    assert c._graphed_cem.graph is captured


# ----------------------------------------------------------------------------- 4. the saturated start, iters = 0, errors
def test_saturated_start_on_the_device(torch):
    """tests/test_cem_model.py::test_saturated_start_adam_is_stuck_cem_is_not on the device (same case, same parameters)."""
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    c = create_mpc_from_config(_load(pHNN, "phnn_cartpole", torch), yaml.safe_load(open(CFG)))
    eng, cost = c.engine, c._cost()
    u_init, adam, cem, c_sat, c_mean = saturated_case(eng, cost)
    assert torch.equal(adam["u_last"], u_init)
    print("\ncost(clamp(u_init)) = %.6e, CEM final mean = %.6e, best_cost = %.6e, mean costs %s, sigma %.3f .. %.3f" % (
        float(c_sat), float(c_mean), float(cem["best_cost"]), cem["costs"][:, 0].tolist(), float(cem["sigma_last"].min()),
        float(cem["sigma_last"].max())))
    assert float(cem["costs"][0, 0]) == float(c_sat)
    assert float(c_mean) < float(c_sat) and float(cem["best_cost"]) < float(c_sat)
    x0 = torch.tensor(X0[None], device="cuda")
    same(torch, cem, eng.solve_cem(x0, u_init, cost, "euler", 0.02, seed=SEED, **SAT))
    # iters = 0: nothing uninitialised comes back
    out = eng.solve_cem(x0, u_init, cost, "euler", 0.02, seed=SEED, **{**SAT, "iters": 0})
    assert bool(torch.isinf(out["best_cost"]).all()) and bool((out["best_cost"] > 0).all()) and bool((out["best_u"] == 0).all())
    assert torch.equal(out["u_last"], torch.clamp(u_init, -15.0, 15.0)) and out["costs"].shape == (0, 1)
    assert bool((out["sigma_last"] == 5.0).all())


def test_argument_errors_and_limits(torch):
    from phnn_mpc_amd.engine import PhnnError
    eng = engine("phnn_cartpole")
    cost = make_cost(eng)
    x0 = torch.tensor(states(2, 13), device="cuda")
    u0 = torch.zeros(2, 20, 1, device="cuda")
    ok = dict(iters=1, samples=4, elites=2, alpha=0.25, sigma=1.0, sigma_min=0.05, seed=0)
    for bad in (dict(samples=1, elites=1), dict(elites=0), dict(elites=5), dict(alpha=-0.1), dict(alpha=1.0),
                dict(alpha=float("nan")), dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma_min=-1.0),
                dict(sigma_min=float("inf")), dict(iters=-1), dict(problem_offset=-1), dict(problem_offset=2 ** 48)):
        with pytest.raises(PhnnError, match="error -1"):
            eng.solve_cem(x0, u0, cost, "euler", 0.02, **{**ok, **bad})
    with pytest.raises(PhnnError, match="error -2"):  # H * m > 256
        eng.solve_cem(x0, torch.zeros(2, 257, 1, device="cuda"), cost, "euler", 0.02, **ok)
    with pytest.raises(ValueError):
        eng.solve_cem(x0, u0, cost, "euler", 0.02, **{**ok, "sigma": (1.0, 2.0)})
    assert eng.cem_workspace_bytes(2, 20, 1) == 0
    a256 = lambda x: (x + 255) // 256 * 256
    assert eng.cem_workspace_bytes(3, 21, 5) == a256(4 * 15 * 21) + a256(4 * 15 * 4) + a256(4 * 15) + a256(4 * 3 * 21)
    assert eng.cem_workspace_bytes(3, 21, 5) == eng.mppi_workspace_bytes(3, 21, 5) + a256(4 * 3 * 21)
    # a too small workspace is refused by the library
    import ctypes as C
    opt, _ = eng._cem_options(1, 4, 2, 0.25, 1.0, 0.05, 0, 0, 0)
    buf = torch.empty(eng.mppi_workspace_bytes(2, 20, 4), dtype=torch.uint8, device="cuda")  # the sigma region is missing
    bc, bu = torch.empty(2, device="cuda"), torch.empty(2, 20, 1, device="cuda")
    rc = eng.lib.phnn_solve_cem(eng.h, x0.data_ptr(), u0.clone().data_ptr(), 2, 20, C.byref(cost), None, 0, 0.02, C.byref(opt),
                                buf.data_ptr(), buf.numel(), None, bc.data_ptr(), bu.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == -1 and b"workspace" in eng.lib.phnn_last_error(eng.h)
    assert eng.lib.phnn_version() >= 260
    B0 = eng.solve_cem(x0[:0], u0[:0], cost, "euler", 0.02, **ok)  # an empty batch
    assert B0["u_last"].shape == (0, 20, 1) and B0["best_cost"].shape == (0,) and B0["sigma_last"].shape == (0, 20, 1)
