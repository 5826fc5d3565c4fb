"""CPU tests of the CEM solve: the NumPy restatement of its kernels (tests/cem_model.py: the elite rule, the refit, the
sampling on top of mppi_model's noise) and the host logic (solver.cem_solve, both controllers, the closed loop) on the
CPU oracle engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import yaml

import cem_model as cm
import oracle_lib as ol
from phnn_mpc_amd import _capi
from phnn_mpc_amd.models import pHNN, pHNN_Canonical
from phnn_mpc_amd.mpc_controller import MPCController, create_mpc_from_config
from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
from phnn_mpc_amd.solver import cem_solve, shooting_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
SEED = 0x5EED2026C0FFEE  # the seed of the MPPI tests
X0 = np.array([0.0, 0.1, 0.0, 0.0], np.float32)
KS = (2, 15, 17, 64)


# ----------------------------------------------------------------------------- 1. the elite rule on synthetic costs
def synthetic_costs(K, seed=0):
    """-> {name: (s (K,) float32, E)}: the edge inputs of the elite rule at K samples (tests/test_gpu_cem.py uploads the
    same ones).  'ties' / 'zeros' put equal costs on both sides of the elite boundary."""
    rng = np.random.default_rng(1000 * seed + K)
    base = rng.uniform(-50, 50, size=K).astype(np.float32)  # negative costs included
    out = {"one": (base.copy(), 1), "all": (base.copy(), K), "some": (base.copy(), min(8, K))}
    few = np.full(K, np.nan, np.float32)
    few[[K - 1, 0][: min(2, K - 1)]] = [3.0, -1.0][: min(2, K - 1)]
    out["fewer_finite_than_E"] = (few, K)
    bad = base.copy()
    bad[0], bad[K // 2], bad[K - 1] = np.nan, np.inf, -np.inf
    out["nonfinite_excluded"] = (bad, min(8, K)) if K > 3 else (np.array([-np.inf, 2.0], np.float32), 1)
    none = np.array([np.nan, np.inf, -np.inf] * K, np.float32)[:K]
    out["none_finite"] = (none, min(8, K))
    ties = base.copy()
    tied = np.arange(K)[:: max(K // 5, 1)][::-1][: max(2, min(5, K))]  # several k share the median cost
    ties[tied] = np.float32(np.median(base))
    nb = int((ties < ties[tied[0]]).sum())
    out["ties_across_the_boundary"] = (ties, min(nb + max(len(tied) // 2, 1), K))
    zeros = np.abs(base) + np.float32(1.0)
    zeros[::2] = np.float32(-0.0) if K > 2 else np.float32(0.0)
    zeros[0] = np.float32(0.0)
    if K > 2:
        zeros[2] = np.float32(0.0)
    zeros[K - 1] = np.float32(-0.0)
    out["zeros"] = (zeros, 1 if K == 2 else 2)
    out["negative"] = (-np.abs(base) - np.float32(1.0), min(3, K))
    return out


def brute_force_elites(s, E):
    """The rule read literally: repeatedly take the finite cost that is lowest, lowest k among equals."""
    left = [k for k in range(len(s)) if np.isfinite(s[k])]
    taken = []
    while left and len(taken) < E:
        best = left[0]
        for k in left[1:]:
            if s[k] < s[best]:  # float comparison: -0 < +0 is false
                best = k
        taken.append(best)
        left.remove(best)
    return taken


@pytest.mark.parametrize("K", KS)
def test_elite_rule_on_synthetic_costs(K):
    cases = synthetic_costs(K)
    for name, (s, E) in cases.items():
        want = brute_force_elites(s, E)
        assert list(cm.elite_order(s, E)) == want, name
        assert list(cm.descent_order(s, E)) == sorted(want), name  # the kernel's method picks the same set
        fin = np.isfinite(s)
        assert len(want) == min(E, int(fin.sum())) and all(fin[k] for k in want), name
    s, _ = cases["one"]
    assert cm.elite_order(s, 1)[0] == int(np.argmin(s))
    assert sorted(cm.elite_order(s, K)) == list(range(K))
    s, E = cases["fewer_finite_than_E"]
    assert len(cm.elite_order(s, E)) == int(np.isfinite(s).sum()) < E
    s, E = cases["none_finite"]
    assert len(cm.elite_order(s, E)) == 0 and len(cm.descent_order(s, E)) == 0
    s, E = cases["ties_across_the_boundary"]
    c = np.sort(s)[E - 1]
    tied = np.nonzero(s == c)[0]
    got = np.array(sorted(cm.elite_order(s, E)))
    n_in = int(np.isin(tied, got).sum())
    assert 0 < n_in < len(tied) and np.array_equal(tied[:n_in], got[np.isin(got, tied)]), "lowest k wins"
    s, E = cases["zeros"]
    assert cm.elite_order(s, 1)[0] == 0 and np.signbit(s[K - 1])  # +0 at k = 0 is not beaten by a later -0
    assert list(cm.elite_order(s, E)) == [0, 1 if K == 2 else 2][:E]
    # keys order as the floats do
    x = np.array([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf, np.nan], np.float32)
    k = cm.cost_keys(x).astype(np.int64)
    assert np.all(np.diff(k[1:9]) >= 0) and k[4] == k[5] and np.all(np.diff(k[[1, 2, 3, 4, 6, 7, 8]]) > 0)
    assert k[0] == k[9] == k[10] == int(cm.NO_KEY) > k[8]


# ----------------------------------------------------------------------------- 2. the refit
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refit_restatement(dtype):
    rng = np.random.default_rng(3)
    B, K, N = 5, 17, 23
    u = rng.uniform(-5, 5, size=(B, N)).astype(np.float32)
    sig = rng.uniform(0.5, 3, size=(B, N)).astype(np.float32)
    v = rng.uniform(-15, 15, size=(B * K, N)).astype(np.float32)
    s = rng.uniform(-10, 50, size=B * K).astype(np.float32)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    # E = K, alpha = 0: the plain mean and population standard deviation of the samples
    r = cm.update(u, sig, v, s, K, 0.0, 0.0, dtype)
    v3 = v.reshape(B, K, N).astype(np.float64)
    assert np.allclose(r["u"], v3.mean(axis=1), atol=tol) and np.allclose(r["sig"], v3.std(axis=1), atol=tol)
    assert r["u"].dtype == dtype and r["sig"].dtype == dtype and np.all(r["n_elite"] == K)
    # E = 1, alpha = 0: that sample, sigma = sigma_min
    r = cm.update(u, sig, v, s, 1, 0.0, 0.05, dtype)
    km = s.reshape(B, K).argmin(axis=1)
    assert np.array_equal(r["kmin"], km) and np.array_equal(r["beta"], s.reshape(B, K).min(axis=1))
    assert np.array_equal(r["u"].astype(np.float32), v.reshape(B, K, N)[np.arange(B), km])
    assert np.all(r["sig"] == dtype(np.float32(0.05)))
    # identical elites, 2 of them (x + x and its half are exact): the variance is exactly zero and sigma_min = 0 is
    # reached; 7 of them: the running sum rounds, the mean is off by an ulp, the variance tiny and never negative
    same = np.repeat(rng.uniform(-15, 15, size=(B, 1, N)).astype(np.float32), K, axis=1).reshape(B * K, N)
    r = cm.update(u, sig, same, s, 2, 0.0, 0.0, dtype)
    assert np.all(r["sig"] == 0) and np.array_equal(r["u"].astype(np.float32), same.reshape(B, K, N)[:, 0])
    r = cm.update(u, sig, same, s, 7, 0.0, 0.0, dtype)
    assert np.all(r["sig"] >= 0) and np.all(r["sig"] <= 2e-6)
    # smoothing and the clamp
    r0, ra = cm.update(u, sig, v, s, 6, 0.0, 0.0, dtype), cm.update(u, sig, v, s, 6, 0.25, 0.0, dtype, -4.0, 4.0)
    a = np.float64(np.float32(0.25))
    assert np.allclose(ra["u"], np.clip(a * u + (1 - a) * r0["u"], -4, 4), atol=tol)
    assert np.allclose(ra["sig"], np.sqrt(a * sig.astype(np.float64) ** 2 + (1 - a) * r0["sig"].astype(np.float64) ** 2), atol=tol)
    assert np.abs(ra["u"]).max() == 4.0
    # non-finite costs never take part; a problem without a finite cost keeps its state bit for bit
    s2 = s.copy().reshape(B, K)
    s2[:, 3], s2[:, 5], s2[:, 8] = np.nan, np.inf, -np.inf
    s2[4] = np.nan
    r2 = cm.update(u, sig, v, s2.ravel(), K, 0.25, 0.05, dtype)
    assert not r2["elite"][:, [3, 5, 8]].any() and np.all(r2["n_elite"][:4] == K - 3) and r2["n_elite"][4] == 0
    assert np.array_equal(r2["u"][4], u[4].astype(dtype)) and np.array_equal(r2["sig"][4], sig[4].astype(dtype))
    assert r2["kmin"][4] == -1 and np.isinf(r2["beta"][4]) and np.all(np.isfinite(r2["u"])) and np.all(np.isfinite(r2["sig"]))
    bc, bu = np.full(B, np.inf, np.float32), np.zeros((B, N), np.float32)
    cm.track_best(bc, bu, v, r2)
    assert np.isinf(bc[4]) and np.all(bu[4] == 0) and np.all(np.isfinite(bc[:4]))


def test_float32_form_stays_next_to_the_float64_form():
    """sigma in [0.5, 3], |v| <= 15: the two forms agree to 2e-6 (measured 5.7e-7 on the mean, 2.9e-7 on sigma)."""
    rng = np.random.default_rng(2)
    B, K, N = 7, 64, 50
    u = rng.uniform(-5, 5, size=(B, N)).astype(np.float32)
    sig = rng.uniform(0.5, 3, size=(B, N)).astype(np.float32)
    v64 = cm.sample(u, sig, SEED, 1, 2, 100, K, -15.0, 15.0, np.float64)
    v32 = cm.sample(u, sig, SEED, 1, 2, 100, K, -15.0, 15.0, np.float32)
    assert np.abs(v32 - v64).max() < 2e-5 and np.array_equal(v32.reshape(B, K, N)[:, 0], u)
    s = rng.uniform(10, 100, size=B * K).astype(np.float32)
    worst = [0.0, 0.0]
    for E, alpha in ((8, 0.25), (8, 0.0), (K, 0.0), (1, 0.5)):
        a, b = cm.update(u, sig, v32, s, E, alpha, 0.05, np.float32), cm.update(u, sig, v32, s, E, alpha, 0.05, np.float64)
        worst = [max(worst[0], np.abs(a["u"] - b["u"]).max()), max(worst[1], np.abs(a["sig"] - b["sig"]).max())]
        assert np.array_equal(a["elite"], b["elite"])
    print(f"f32 vs f64 form: mean {worst[0]:.2e}, sigma {worst[1]:.2e}")
    assert worst[0] < 2e-6 and worst[1] < 2e-6


# ----------------------------------------------------------------------------- 3. options
def test_options_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} phnn_cem_options;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _capi.CemOptions._fields_]
    # 3 x int32, float, float[4], float (+4 padding), uint64, int64, pointer, int32, int32[4] (+4 padding)
    assert C.sizeof(_capi.CemOptions) == 88
    o = _capi.CemOptions
    assert (o.sigma_init.offset, o.sigma_min.offset, o.seed.offset, o.epoch_dev.offset, o.reserved.offset) == (16, 32, 40, 56, 68)
    for name in ("phnn_cem_workspace_bytes", "phnn_cem_sample", "phnn_cem_update", "phnn_solve_cem"):
        assert name in _capi.EXPORTED and re.search(r"\b%s\(" % name, header)


# ----------------------------------------------------------------------------- 4. host logic on the CPU oracle
def _model(name, cls, precision="f64"):
    w = ol.load_weights(name)
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return m.set_engine(cm.CemOracleEngine(w, precision))


def _cfg(**mpc):
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(dict(optimizer="CrossEntropy", samples=16, elites=4, alpha=0.25, sigma=3.0, sigma_min=0.05, seed=SEED,
                           optimizer_steps=3), **mpc)
    return cfg


def test_cem_solve_best_cost_is_monotone_and_reproducible():
    eng = _model("phnn_cartpole", pHNN).engine
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), _cfg())
    x0 = torch.tensor(np.stack([X0, -X0, 2 * X0]))
    u0 = torch.full((3, 20, 1), 20.0)  # past the clamp
    kw = dict(samples=16, elites=4, alpha=0.25, sigma=3.0, sigma_min=0.05, seed=SEED)
    prev = None
    for iters in range(0, 4):
        out = cem_solve(eng, x0, u0, c._cost(), "euler", 0.02, iters, **kw)
        assert out["costs"].shape == (iters, 3)
        if iters == 0:
            assert torch.all(torch.isinf(out["best_cost"])) and torch.all(out["best_u"] == 0)
            assert torch.equal(out["u_last"], torch.clamp(u0, -15.0, 15.0)) and torch.all(out["sigma_last"] == 3.0)
        else:
            assert torch.all(out["best_cost"] <= prev) and torch.all(out["best_cost"] <= out["costs"][0])
            assert torch.all(out["u_last"].abs() <= 15.0) and torch.all(out["sigma_last"] >= np.float32(0.05))
        prev = out["best_cost"]
    assert float(out["sigma_last"].std()) > 0  # per element by now
    again = cem_solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, **kw)
    assert all(torch.equal(out[k], again[k]) for k in out)
    # problem 1 alone, with its offset: the same problem
    one = cem_solve(eng, x0[1:2], u0[1:2], c._cost(), "euler", 0.02, 3, problem_offset=1, **kw)
    assert all(torch.equal(out[k][..., 1:2] if k == "costs" else out[k][1:2], one[k]) for k in out)
    other = cem_solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, epoch=1, **kw)
    assert not torch.equal(out["u_last"], other["u_last"])


def test_controllers_route_cross_entropy():
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), _cfg())
    assert (c.optimizer_type, c.samples, c.elites, c.alpha, c.sigma, c.sigma_min, c.seed, c.max_iterations) == (
        "CrossEntropy", 16, 4, 0.25, 3.0, 0.05, SEED, 3)
    states = np.stack([X0, -X0])
    u = c.compute_control_batch(states, epoch=4)
    assert u.shape == (2, 1) and np.all(np.abs(u) <= 15.0) and np.any(u != 0)
    assert np.array_equal(u, c.compute_control_batch(states, epoch=4))
    out = cem_solve(c.engine, torch.tensor(states), torch.zeros(2, 20, 1), c._cost(), "euler", 0.02, epoch=4,
                    **c.cem_options())
    assert np.array_equal(u, out["u_last"][:, 0, :].numpy())
    # the single-plant call numbers its own solves: fresh noise per call, the same sequence after a reset
    c.epoch = 0
    a, b = c.compute_control(X0.copy()), c.compute_control(X0.copy())
    c.epoch = 0
    assert a.shape == (1,) and np.array_equal(a, c.compute_control(X0.copy())) and not np.array_equal(a, b)

    k = create_mpc_controller(_model("canonical_cartpole", pHNN_Canonical), _cfg())
    assert (k.optimizer, k.samples, k.elites, k.alpha, k.sigma_min, k.optimizer_steps) == ("CrossEntropy", 16, 4, 0.25, 0.05, 3)
    u1, seq, best = k.control_batch(states, None, epoch=0)
    assert u1.shape == (2, 1) and seq.shape == (2, 20, 1) and np.all(np.abs(seq) <= 15.0) and np.all(np.isfinite(best))
    u2, seq2, best2 = k.control_batch(states, seq, epoch=1)  # warm start from the shift
    assert np.all(np.isfinite(best2))
    uu, info = k.control(X0.copy(), None)
    assert uu.shape == (1,) and len(info["optimization"]["costs"]) == 3
    assert info["optimization"]["final_cost"] <= info["optimization"]["costs"][0]
    # closed loop on the host: step s solves with epoch s
    log = run_mpc_batch(BatchedCartPole(0.02), c, states, 3)
    assert log["controls"].shape == (3, 2, 1)
    assert np.array_equal(log["controls"][1], c.compute_control_batch(log["states"][1].astype(np.float32), epoch=1))
    assert not np.array_equal(log["controls"][1], c.compute_control_batch(log["states"][1].astype(np.float32), epoch=2))


def test_argument_errors():
    m = _model("phnn_cartpole", pHNN)
    with pytest.raises(ValueError, match="Unknown optimizer type"):
        MPCController(m, 20, 0.02, [1.0] * 4, 0.01, optimizer_type="CrossEntropyMethod").solve_batch(X0[None])
    with pytest.raises(ValueError, match="Unknown optimizer type"):
        create_mpc_controller(_model("canonical_cartpole", pHNN_Canonical), _cfg(optimizer="CrossEntropyMethod"))
    c = create_mpc_from_config(m, _cfg())
    x0, u0 = torch.tensor(X0[None]), torch.zeros(1, 20, 1)
    ok = dict(samples=4, elites=2, alpha=0.25, sigma=1.0, sigma_min=0.05, seed=0)
    for bad in (dict(samples=1, elites=1), dict(elites=0), dict(elites=5), dict(alpha=-0.1), dict(alpha=1.0),
                dict(alpha=float("nan")), dict(sigma=-1.0), dict(sigma=float("inf")), dict(sigma_min=-1.0),
                dict(sigma=(1.0, 2.0))):
        with pytest.raises(ValueError):
            cem_solve(m.engine, x0, u0, c._cost(), "euler", 0.02, 1, **{**ok, **bad})
    with pytest.raises(NotImplementedError):
        cem_solve(m.engine, x0, u0, c._cost(), "euler", 0.02, 1, x_ref=np.zeros((1, 3, 4), np.float32), **ok)


# ----------------------------------------------------------------------------- 5. static: the new code object
def test_cem_kernels_are_in_the_library_without_scratch():
    """k_sample, shared with MPPI (both sigma sources x both alignments), and k_cem_update (four widths x two
    alignments) are in libphnn_mpc.so and none of them touches scratch memory: the check tests/test_mppi_model.py makes
    for the MPPI kernels."""
    import test_static_isa as si
    if not os.path.exists(os.path.join(si.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    import subprocess
    import tempfile
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, img in enumerate(si._code_objects(si.LIB)):
            if b"k_cem_update" not in img:
                continue
            f = os.path.join(tmp, f"co{k}.elf")
            open(f, "wb").write(img)
            txt = subprocess.run([os.path.join(si.LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", f], capture_output=True,
                                 text=True, check=True).stdout
            for name, body in re.findall(r"^[0-9a-f]+ <([^>]*k_(?:cem_update|sample|clamp|sigma_init)[^>]*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", txt, re.S | re.M):
                found[name] = body
    upd = sorted(n for n in found if "k_cem_update" in n)
    smp = sorted(n for n in found if "k_sample" in n)
    assert len(upd) == 8 and len(smp) == 4, (upd, smp)
    assert any("k_clamp" in n for n in found) and any("k_sigma_init" in n for n in found)  # the small kernels, no scratch either
    for name, body in found.items():
        assert "scratch_" not in body, name


# ----------------------------------------------------------------------------- 6. the saturated start
SAT = dict(samples=64, elites=8, alpha=0.25, sigma=5.0, sigma_min=0.05, iters=4)  # tests/test_gpu_cem.py: same case


def saturated_case(engine, cost):
    """u_init = 2 u_max everywhere.  -> (u_init, Adam result, CEM result, cost of clamp(u_init), cost of CEM's mean)."""
    x0 = torch.tensor(X0[None]).to(engine.device)
    u_init = torch.full((1, 20, 1), 2.0 * float(cost.u_max), device=engine.device)
    adam = shooting_solve(engine, x0, u_init, cost, "euler", 0.02, 0.015, 30, u_min=float(cost.u_min), u_max=float(cost.u_max))
    cem = cem_solve(engine, x0, u_init, cost, "euler", 0.02, seed=SEED, **SAT)
    c_sat = engine.rollout_cost(x0, torch.clamp(u_init, float(cost.u_min), float(cost.u_max)), cost, "euler", 0.02)
    c_mean = engine.rollout_cost(x0, cem["u_last"], cost, "euler", 0.02)
    return u_init, adam, cem, c_sat, c_mean


def test_saturated_start_adam_is_stuck_cem_is_not():
    """The golden cart-pole pHNN with the shipped controller settings (H = 20, u in [-15, 15]) from u_init = 30
    everywhere (tests/test_mppi_model.py::saturated_case).  Adam's last iterate is u_init bit for bit; CEM with K = 64,
    E = 8, alpha = 0.25, sigma = 5, sigma_min = 0.05, 4 iterations must end strictly below cost(clamp(u_init)) = 332.56
    with both its final mean and its best sample.  Float64 model on the CPU: the mean's cost over the iterations 332.56,
    240.00, 200.11, 173.60, the final mean 155.74, best_cost 141.52."""
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), yaml.safe_load(open(CFG)))
    u_init, adam, cem, c_sat, c_mean = saturated_case(c.engine, c._cost())
    assert torch.equal(adam["u_last"], u_init)
    print("cost(clamp(u_init)) = %.6e, CEM final mean = %.6e, best_cost = %.6e, mean costs %s, sigma %.3f .. %.3f" % (
        float(c_sat), float(c_mean), float(cem["best_cost"]), cem["costs"][:, 0].tolist(), float(cem["sigma_last"].min()),
        float(cem["sigma_last"].max())))
    assert float(cem["costs"][0, 0]) == float(c_sat)  # iteration 0's sample 0 is clamp(u_init)
    assert float(c_mean) < float(c_sat) and float(cem["best_cost"]) < float(c_sat)
