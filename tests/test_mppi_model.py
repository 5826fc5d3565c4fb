"""CPU tests of the MPPI solve: the NumPy restatement of its kernels (tests/mppi_model.py: Philox4x32-10, the counter
layout, Box-Muller, the softmin update) and the host logic (solver.mppi_solve, both controllers, the closed loop) on the
CPU oracle engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import yaml

import mppi_model as mm
import oracle_lib as ol
from phnn_mpc_amd import _capi
from phnn_mpc_amd.models import pHNN, pHNN_Canonical
from phnn_mpc_amd.mpc_controller import MPCController, create_mpc_from_config
from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
from phnn_mpc_amd.solver import mppi_solve, shooting_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
SEED = 0x5EED2026C0FFEE  # the seed tests/test_gpu_mppi.py draws with
X0 = np.array([0.0, 0.1, 0.0, 0.0], np.float32)


# ----------------------------------------------------------------------------- 1. Philox known answers
@pytest.mark.parametrize("ctr, key, want", [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])])
def test_philox_known_answers(ctr, key, want):
    got = mm.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
    assert [int(x) for x in got] == want


# ----------------------------------------------------------------------------- 2. counter layout
def test_counter_layout_is_injective_and_every_field_matters():
    ends = dict(epoch=[0, 1, 99, 2 ** 31 - 1], iteration=[0, 1, 7, mm.MAX_ITERS - 1],
                gid=[0, 1, 4095, 2 ** 32 - 1, 2 ** 32, mm.MAX_PROBLEM - 1], k=[0, 1, 63, mm.MAX_SAMPLES - 1],
                j=[0, 1, 15, mm.MAX_J - 1])
    grid = np.array(np.meshgrid(*ends.values(), indexing="ij"), dtype=np.int64).reshape(5, -1)
    c = mm.counter(*grid)
    assert len({tuple(int(x) for x in row) for row in c}) == grid.shape[1]
    base = dict(epoch=3, iteration=2, gid=17, k=5, j=1)
    ref = mm.philox4x32_10(mm.counter(**base), mm.key(SEED))
    for name in base:
        other = mm.philox4x32_10(mm.counter(**{**base, name: base[name] + 1}), mm.key(SEED))
        assert not np.array_equal(ref, other), name
    assert not np.array_equal(ref, mm.philox4x32_10(mm.counter(**base), mm.key(SEED + 1)))
    assert not np.array_equal(ref, mm.philox4x32_10(mm.counter(**base), mm.key(SEED + (1 << 32))))
    # a problem's noise does not depend on the batch it is drawn in
    z = mm.normals(SEED, 3, 2, np.arange(10, 20), 8, 20)
    assert np.array_equal(z[7], mm.normals(SEED, 3, 2, [17], 8, 20)[0])


# ----------------------------------------------------------------------------- 3. noise quality
def test_noise_moments_at_the_gpu_tests_seed():
    """|mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N), |excess kurtosis| <= 5 sqrt(24 / N) over the N = B (K - 1) H m
    values of samples 1 .. K-1 (B = 37, K = 64, H = 20, m = 1); sample 0 is exactly zero."""
    B, K, N = 37, 64, 20
    z = mm.normals(SEED, 0, 0, np.arange(B), K, N)
    assert np.all(z[:, 0] == 0)
    x = z[:, 1:].ravel()
    n = x.size
    mean, var = x.mean(), x.var()
    kurt = ((x - mean) ** 4).mean() / var ** 2 - 3
    print(f"N={n} mean={mean:.3e} (bound {5 / np.sqrt(n):.3e}) var-1={var - 1:.3e} ({5 * np.sqrt(2 / n):.3e}) "
          f"kurt={kurt:.3e} ({5 * np.sqrt(24 / n):.3e})")
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n) and abs(kurt) <= 5 * np.sqrt(24 / n)
    z32 = mm.normals(SEED, 0, 0, np.arange(B), K, N, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5 and np.all(np.isfinite(z32))


# ----------------------------------------------------------------------------- 4. the update
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_update_restatement(dtype):
    rng = np.random.default_rng(1)
    B, K, N = 5, 37, 23
    u = rng.normal(size=(B, N)).astype(np.float32)
    v = rng.normal(size=(B * K, N)).astype(np.float32)
    v.reshape(B, K, N)[:, 0] = u
    s = rng.uniform(1, 50, size=B * K).astype(np.float32)
    r = mm.update(u, v, s, 3.0, dtype)
    assert np.allclose(r["p"].sum(axis=1), 1, atol=1e-6 if dtype == np.float32 else 1e-14)
    assert np.array_equal(r["kmin"], s.reshape(B, K).argmin(axis=1))
    # equal costs: the plain mean; with every sample equal to the nominal, the nominal
    same = np.repeat(u, K, axis=0)
    r = mm.update(u, same, np.full(B * K, 7.0, np.float32), 3.0, dtype)
    assert np.allclose(r["u"], u, atol=1e-6) and np.all(r["kmin"] == 0)  # tie -> lowest k
    # lambda -> small: the single best sample
    r = mm.update(u, v, s, 1e-4, dtype)
    assert np.array_equal(r["u"].astype(np.float32), v.reshape(B, K, N)[np.arange(B), r["kmin"]])
    # non-finite costs are ignored (even the lowest-looking ones); all non-finite keeps u
    s2 = s.copy().reshape(B, K)
    s2[:, 3], s2[:, 5], s2[:, 8] = np.nan, np.inf, -np.inf
    s2[4] = np.nan
    r2 = mm.update(u, v, s2.ravel(), 3.0, dtype)
    keep = np.ones(K, bool)
    keep[[3, 5, 8]] = False
    r3 = mm.update(u[:4], v.reshape(B, K, N)[:4][:, keep].reshape(-1, N), s.reshape(B, K)[:4][:, keep].ravel(), 3.0,
                   np.float64)
    assert np.allclose(r2["u"][:4], r3["u"], atol=1e-5) and np.all(r2["p"][:, [3, 5, 8]] == 0)
    assert np.array_equal(r2["u"][4], u[4].astype(dtype)) and r2["kmin"][4] == -1 and np.all(np.isfinite(r2["u"]))
    # ties: lowest k
    s3 = s.copy().reshape(B, K)
    s3[:, 20], s3[:, 11] = 0.5, 0.5
    assert np.all(mm.update(u, v, s3.ravel(), 3.0, dtype)["kmin"] == 11)


def test_float32_form_stays_next_to_the_float64_form():
    rng = np.random.default_rng(2)
    B, K, N = 7, 64, 50
    u = rng.uniform(-5, 5, size=(B, N)).astype(np.float32)
    v64 = mm.sample(u, 2.0, 1, SEED, 1, 2, 100, K, -15.0, 15.0, np.float64)
    v32 = mm.sample(u, 2.0, 1, SEED, 1, 2, 100, K, -15.0, 15.0, np.float32)
    assert np.abs(v32 - v64).max() < 2e-5 and np.array_equal(v32.reshape(B, K, N)[:, 0], u)
    s = rng.uniform(10, 100, size=B * K).astype(np.float32)
    a, b = mm.update(u, v32, s, 5.0, np.float32), mm.update(u, v32, s, 5.0, np.float64)
    assert np.abs(a["u"] - b["u"]).max() < 2e-5


# ----------------------------------------------------------------------------- 5. host logic on the CPU oracle
def _model(name, cls, precision="f64"):
    w = ol.load_weights(name)
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return m.set_engine(mm.MppiOracleEngine(w, precision))


def _cfg(**mpc):
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(dict(optimizer="MPPI", samples=16, lam=5.0, sigma=3.0, seed=SEED, optimizer_steps=3), **mpc)
    return cfg


def test_options_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} phnn_mppi_options;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _capi.MppiOptions._fields_]
    # 2 x int32, float, float[4] (+4 padding), uint64, int64, pointer, int32, int32[4] (+4 padding)
    assert C.sizeof(_capi.MppiOptions) == 80
    assert (_capi.MppiOptions.seed.offset, _capi.MppiOptions.epoch_dev.offset, _capi.MppiOptions.reserved.offset) == (32, 48, 60)
    assert "phnn_solve_mppi" in _capi.EXPORTED and "phnn_mppi_sample" in _capi.EXPORTED and "phnn_mppi_update" in _capi.EXPORTED


def test_mppi_solve_best_cost_is_monotone_and_reproducible():
    eng = _model("phnn_cartpole", pHNN).engine
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), _cfg())
    x0 = torch.tensor(np.stack([X0, -X0, 2 * X0]))
    u0 = torch.zeros(3, 20, 1)
    kw = dict(samples=16, lam=5.0, sigma=3.0, seed=SEED)
    prev = None
    for iters in range(0, 4):
        out = mppi_solve(eng, x0, u0, c._cost(), "euler", 0.02, iters, **kw)
        assert out["costs"].shape == (iters, 3)
        if iters == 0:
            assert torch.all(torch.isinf(out["best_cost"])) and torch.all(out["best_u"] == 0)
            assert torch.equal(out["u_last"], u0)
        else:
            assert torch.all(out["best_cost"] <= prev) and torch.all(out["best_cost"] <= out["costs"][0])
            assert torch.all(out["u_last"].abs() <= 15.0)
        prev = out["best_cost"]
    again = mppi_solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, **kw)
    assert all(torch.equal(out[k], again[k]) for k in out)
    # problem 1 alone, with its offset: the same problem
    one = mppi_solve(eng, x0[1:2], u0[1:2], c._cost(), "euler", 0.02, 3, problem_offset=1, **kw)
    assert all(torch.equal(out[k][..., 1:2] if k == "costs" else out[k][1:2], one[k]) for k in out)
    other = mppi_solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, epoch=1, **kw)
    assert not torch.equal(out["u_last"], other["u_last"])


def test_controllers_route_mppi():
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), _cfg())
    assert (c.optimizer_type, c.samples, c.lam, c.sigma, c.seed, c.max_iterations) == ("MPPI", 16, 5.0, 3.0, SEED, 3)
    states = np.stack([X0, -X0])
    u = c.compute_control_batch(states, epoch=4)
    assert u.shape == (2, 1) and np.all(np.abs(u) <= 15.0) and np.any(u != 0)
    assert np.array_equal(u, c.compute_control_batch(states, epoch=4))
    out = mppi_solve(c.engine, torch.tensor(states), torch.zeros(2, 20, 1), c._cost(), "euler", 0.02, epoch=4,
                     **c.mppi_options())
    assert np.array_equal(u, out["u_last"][:, 0, :].numpy())
    # the single-plant call numbers its own solves: fresh noise per call, the same sequence after a reset
    c.epoch = 0
    a, b = c.compute_control(X0.copy()), c.compute_control(X0.copy())
    c.epoch = 0
    assert a.shape == (1,) and np.array_equal(a, c.compute_control(X0.copy())) and not np.array_equal(a, b)

    k = create_mpc_controller(_model("canonical_cartpole", pHNN_Canonical), _cfg())
    assert (k.optimizer, k.samples, k.optimizer_steps) == ("MPPI", 16, 3)
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


def test_argument_errors():
    m = _model("phnn_cartpole", pHNN)
    with pytest.raises(ValueError, match="Unknown optimizer type"):
        MPCController(m, 20, 0.02, [1.0] * 4, 0.01, optimizer_type="CEM").solve_batch(X0[None])
    with pytest.raises(ValueError, match="Unknown optimizer type"):
        create_mpc_controller(_model("canonical_cartpole", pHNN_Canonical), _cfg(optimizer="CEM"))
    c = create_mpc_from_config(m, _cfg())
    x0, u0 = torch.tensor(X0[None]), torch.zeros(1, 20, 1)
    with pytest.raises(ValueError):
        mppi_solve(m.engine, x0, u0, c._cost(), "euler", 0.02, 1, samples=1, lam=1.0, sigma=1.0, seed=0)
    with pytest.raises(ValueError):
        mppi_solve(m.engine, x0, u0, c._cost(), "euler", 0.02, 1, samples=4, lam=0.0, sigma=1.0, seed=0)
    with pytest.raises(ValueError):
        mppi_solve(m.engine, x0, u0, c._cost(), "euler", 0.02, 1, samples=4, lam=1.0, sigma=-1.0, seed=0)
    with pytest.raises(NotImplementedError):
        mppi_solve(m.engine, x0, u0, c._cost(), "euler", 0.02, 1, samples=4, lam=1.0, sigma=1.0, seed=0,
                   x_ref=np.zeros((1, 3, 4), np.float32))


# ----------------------------------------------------------------------------- 11. static: the new code object
def test_mppi_kernels_are_in_the_library_without_scratch():
    """k_sample, shared with CEM (both sigma sources x both alignments), and k_mppi_update (four widths x two alignments)
    are in libphnn_mpc.so; none of them touches scratch memory, the aligned sampler stores 16 bytes at a time, and the
    update's row reductions are DPP."""
    import test_static_isa as si
    if not os.path.exists(os.path.join(si.LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    import subprocess
    import tempfile
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, img in enumerate(si._code_objects(si.LIB)):
            if b"k_mppi_update" not in img:
                continue
            f = os.path.join(tmp, f"co{k}.elf")
            open(f, "wb").write(img)
            txt = subprocess.run([os.path.join(si.LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", f], capture_output=True,
                                 text=True, check=True).stdout
            for name, body in re.findall(r"^[0-9a-f]+ <([^>]*k_(?:mppi_update|sample|clamp|sigma_init)[^>]*)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", txt, re.S | re.M):
                found[name] = body
    upd = sorted(n for n in found if "k_mppi_update" in n)
    smp = sorted(n for n in found if "k_sample" in n)
    assert len(upd) == 8 and len(smp) == 4, (upd, smp)
    assert any("k_clamp" in n for n in found) and any("k_sigma_init" in n for n in found)  # the small kernels, no scratch either
    assert {re.search(r"k_sampleI(Lb\dELb\d)E", n).group(1) for n in smp} == {"Lb0ELb0", "Lb0ELb1", "Lb1ELb0", "Lb1ELb1"}
    for name, body in found.items():
        assert "scratch_" not in body, name
    assert all("_dpp" in found[n] for n in upd)
    assert all(("global_store_dwordx4" in found[n]) == ("ELb1EE" in n) for n in smp)


# ----------------------------------------------------------------------------- 6. the saturated start
SAT = dict(samples=64, lam=50.0, sigma=5.0, iters=4)  # tests/test_gpu_mppi.py runs the same case on the device


def saturated_case(engine, cost):
    """u_init = 2 u_max everywhere.  -> (u_init, Adam result, MPPI result, cost of clamp(u_init))."""
    x0 = torch.tensor(X0[None]).to(engine.device)
    u_init = torch.full((1, 20, 1), 2.0 * float(cost.u_max), device=engine.device)
    adam = shooting_solve(engine, x0, u_init, cost, "euler", 0.02, 0.015, 30, u_min=float(cost.u_min), u_max=float(cost.u_max))
    mppi = mppi_solve(engine, x0, u_init, cost, "euler", 0.02, seed=SEED, **SAT)
    c_sat = engine.rollout_cost(x0, torch.clamp(u_init, float(cost.u_min), float(cost.u_max)), cost, "euler", 0.02)
    return u_init, adam, mppi, c_sat


def test_saturated_start_adam_is_stuck_mppi_is_not():
    """The golden cart-pole pHNN with the shipped controller settings (H = 20, u in [-15, 15]) from u_init = 30
    everywhere.  Adam's gradient is exactly zero past the bound, so its last iterate is u_init bit for bit; MPPI samples
    around clamp(u_init) = 15 and must end strictly below that sequence's cost.  Chosen K = 64, sigma = 5 (a third of
    the bound), lambda = 50, 4 iterations.  Float64 model on the CPU: cost(clamp(u_init)) = 332.56, the nominal's cost
    over the iterations 332.56, 242.12, 197.90, 173.16, MPPI best_cost = 115.12: a factor 2.9 below."""
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), yaml.safe_load(open(CFG)))
    u_init, adam, mppi, c_sat = saturated_case(c.engine, c._cost())
    assert torch.equal(adam["u_last"], u_init)
    print("cost(clamp(u_init)) = %.6e, MPPI best_cost = %.6e, nominal costs %s" % (
        float(c_sat), float(mppi["best_cost"]), mppi["costs"][:, 0].tolist()))
    assert float(mppi["costs"][0, 0]) == float(c_sat)  # iteration 0's sample 0 is clamp(u_init)
    assert float(mppi["best_cost"]) < float(c_sat)
    assert float(mppi["best_cost"]) < 0.5 * float(c_sat)  # the room the docstring records
