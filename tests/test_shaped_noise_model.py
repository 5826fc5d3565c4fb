"""Shaped (time-correlated) sampling noise on the CPU: the builders of phnn_mpc_amd/noise.py, the NumPy restatement of
k_shaped_sample (tests/shaped_noise_model.py), the ctypes struct, and the `noise` plumbing of the solvers and controllers
on the CPU oracle engines.  The device side is tests/test_gpu_shaped_noise.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import yaml

import cem_model as cm
import mppi_model as mm
import oracle_lib as ol
import shaped_noise_model as sn
from phnn_mpc_amd import _capi, noise
from phnn_mpc_amd.models import pHNN, pHNN_Canonical
from phnn_mpc_amd.mpc_controller import MPCController, create_mpc_from_config
from phnn_mpc_amd.mpc_controller_canonical import MPCControllerCanonical, create_mpc_controller
from phnn_mpc_amd.solver import cem_solve, mppi_solve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
SEED = 0x5EED2026C0FFEE
X0 = np.array([0.0, 0.1, 0.0, 0.0], np.float32)
HORIZONS = [1, 5, 20, 50, 64, 256]


def row_norms(L):
    return np.sqrt((L.astype(np.float64) ** 2).sum(axis=1))


# ----------------------------------------------------------------------------- 1. builders
@pytest.mark.parametrize("H", HORIZONS)
def test_builders_return_unit_norm_float32_factors_of_the_requested_covariance(H):
    t = np.arange(H)
    shapes = {"ar1(0.9)": (noise.ar1(H, 0.9), 0.9 ** np.abs(t[:, None] - t[None, :])),
              "ar1(-0.5)": (noise.ar1(H, -0.5), (-0.5) ** np.abs(t[:, None] - t[None, :]))}
    for beta in (0.5, 1.0, 2.0, 3.0):  # a Cholesky factor exists in float64 up to beta = 3 at H = 256
        shapes[f"colored({beta})"] = (noise.colored(H, beta), noise.colored_covariance(H, beta))
    rng = np.random.default_rng(H)
    A = rng.normal(size=(H, H + 3))
    cov = A @ A.T
    d = np.sqrt(np.diag(cov))
    shapes["from_covariance"] = (noise.from_covariance(cov), cov / d[:, None] / d[None, :])
    for name, (L, want) in shapes.items():
        assert L.dtype == np.float32 and L.shape == (H, H), name
        assert np.abs(row_norms(L) - 1).max() <= 1e-6, name
        assert np.array_equal(L, np.tril(L)), name
        L64 = L.astype(np.float64)
        assert np.abs(np.diag(want) - 1).max() < 1e-12, name
        # float32 rounding of L: |d(L L^T)| <= 2 * 2^-24 * |L| |L|^T <= 2^-23 per entry for unit rows
        assert np.abs(L64 @ L64.T - want).max() <= 4e-7, name
    for name, L in (("colored(0)", noise.colored(H, 0)), ("colored(0.0)", noise.colored(H, 0.0)), ("ar1(0)", noise.ar1(H, 0.0))):
        assert L.dtype == np.float32 and np.array_equal(L, np.eye(H, dtype=np.float32)), name
    W = rng.normal(size=(H, max(H // 2, 1)))
    Ln = noise.normalize_rows(W)
    assert Ln.dtype == np.float32 and np.abs(row_norms(Ln) - 1).max() <= 1e-6
    assert np.allclose(Ln, W / np.sqrt((W * W).sum(axis=1, keepdims=True)), rtol=0, atol=1e-7)


@pytest.mark.parametrize("H", HORIZONS)
def test_knots_reproduce_their_values_at_the_knot_steps(H):
    for P in sorted({1, 2, min(8, H), H}):
        if P > H:
            continue
        L = noise.knots(H, P)
        assert L.dtype == np.float32 and L.shape == (H, P) and np.abs(row_norms(L) - 1).max() <= 1e-6
        steps = noise.knot_steps(H, P)
        assert len(set(steps.tolist())) == P and steps[0] == 0 and (P == 1 or steps[-1] == H - 1)
        vals = np.random.default_rng(P).normal(size=(P, 2))
        z = sn.shape(L, vals)  # (H, 2)
        if P > 1:
            assert np.array_equal(L[steps], np.eye(P, dtype=np.float32))
            assert np.array_equal(z[steps], vals)
        else:
            assert np.array_equal(z, np.repeat(vals, H, axis=0))
        assert np.all(L >= 0) and np.all((L > 0).sum(axis=1) <= 2)  # a step mixes at most its two neighbouring knots
    assert np.array_equal(noise.knots(H, H), np.eye(H, dtype=np.float32))


def test_builder_and_holder_argument_errors():
    for bad in (lambda: noise.ar1(5, 1.0), lambda: noise.ar1(0, 0.5), lambda: noise.colored(5, -1.0), lambda: noise.knots(5, 6),
                lambda: noise.knots(5, 0), lambda: noise.knots(5, 2, kind="cubic"), lambda: noise.from_covariance(-np.eye(3)),
                lambda: noise.from_covariance(np.ones((2, 3))), lambda: noise.normalize_rows(np.zeros((3, 2))),
                lambda: noise.normalize_rows(np.ones((2, 3))), lambda: noise.Noise(np.ones((2, 3))),
                lambda: noise.Noise(np.full((2, 2), np.nan)), lambda: noise.resolve({"type": "pink"}, 5),
                lambda: noise.resolve({"rho": 0.5}, 5), lambda: noise.resolve({"type": "ar1", "beta": 1.0}, 5),
                lambda: noise.resolve(np.eye(4), 5), lambda: noise.resolve(noise.Noise(np.eye(4)), 5)):
        with pytest.raises(ValueError):
            bad()
    assert noise.resolve(None, 5) is None
    n = noise.Noise(noise.ar1(5, 0.5))
    assert noise.resolve(n, 5) is n and (n.H, n.P) == (5, 5) and hash(n) == hash(n) and n != noise.Noise(noise.ar1(5, 0.5))
    assert {n: 1}[n] == 1 and n.tensor("cpu") is n.tensor("cpu") and n.tensor("cpu").dtype == torch.float32
    assert np.array_equal(noise.resolve({"type": "ar1", "rho": 0.9}, 20).L, noise.ar1(20, 0.9))
    assert np.array_equal(noise.resolve({"type": "colored", "beta": 2.0}, 20).L, noise.colored(20, 2.0))
    assert np.array_equal(noise.resolve({"type": "knots", "count": 8}, 20).L, noise.knots(20, 8))
    assert noise.resolve({"type": "knots", "count": 8}, 5).P == 5  # no more knots than steps
    assert np.array_equal(noise.resolve(np.eye(5) * 2, 5).L, 2 * np.eye(5, dtype=np.float32))  # an array is used as given


# ----------------------------------------------------------------------------- 2. the model
@pytest.mark.parametrize("m, H", [(1, 20), (2, 25), (4, 64), (1, 1), (1, 256)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_shape_is_the_unshaped_sampler(m, H, dtype):
    B, K, N = 3, 5, H * m
    rng = np.random.default_rng(H + m)
    u = rng.uniform(-12, 12, size=(B, N)).astype(np.float32)
    sig_t = tuple(2.0 + 0.5 * i for i in range(m))
    sig = rng.uniform(0.0, 3.0, size=(B, N)).astype(np.float32)
    eye = np.eye(H, dtype=np.float32)
    for bounds in ((None, None), (-10.0, 10.0)):
        a = sn.sample(u, sig_t, m, eye, SEED, 3, 2, 1000, K, *bounds, dtype)
        b = mm.sample(u, sig_t, m, SEED, 3, 2, 1000, K, *bounds, dtype)
        assert a.dtype == b.dtype and np.all(a == b)
        a = sn.sample_tensor(u, sig, m, eye, SEED, 3, 2, 1000, K, *bounds, dtype)
        b = cm.sample(u, sig, SEED, 3, 2, 1000, K, *bounds, dtype)
        assert a.dtype == b.dtype and np.all(a == b)
    assert np.all(a.reshape(B, K, N)[:, 0] == np.clip(u, -10, 10))  # sample 0 is the clamped mean


def test_float32_form_stays_next_to_the_float64_form_and_sums_in_order():
    H, P, m, K = 50, 50, 2, 9
    L = noise.ar1(H, 0.9)
    gids = 7 + np.arange(4)
    z32, z64 = sn.noise(L, m, SEED, 1, 0, gids, K, np.float32), sn.noise(L, m, SEED, 1, 0, gids, K, np.float64)
    assert z32.dtype == np.float32 and np.abs(z32 - z64).max() < 2e-5 and np.all(z32[:, 0] == 0)
    eps = sn.white(SEED, 1, 0, gids, K, P, m, np.float32)
    acc = np.float32(0)
    for s in range(P):  # element (t, c) = (17, 1) of problem 2, sample 4, by hand
        acc = np.float32(acc + np.float32(L[17, s] * eps[2, 4, s, 1]))
    assert z32[2, 4, 17 * m + 1] == acc


def test_statistics_of_ar1_noise():
    """B = 8, K = 513, H = 20, m = 1, ar1(20, 0.9): n = 4096 shaped rows.  max |C^ - L L^T| <= 6 sqrt(2 / n) = 0.133
    (six standard deviations of a sample variance of unit normals), mean squared first difference within 5 % of
    2 (1 - rho) = 0.2."""
    B, K, H, rho = 8, 513, 20, 0.9
    L = noise.ar1(H, rho)
    z = sn.noise(L, 1, SEED, 0, 0, np.arange(B), K)[:, 1:].reshape(-1, H)
    n = z.shape[0]
    assert n == 4096
    Chat = z.T @ z / n
    L64 = L.astype(np.float64)
    err = np.abs(Chat - L64 @ L64.T).max()
    msd = float((np.diff(z, axis=1) ** 2).mean())
    print(f"\nmax |C^ - L L^T| = {err:.3f} (bound {6 * np.sqrt(2 / n):.3f}), mean squared first difference = {msd:.3f}")
    assert err <= 6 * np.sqrt(2 / n)
    assert abs(msd / (2 * (1 - rho)) - 1) <= 0.05
    assert abs(z.mean()) < 6 / np.sqrt(n)  # the mean of n*H correlated unit normals: well inside 6 / sqrt(n)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_components_are_shaped_separately(dtype):
    H, P, m, K = 25, 25, 2, 6
    L = noise.colored(H, 2.0)
    gids = np.arange(3)
    eps = sn.white(SEED, 0, 1, gids, K, P, m, dtype)
    z = sn.noise(L, m, SEED, 0, 1, gids, K, dtype, eps=eps).reshape(3, K, H, m)
    eps0 = eps.copy()
    eps0[..., 1] = 0
    z0 = sn.noise(L, m, SEED, 0, 1, gids, K, dtype, eps=eps0).reshape(3, K, H, m)
    assert z[..., 0].tobytes() == z0[..., 0].tobytes()  # bit for bit
    assert np.all(z0[..., 1] == 0) and np.any(z[..., 1] != 0)
    # the white row is the unshaped sampler's row of length P * m: element s * m + c
    assert np.array_equal(eps.reshape(3, K, P * m), mm.normals(SEED, 0, 1, gids, K, P * m, dtype))


# ----------------------------------------------------------------------------- 3. the struct
def test_noise_shape_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} phnn_noise_shape;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _capi.NoiseShape._fields_] == ["L_dev", "rows", "cols", "reserved"]
    # pointer, 2 x int32, int32[4]
    assert C.sizeof(_capi.NoiseShape) == 32
    assert (_capi.NoiseShape.L_dev.offset, _capi.NoiseShape.rows.offset, _capi.NoiseShape.cols.offset,
            _capi.NoiseShape.reserved.offset) == (0, 8, 12, 16)
    for name in ("phnn_mppi_sample_shaped", "phnn_cem_sample_shaped", "phnn_solve_mppi_shaped", "phnn_solve_cem_shaped"):
        assert name in _capi.EXPORTED and re.search(r"\b%s\(" % name, header)
    s = noise.Noise(noise.knots(20, 8)).struct("cpu")
    assert (s.rows, s.cols, list(s.reserved)) == (20, 8, [0, 0, 0, 0]) and s.L_dev


# ----------------------------------------------------------------------------- 4. solvers and controllers on the CPU oracle
class Recorder:
    """Wraps an engine: records the keyword names of every *_sample call."""

    def __init__(self, engine):
        self._e, self.calls = engine, []

    def __getattr__(self, name):
        attr = getattr(self._e, name)
        if name in ("mppi_sample", "cem_sample"):
            def wrapped(*a, **k):
                self.calls.append((name, dict(k)))
                return attr(*a, **k)
            return wrapped
        return attr


def _model(name, cls, engine_cls=sn.ShapedCemOracleEngine):
    w = ol.load_weights(name)
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return m.set_engine(engine_cls(w, "f64"))


def _cfg(optimizer, **mpc):
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(dict(optimizer=optimizer, samples=16, lam=5.0, sigma=3.0, seed=SEED, optimizer_steps=2, elites=4), **mpc)
    return cfg


@pytest.mark.parametrize("optimizer", ["MPPI", "CrossEntropy"])
def test_controllers_route_noise(optimizer):
    meth = {"MPPI": "mppi", "CrossEntropy": "cem"}[optimizer]
    states = np.stack([X0, -X0])
    for make, name, cls in ((create_mpc_from_config, "phnn_cartpole", pHNN), (create_mpc_controller, "canonical_cartpole", pHNN_Canonical)):
        run = (lambda c, **k: c.control_batch(states, None, **k)[0]) if make is create_mpc_controller else \
            (lambda c, **k: c.compute_control_batch(states, **k))
        # noise = None: the engine is called without a `noise` keyword, and an engine that has none keeps working
        c = make(_model(name, cls, cm.CemOracleEngine), _cfg(optimizer))
        assert c.noise is None and "noise" not in getattr(c, meth + "_options")()
        rec = Recorder(c.model.engine)
        c.model.set_engine(rec)
        white = run(c, epoch=3)
        assert rec.calls and all(n == meth + "_sample" and "noise" not in k for n, k in rec.calls)
        # every config form reaches the solve
        got = {}
        for key, spec in (("ar1", {"type": "ar1", "rho": 0.9}), ("colored", {"type": "colored", "beta": 2.0}),
                          ("knots", {"type": "knots", "count": 8}), ("array", noise.ar1(20, 0.9).tolist())):
            c = make(_model(name, cls), _cfg(optimizer, noise=spec))
            assert isinstance(c.noise, noise.Noise) and (c.noise.H, c.noise.P) == (20, 8 if key == "knots" else 20)
            assert getattr(c, meth + "_options")()["noise"] is c.noise
            rec = Recorder(c.model.engine)
            c.model.set_engine(rec)
            got[key] = run(c, epoch=3)
            assert rec.calls and all(k["noise"] is c.noise for _, k in rec.calls)
            assert got[key].shape == (2, 1) and np.all(np.abs(got[key]) <= 15.0)
            assert np.array_equal(got[key], run(c, epoch=3))  # repeatable
            assert not np.array_equal(got[key], white)
        assert np.array_equal(got["ar1"], got["array"]) and not np.array_equal(got["ar1"], got["colored"])
        with pytest.raises(ValueError, match="unknown noise type"):
            make(_model(name, cls), _cfg(optimizer, noise={"type": "brown"}))
        with pytest.raises(ValueError, match="rows"):
            make(_model(name, cls), _cfg(optimizer, noise=noise.ar1(19, 0.9)))
    # the constructor keyword, both classes
    m = _model("phnn_cartpole", pHNN)
    k = MPCController(m, 20, 0.02, [10.0, 100.0, 1.0, 10.0], 0.01, optimizer_type=optimizer, noise={"type": "ar1", "rho": 0.5})
    assert np.array_equal(k.noise.L, noise.ar1(20, 0.5))
    k = MPCControllerCanonical(_model("canonical_cartpole", pHNN_Canonical), horizon=12, optimizer=optimizer, noise=noise.Noise(noise.knots(12, 3)))
    assert (k.noise.H, k.noise.P) == (12, 3)
    with pytest.raises(ValueError):
        MPCControllerCanonical(_model("canonical_cartpole", pHNN_Canonical), horizon=12, optimizer=optimizer, noise=noise.knots(20, 3))


def test_shaped_solves_on_the_oracle_engines_repeat_bit_for_bit():
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch
    eng = _model("phnn_cartpole", pHNN).engine
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), _cfg("MPPI"))
    x0 = torch.tensor(np.stack([X0, -X0, 2 * X0]))
    u0 = torch.zeros(3, 20, 1)
    shp = noise.Noise(noise.ar1(20, 0.9))
    kw = dict(samples=16, seed=SEED, noise=shp)
    for solve, extra in ((mppi_solve, dict(lam=5.0, sigma=3.0)), (cem_solve, dict(elites=4, alpha=0.25, sigma=3.0, sigma_min=0.05))):
        a = solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, **extra, **kw)
        b = solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, **extra, **kw)
        assert all(torch.equal(a[k], b[k]) for k in a)
        assert torch.all(a["u_last"].abs() <= 15.0) and torch.all(a["best_cost"] <= a["costs"][0])
        one = solve(eng, x0[1:2], u0[1:2], c._cost(), "euler", 0.02, 3, problem_offset=1, **extra, **kw)
        assert all(torch.equal(a[k][..., 1:2] if k == "costs" else a[k][1:2], one[k]) for k in a)
        w = solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, **extra, **{**kw, "noise": None})
        assert not torch.equal(a["u_last"], w["u_last"])
        i = solve(eng, x0, u0, c._cost(), "euler", 0.02, 3, **extra, **{**kw, "noise": noise.Noise(np.eye(20))})
        assert all(torch.equal(i[k], w[k]) for k in w)  # L = I is the white solve
    # the host closed loop takes the controller's noise along
    c = create_mpc_from_config(_model("phnn_cartpole", pHNN), _cfg("MPPI", noise={"type": "ar1", "rho": 0.9}))
    log = run_mpc_batch(BatchedCartPole(0.02), c, np.stack([X0, -X0]), 3)
    assert np.array_equal(log["controls"][1], c.compute_control_batch(log["states"][1].astype(np.float32), epoch=1))
