"""Shaped (time-correlated) sampling noise on the device: k_shaped_sample through phnn_{mppi,cem}_sample_shaped and
phnn_solve_{mppi,cem}_shaped (engine.mppi_sample / cem_sample / solve_mppi / solve_cem with noise=).

  1 primitive   both sigma sources, with and without bounds, against the float64 model (tests/shaped_noise_model.py) with
                test_gpu_mppi's allowance: 8 x |float32 model - float64 model| + 1 ulp
  2 identity    L = I is the unshaped sampler value for value; sample 0 is clamp(u); x0_rep is the unshaped one
  3 bitwise     a batch == its problems alone; library loop == Python loop == its repeat; graph == eager; split-tile and
                whole-tile K1; per-problem x_ref == separate solves
  4 bounds      samples and means inside [u_min, u_max] (asserted in 1 and 3)
  5 arguments   one bad phnn_noise_shape field at a time through the four entry points; shape = NULL == the old entry point
  6 footprint   the four entry points on guarded buffers of exactly the documented sizes (tests/footprint.py), L against a
                guard
  7 oracle      one MPPI iteration with ar1(H, 0.9) against the float64 oracle, test_gpu_mppi's bound
  8 closed loop DeviceClosedLoop == run_mpc_batch, 256 plants x 30 steps, MPPI and CEM with ar1 noise
Shapes: B in {1, 3, 37}, K in {2, 5, 30, 64}; N = H*m mod 4 = 0, 1, 2, 3, aligned and misaligned bases; m = 1, 2, 4;
P = H and P < H; H = 1; the width limit (H = 256, m = 1) and (H = 64, m = 4); H = P = 64 (L staged in LDS: 64 * 65 * 4 B =
16.3 KiB <= 48 KiB) and H = P = 160 (100.6 KiB: L read from global memory).
"""
import ctypes as C

import numpy as np
import pytest
import yaml

import footprint as fp
import shaped_noise_model as sn
import test_gpu_mppi as tm
import variant_census as vc
from test_gpu_footprint import Report, footprint, rng_of
from test_gpu_footprint import engine as census_engine
from test_mppi_model import CFG, SEED

pytestmark = pytest.mark.gpu

M2 = "phnn<n=4,m=2,hid=128,fixedG,f16x2>"
M4 = "phnn<n=4,m=4,hid=128,fixedG,f16x2>"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def engine(model):
    return census_engine(model) if model in vc.CENSUS else tm.engine(model)


def shape_of(kind, H):
    from phnn_mpc_amd import noise
    return {"ar1": lambda: noise.ar1(H, 0.9), "colored": lambda: noise.colored(H, 2.0), "knots": lambda: noise.knots(H, min(8, H)),
            "eye": lambda: np.eye(H, dtype=np.float32), "one": lambda: np.ones((1, 1), np.float32),
            "half": lambda: noise.normalize_rows(np.random.default_rng(H).normal(size=(H, max(H // 2, 1))))}[kind]()


def holder(L):
    from phnn_mpc_amd.noise import Noise
    return Noise(L)


def cost_of(eng, bounds=True):
    c = tm.make_cost(eng)
    if not bounds:
        c.has_u_bounds = 0
    return c


def misaligned(torch, a):
    """A contiguous device copy of `a` whose base is 4 bytes past a 16-byte boundary."""
    flat = torch.empty(a.size + 5, dtype=torch.float32, device="cuda")
    off = 1 + (-(flat.data_ptr() // 4) % 4)
    out = flat[off: off + a.size].view(*a.shape)
    out.copy_(torch.tensor(a))
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


# (model, B, K, H, shape kind, misaligned bases): N = H*m mod 4 and the path taken
CASES = [("phnn_cartpole", 37, 64, 20, "ar1", False),   # N = 20: mod 4 = 0, aligned, staged
         ("phnn_cartpole", 37, 30, 20, "ar1", True),    # N = 20 on misaligned bases: the element path
         ("phnn_cartpole", 1, 30, 77, "knots", False),  # N = 77: mod 4 = 1, P = 8 < H
         (M2, 37, 30, 25, "colored", False),            # m = 2, N = 50: mod 4 = 2
         ("phnn_cartpole", 37, 2, 255, "half", False),  # N = 255: mod 4 = 3, P = 127, L from global memory
         ("phnn_cartpole", 3, 5, 256, "ar1", False),    # the width limit, m = 1: P * m = 256, 64 Philox calls, global L
         (M4, 3, 5, 64, "ar1", False),                  # the width limit, m = 4: N = 256, staged
         ("phnn_cartpole", 3, 5, 64, "colored", False),   # H = P = 64: staged
         ("phnn_cartpole", 3, 5, 160, "colored", False),  # H = P = 160: global
         ("phnn_cartpole", 1, 2, 1, "one", False)]      # H = 1, L = [[1]]


def inputs(torch, eng, B, H, mis, seed=1):
    m = eng.m
    x0 = torch.tensor(tm.states(B, seed), device="cuda")
    un = np.clip(tm.nominal(B, H, m, seed + 1), -10, 10)
    sg = np.random.default_rng(seed + 2).uniform(0.0, 3.0, size=(B, H, m)).astype(np.float32)
    if mis:
        return x0, misaligned(torch, un), misaligned(torch, sg), un, sg
    return x0, torch.tensor(un, device="cuda"), torch.tensor(sg, device="cuda"), un, sg


# ----------------------------------------------------------------------------- 1. the primitive against the float64 model
@pytest.mark.parametrize("model, B, K, H, kind, mis", CASES)
def test_primitive_against_the_float64_model(torch, model, B, K, H, kind, mis):
    eng = engine(model)
    m, N = eng.m, H * eng.m
    L = shape_of(kind, H)
    shp = holder(L)
    x0, u, sg, un, sgn = inputs(torch, eng, B, H, mis)
    sig, it, ep, off = tm.sigma_of(m), 3, 11, 1000
    ratios = []
    for bounds in (True, False):
        cost = cost_of(eng, bounds)
        lim = (-10.0, 10.0) if bounds else (None, None)
        for source in ("table", "tensor"):
            if source == "table":
                v, x0r = eng.mppi_sample(x0, u, cost, K, sig, SEED, it, epoch=ep, problem_offset=off, noise=shp)
                args = (un.reshape(B, N), sig, m, L, SEED, ep, it, off, K, *lim)
                v64, v32 = sn.sample(*args, np.float64), sn.sample(*args, np.float32)
            else:
                v, x0r = eng.cem_sample(x0, u, sg, cost, K, SEED, it, epoch=ep, problem_offset=off, noise=shp)
                args = (un.reshape(B, N), sgn.reshape(B, N), m, L, SEED, ep, it, off, K, *lim)
                v64, v32 = sn.sample_tensor(*args, np.float64), sn.sample_tensor(*args, np.float32)
            vd = tm.npy(v).reshape(B * K, N)
            floor = float(np.abs(v32 - v64).max())
            tol = tm.allowance(v32, v64)
            err = float(np.abs(vd - v64).max())
            ratios.append(err / max(floor, 1e-30))
            print(f"\n{model} B={B} K={K} H={H} P={L.shape[1]} m={m} {source} bounds={bounds}: |dev - f64| = {err:.3e}, "
                  f"f32 model floor = {floor:.3e}, allowance = {tol:.3e}, ratio dev/floor = {ratios[-1]:.2f}")
            assert err <= tol
            assert np.array_equal(vd.reshape(B, K, N)[:, 0], np.clip(un.reshape(B, N), *lim) if bounds else un.reshape(B, N))
            assert np.array_equal(tm.npy(x0r), np.repeat(tm.npy(x0), K, axis=0))
            if bounds:
                assert np.abs(vd).max() <= 10.0
            assert np.any(vd.reshape(B, K, N)[:, 1:] != vd.reshape(B, K, N)[:, :1])


# ----------------------------------------------------------------------------- 2. identity
@pytest.mark.parametrize("model, B, K, H, kind, mis", CASES)
def test_identity_shape_is_the_unshaped_sampler(torch, model, B, K, H, kind, mis):
    eng = engine(model)
    m = eng.m
    eye = holder(np.eye(H, dtype=np.float32))
    x0, u, sg, un, _ = inputs(torch, eng, B, H, mis, seed=4)
    cost = cost_of(eng)
    kw = dict(epoch=5, problem_offset=77)
    for sample in (lambda **k: eng.mppi_sample(x0, u, cost, K, tm.sigma_of(m), SEED, 2, **kw, **k),
                   lambda **k: eng.cem_sample(x0, u, sg, cost, K, SEED, 2, **kw, **k)):
        vw, xw = (t.clone() for t in sample())
        vs, xs = sample(noise=eye)
        assert bool((vw == vs).all()) and torch.equal(xw, xs)
        assert torch.equal(vs.view(B, K, H, m)[:, 0], torch.clamp(u, -10.0, 10.0))  # sample 0: clamp(u) bit for bit


# ----------------------------------------------------------------------------- 3. bitwise invariances
def test_batch_equals_problems_sampled_alone(torch):
    eng = engine(M2)
    B, K, H = 37, 30, 25
    shp = holder(shape_of("ar1", H))
    x0, u, sg, _, _ = inputs(torch, eng, B, H, False, seed=7)
    cost = cost_of(eng)
    full_m = eng.mppi_sample(x0, u, cost, K, tm.sigma_of(2), SEED, 1, epoch=3, problem_offset=50, noise=shp)[0].clone()
    full_c = eng.cem_sample(x0, u, sg, cost, K, SEED, 1, epoch=3, problem_offset=50, noise=shp)[0].clone()
    ws = {}
    for b in range(B):
        one = eng.mppi_sample(x0[b:b + 1], u[b:b + 1], cost, K, tm.sigma_of(2), SEED, 1, epoch=3, problem_offset=50 + b, noise=shp,
                              workspace=ws)[0]
        assert torch.equal(one, full_m[b * K:(b + 1) * K])
        one = eng.cem_sample(x0[b:b + 1], u[b:b + 1], sg[b:b + 1], cost, K, SEED, 1, epoch=3, problem_offset=50 + b, noise=shp,
                             workspace=ws)[0]
        assert torch.equal(one, full_c[b * K:(b + 1) * K])


SOLVES = {"mppi": dict(lam=25.0), "cem": dict(elites=8, alpha=0.25, sigma_min=0.05)}


def solve(eng, meth, *a, **k):
    return getattr(eng, "solve_" + meth)(*a, **SOLVES[meth], **k)


@pytest.mark.parametrize("meth", ["mppi", "cem"])
@pytest.mark.parametrize("model, integ, B, K, H, kind", [("phnn_cartpole", "euler", 37, 64, 20, "ar1"),
                                                         (M2, "rk4", 37, 30, 25, "knots"),
                                                         ("canonical_cartpole", "euler", 1, 30, 77, "colored")])
def test_library_loop_equals_python_loop_and_repeats(torch, meth, model, integ, B, K, H, kind):
    from phnn_mpc_amd.solver import cem_solve, mppi_solve
    eng = engine(model)
    cost = cost_of(eng)
    shp = holder(shape_of(kind, H))
    x0 = torch.tensor(tm.states(B, 4), device="cuda")
    u0 = torch.tensor(tm.nominal(B, H, eng.m, 5), device="cuda")  # past the clamp in places
    kw = dict(iters=3, samples=K, sigma=tm.sigma_of(eng.m), seed=SEED, epoch=2, problem_offset=7)
    a = solve(eng, meth, x0, u0, cost, integ, 0.02, noise=shp, **kw)
    b = {"mppi": mppi_solve, "cem": cem_solve}[meth](eng, x0, u0, cost, integ, 0.02, noise=shp, **SOLVES[meth], **kw)
    tm.same(torch, a, b)
    tm.same(torch, a, solve(eng, meth, x0, u0, cost, integ, 0.02, noise=shp, **kw))
    assert bool((a["u_last"].abs() <= 10.0).all()) and bool((a["best_u"].abs() <= 10.0).all())
    assert bool(torch.isfinite(a["best_cost"]).all()) and bool((a["best_cost"] <= a["costs"].min(dim=0).values).all())
    white = solve(eng, meth, x0, u0, cost, integ, 0.02, **kw)
    assert not torch.equal(a["u_last"], white["u_last"])
    tm.same(torch, white, solve(eng, meth, x0, u0, cost, integ, 0.02, noise=holder(np.eye(H, dtype=np.float32)), **kw))
    ep = torch.tensor([2], dtype=torch.int32, device="cuda")  # the epoch read from the device
    tm.same(torch, a, solve(eng, meth, x0, u0, cost, integ, 0.02, noise=shp, **{**kw, "epoch": ep}))


@pytest.mark.parametrize("meth", ["mppi", "cem"])
@pytest.mark.parametrize("B, K", [(37, 64), (300, 30)])
def test_batch_equals_problems_solved_alone(torch, meth, B, K):
    """B = 37, K = 64: 148 tiles, the split-tile K1; B = 300, K = 30: 563 tiles, the whole-tile K1; one problem alone: at
    most 4 tiles, split-tile."""
    eng = engine("phnn_cartpole")
    H, cost = 20, cost_of(eng)
    shp = holder(shape_of("ar1", H))
    x0 = torch.tensor(tm.states(B, 6), device="cuda")
    u0 = torch.tensor(tm.nominal(B, H, 1, 7), device="cuda")
    kw = dict(iters=2, samples=K, sigma=2.0, seed=SEED, epoch=5, noise=shp)
    full = solve(eng, meth, x0, u0, cost, "euler", 0.02, problem_offset=100, **kw)
    alone = {k: torch.empty_like(v) for k, v in full.items()}
    ws = {}
    for b in range(B):
        one = solve(eng, meth, x0[b:b + 1], u0[b:b + 1], cost, "euler", 0.02, problem_offset=100 + b, workspace=ws, **kw)
        for k in full:
            (alone[k][:, b:b + 1] if k == "costs" else alone[k][b:b + 1]).copy_(one[k])
    tm.same(torch, full, alone)
    half = solve(eng, meth, x0[B // 2:], u0[B // 2:], cost, "euler", 0.02, problem_offset=100 + B // 2, **kw)
    assert torch.equal(half["u_last"], full["u_last"][B // 2:]) and torch.equal(half["best_u"], full["best_u"][B // 2:])


@pytest.mark.parametrize("meth", ["mppi", "cem"])
def test_graph_equals_eager(torch, meth):
    from phnn_mpc_amd import solver
    eng = engine("canonical_cartpole")
    cost = cost_of(eng)
    B, H, K = 37, 20, 30
    shp = holder(shape_of("ar1", H))
    eager = {"mppi": solver._mppi_eager, "cem": solver._cem_eager}[meth]
    g = {"mppi": solver.mppi_solver_for, "cem": solver.cem_solver_for}[meth](eng, True)
    assert isinstance(g, solver.Graphed)
    ep = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(iters=3, samples=K, sigma=(2.0,), seed=SEED, noise=shp, **SOLVES[meth])
    for trial in range(3):  # the second and third calls replay the graph with new inputs and a new epoch
        x0 = torch.tensor(tm.states(B, 8 + trial), device="cuda")
        u0 = torch.tensor(tm.nominal(B, H, 1, 9 + trial), device="cuda")
        ep.fill_(trial)
        graph = g(eng, x0, u0, cost, "euler", 0.02, epoch=ep, **kw)
        tm.same(torch, eager(eng, x0, u0, cost, "euler", 0.02, epoch=trial, **kw), graph)
        captured = g.graph
    assert g.graph is captured
    white = eager(eng, x0, u0, cost, "euler", 0.02, epoch=2, **{**kw, "noise": None})
    assert not torch.equal(white["u_last"], graph["u_last"])


@pytest.mark.parametrize("meth", ["mppi", "cem"])
def test_per_problem_setpoints_equal_separate_solves(torch, meth):
    eng = engine("phnn_cartpole")
    B, H, K = 5, 20, 30
    shp = holder(shape_of("colored", H))
    rng = np.random.default_rng(10)
    setp = (rng.uniform(-1, 1, size=(B, 1, 4)) * [0.5, 0.05, 0.0, 0.0]).astype(np.float32)
    x0 = torch.tensor(tm.states(B, 11), device="cuda")
    u0 = torch.zeros(B, H, 1, device="cuda")
    kw = dict(iters=3, samples=K, sigma=2.0, seed=SEED, noise=shp)
    tracked = solve(eng, meth, x0, u0, tm.make_cost(eng), "euler", 0.02, x_ref=torch.tensor(setp, device="cuda"), **kw)
    for b in range(B):
        one = solve(eng, meth, x0[b:b + 1], u0[b:b + 1], tm.make_cost(eng, x_target=setp[b, 0]), "euler", 0.02, problem_offset=b, **kw)
        assert torch.equal(one["u_last"][0], tracked["u_last"][b]) and torch.equal(one["best_cost"][0], tracked["best_cost"][b])
        assert torch.equal(one["costs"][:, 0], tracked["costs"][:, b])


# ----------------------------------------------------------------------------- 5. arguments
PATTERN = -123.25


def _entry_points(torch, eng, B, H, K):
    """-> {name: call(shape pointer or None) -> (rc, [output tensors])} of the four entry points and their unshaped
    counterparts (shape = 'old'), each on fresh pattern-filled outputs."""
    from phnn_mpc_amd import _capi
    m, n = eng.m, eng.n
    cost = cost_of(eng)
    x0 = torch.tensor(tm.states(B, 20), device="cuda")
    u = torch.tensor(np.clip(tm.nominal(B, H, m, 21), -10, 10), device="cuda")
    sg = torch.full((B, H, m), 1.5, device="cuda")
    mo, _ = eng._mppi_options(2, K, 25.0, 2.0, SEED, 3, 9)
    co, _ = eng._cem_options(2, K, 3, 0.25, 2.0, 0.05, SEED, 3, 9)
    st, p = eng._stream(), (lambda t: t.data_ptr())
    full = lambda *shape: torch.full(shape, PATTERN, device="cuda")
    lib = eng.lib

    def sample(meth, opt, shape):
        v, xr = full(B * K, H, m), full(B * K, n)
        head = (eng.h, p(x0), p(u)) + ((p(sg),) if meth == "cem" else ()) + (B, H, C.byref(cost), C.byref(opt), 1)
        if shape == "old":
            rc = getattr(lib, f"phnn_{meth}_sample")(*head, p(v), p(xr), st)
        else:
            rc = getattr(lib, f"phnn_{meth}_sample_shaped")(*head, shape, p(v), p(xr), st)
        return rc, [v, xr]

    def solve_(meth, opt, shape):
        nws = getattr(eng, meth + "_workspace_bytes")(B, H, K)
        ws = torch.full((nws,), 0x5A, dtype=torch.uint8, device="cuda")
        uu, costs, bc, bu = u.clone(), full(2, B), full(B), full(B, H, m)
        outs = [uu, costs, bc, bu, ws] + ([full(B, H, m)] if meth == "cem" else [])
        head = (eng.h, p(x0), p(uu), B, H, C.byref(cost), None, 0, 0.02, C.byref(opt))
        tail = (p(ws), nws, p(costs), p(bc), p(bu)) + ((p(outs[-1]),) if meth == "cem" else ()) + (st,)
        if shape == "old":
            rc = getattr(lib, "phnn_solve_" + meth)(*head, *tail)
        else:
            rc = getattr(lib, f"phnn_solve_{meth}_shaped")(*head, shape, *tail)
        return rc, outs

    return {"phnn_mppi_sample_shaped": lambda s: sample("mppi", mo, s), "phnn_cem_sample_shaped": lambda s: sample("cem", co, s),
            "phnn_solve_mppi_shaped": lambda s: solve_("mppi", mo, s), "phnn_solve_cem_shaped": lambda s: solve_("cem", co, s)}, u


def test_argument_errors_and_the_null_shape(torch):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    eng = engine("phnn_cartpole")
    B, H, K = 2, 20, 4
    calls, u = _entry_points(torch, eng, B, H, K)
    good = holder(shape_of("ar1", H))
    for name, call in calls.items():
        for field, value in (("L_dev", None), ("rows", H + 1), ("rows", H - 1), ("cols", 0), ("cols", -1), ("cols", H + 1)):
            s = good.struct(eng.device)
            setattr(s, field, value)
            rc, outs = call(C.byref(s))
            torch.cuda.synchronize()
            msg = eng.lib.phnn_last_error(eng.h)
            assert rc == -1 and b"phnn_noise_shape" in msg, (name, field, value, rc, msg)
            for t in outs:  # nothing was launched: the pattern is still there (u of a solve: its input)
                want = u if t.shape == u.shape and t.dtype == u.dtype and bool((t != PATTERN).any()) else None
                if t.dtype == torch.uint8:
                    assert bool((t == 0x5A).all()), (name, field)
                elif want is not None:
                    assert torch.equal(t, want), (name, field)
                else:
                    assert bool((t == PATTERN).all()), (name, field)
        rc_null, out_null = call(None)  # shape = NULL: the old entry point, bit for bit
        rc_old, out_old = call("old")
        rc_good, out_good = call(C.byref(good.struct(eng.device)))
        torch.cuda.synchronize()
        assert rc_null == 0 and rc_old == 0 and rc_good == 0, (name, eng.lib.phnn_last_error(eng.h))
        assert all(torch.equal(a, b) for a, b in zip(out_null, out_old)), name
        assert not torch.equal(out_good[0], out_old[0]), name
    # the checks keep their order: the options' own errors come first, the width limit last
    x0 = torch.tensor(tm.states(2, 13), device="cuda")
    cost = cost_of(eng)
    with pytest.raises(PhnnError, match="samples"):
        eng.solve_mppi(x0, torch.zeros(2, 20, 1, device="cuda"), cost, "euler", 0.02, iters=1, samples=1, noise=holder(np.eye(19)))
    with pytest.raises(PhnnError, match="error -1.*rows"):  # H = 257 with a 256-row shape: the shape is refused before the width
        eng.solve_mppi(x0, torch.zeros(2, 257, 1, device="cuda"), cost, "euler", 0.02, iters=1, samples=4, noise=holder(np.eye(256)))
    with pytest.raises(PhnnError, match="error -2"):  # a matching shape: H * m > 256 is the refusal
        eng.solve_cem(x0, torch.zeros(2, 257, 1, device="cuda"), cost, "euler", 0.02, iters=1, samples=4, elites=2,
                      noise=holder(np.eye(257)))
    assert C.sizeof(_capi.NoiseShape) == 32


# ----------------------------------------------------------------------------- 6. footprint
class ShapedSampleOp(fp.SampleOp):
    """phnn_mppi_sample_shaped / phnn_cem_sample_shaped: SampleOp with L (H, P) as one more guarded input."""

    def __init__(self, which, cost, x0, U, rng, L, with_x0rep=True):
        super().__init__(which, cost, x0, U, rng, with_x0rep)
        self.name = "shaped " + self.name + f" P{L.shape[1]}"
        self.L = np.ascontiguousarray(L, dtype=np.float32)
        self.add("L", np.float32, self.L.shape, fp.IN, self.L)

    def _shape(self, p):
        from phnn_mpc_amd import _capi
        s = _capi.NoiseShape()
        s.L_dev, s.rows, s.cols = p["L"].value, self.L.shape[0], self.L.shape[1]
        return s

    def call(self, eng, p):
        s = self._shape(p)
        if self.which == "mppi":
            opt, _ = eng._mppi_options(0, fp.K_SAMPLES, 1.0, self.sigma, fp.SEED, 3, 5)
            fp.check_rc(eng, eng.lib.phnn_mppi_sample_shaped(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), C.byref(opt), 1,
                                                             C.byref(s), p["v"], p.get("x0_rep"), eng._stream()))
        else:
            opt, _ = eng._cem_options(0, fp.K_SAMPLES, 1, 0.0, 0.0, 0.0, fp.SEED, 3, 5)
            fp.check_rc(eng, eng.lib.phnn_cem_sample_shaped(eng.h, p["x0"], p["u"], p["sig"], self.B, self.H, C.byref(self.cost),
                                                            C.byref(opt), 1, C.byref(s), p["v"], p.get("x0_rep"), eng._stream()))

    def engine(self, eng):
        import torch
        shp = holder(self.L)
        if self.which == "mppi":
            v, xr = eng.mppi_sample(self.input("x0"), self.input("u"), self.cost, fp.K_SAMPLES, self.sigma, fp.SEED, 1, epoch=3,
                                    problem_offset=5, noise=shp)
        else:
            sig = torch.tensor(self.input("sig"), device=eng.device)
            v, xr = eng.cem_sample(self.input("x0"), self.input("u"), sig, self.cost, fp.K_SAMPLES, fp.SEED, 1, epoch=3,
                                   problem_offset=5, noise=shp)
        return {"v": v, "x0_rep": xr} if self.with_x0rep else {"v": v}


class ShapedSolveOp(fp.SampleSolveOp):
    """phnn_solve_mppi_shaped / phnn_solve_cem_shaped in a workspace of exactly the unshaped size."""

    def __init__(self, which, eng, cost, x0, U, integ, dt, L):
        super().__init__(which, eng, cost, x0, U, integ, dt)
        self.name = "shaped " + self.name + f" P{L.shape[1]}"
        self.L = np.ascontiguousarray(L, dtype=np.float32)
        self.add("L", np.float32, self.L.shape, fp.IN, self.L)

    _shape = ShapedSampleOp._shape

    def call(self, eng, p):
        s = self._shape(p)
        if self.which == "mppi":
            opt, _ = eng._mppi_options(self.iters, fp.K_SAMPLES, 0.7, self.sigma, fp.SEED, 3, 5)
            fp.check_rc(eng, eng.lib.phnn_solve_mppi_shaped(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), None, self.integ,
                                                            float(self.dt), C.byref(opt), C.byref(s), p["ws"], self.nws, p["costs"],
                                                            p["best_cost"], p["best_u"], eng._stream()))
        else:
            opt, _ = eng._cem_options(self.iters, fp.K_SAMPLES, fp.ELITES, 0.25, self.sigma, 0.05, fp.SEED, 3, 5)
            fp.check_rc(eng, eng.lib.phnn_solve_cem_shaped(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), None, self.integ,
                                                           float(self.dt), C.byref(opt), C.byref(s), p["ws"], self.nws, p["costs"],
                                                           p["best_cost"], p["best_u"], p["sigma_out"], eng._stream()))

    def engine(self, eng):
        name = {0: "euler", 1: "rk4"}[self.integ]
        kw = dict(iters=self.iters, samples=fp.K_SAMPLES, sigma=self.sigma, seed=fp.SEED, epoch=3, problem_offset=5, noise=holder(self.L))
        if self.which == "mppi":
            r = eng.solve_mppi(self.input("x0"), self.input("u"), self.cost, name, self.dt, lam=0.7, **kw)
        else:
            r = eng.solve_cem(self.input("x0"), self.input("u"), self.cost, name, self.dt, elites=fp.ELITES, alpha=0.25, sigma_min=0.05, **kw)
        out = {"u": r["u_last"], "costs": r["costs"], "best_cost": r["best_cost"], "best_u": r["best_u"]}
        if self.which == "cem":
            out["sigma_out"] = r["sigma_last"]
        return out


@pytest.mark.parametrize("which", ["mppi", "cem"])
@pytest.mark.parametrize("H, m, P", [(4, 1, 4), (13, 1, 5), (5, 2, 5), (5, 3, 2), (160, 1, 160)])
def test_footprint(torch, H, m, P, which):
    """The four new entry points on guarded buffers of exactly the documented sizes, L (H * P floats) between two guards:
    nothing outside the outputs is written, the inputs (L among them) are unchanged, and the outputs do not depend on what
    the guards around the inputs hold (0xFF: NaN to every float view) -- a read past L would show.  (160, 1, 160): L read
    from global memory; the others staged in LDS."""
    from test_gpu_footprint import SOLVE_MODEL
    rep = Report(f"shaped {which} H{H} m{m} P{P}")
    for B in (1, 19) if H < 100 else (3,):
        sid = SOLVE_MODEL[m]
        s = vc.CENSUS[sid]
        rng = rng_of("shaped", H, m, B)
        x0, U, cost = vc.states(rng, s["n"], B), vc.controls(rng, B, H, m), vc.cost_of(s, rng)
        from phnn_mpc_amd import noise
        L = noise.normalize_rows(rng.normal(size=(H, P)))
        eng = census_engine(sid)
        for with_x0rep in (True, False):
            footprint(rep, torch, eng, ShapedSampleOp(which, cost, x0, U, rng, L, with_x0rep))
        footprint(rep, torch, eng, ShapedSolveOp(which, eng, cost, x0, U, 0, vc.dt_of(s), L))
    rep.finish()


# ----------------------------------------------------------------------------- 7. one iteration against the float64 oracle
@pytest.mark.parametrize("model, integ, B, K, H", [("phnn_cartpole", "euler", 37, 64, 20), ("phnn_m2_fix", "rk4", 37, 30, 25)])
def test_iterations_against_the_float64_oracle(torch, model, integ, B, K, H):
    import mppi_model as mm
    import oracle_lib as ol
    eng = tm.engine(model)
    m, N = eng.m, H * eng.m
    cost = tm.make_cost(eng)
    shp = holder(shape_of("ar1", H))
    o64 = ol.OracleModel(tm.weights(model), "f64")
    x0 = torch.tensor(tm.states(B, 3), device="cuda")
    u = torch.zeros(B, H, m, device="cuda")
    sig, lam = tm.sigma_of(m), 25.0
    for it in range(2):
        un = tm.npy(u).reshape(B, N).copy()  # the device's nominal: every iteration is checked from it
        v, x0r = eng.mppi_sample(x0, u, cost, K, sig, SEED, it, noise=shp)
        s = eng.rollout_cost(x0r, v, cost, integ, 0.02)
        eng.mppi_update(u, v, s, lam, cost)
        vd = tm.npy(v).reshape(B * K, N)
        s64 = o64.rollout(tm.npy(x0r), vd.reshape(B * K, H, m), cost, integ, 0.02, grad=False, traj=False, nthreads=8)["cost"]
        r64 = mm.update(un, vd, s64, lam, np.float64, -10.0, 10.0)
        r32 = mm.update(un, vd, tm.npy(s), lam, np.float32, -10.0, 10.0)
        r64dev = mm.update(un, vd, tm.npy(s), lam, np.float64, -10.0, 10.0)
        allow7 = tm.ALLOW * np.abs(r32["u"] - r64dev["u"]).max(axis=1) + tm.ulp(r64["u"])
        bound = 2 * 1e-5 * np.abs(s64.reshape(B, K)).max(axis=1) / lam * np.abs(vd.reshape(B, K, N)).max(axis=(1, 2)) + allow7
        err = np.abs(tm.npy(u).reshape(B, N) - r64["u"]).max(axis=1)
        print(f"\n{model} {integ} it={it}: max |u_dev - u_64| = {err.max():.3e}, bound (min over problems) = "
              f"{bound.min():.3e}, worst err/bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound)
        # the samples themselves are the model's shaped samples
        v64 = sn.sample(un, sig, m, shp.L, SEED, 0, it, 0, K, -10.0, 10.0, np.float64)
        v32 = sn.sample(un, sig, m, shp.L, SEED, 0, it, 0, K, -10.0, 10.0, np.float32)
        assert np.abs(vd - v64).max() <= tm.allowance(v32, v64)


# ----------------------------------------------------------------------------- 8. closed loop
def test_device_closed_loop_equals_host_loop(torch):
    """256 plants x 30 control steps with ar1(0.9) noise: DeviceClosedLoop (graph and eager; the step counter is the noise
    epoch) == the run_mpc_batch host loop: controls bit for bit, states to 1e-12 (the closed-loop contract)."""
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
    from phnn_mpc_amd.noise import Noise
    rng = np.random.default_rng(12)
    X = rng.uniform(-1, 1, size=(256, 4)) * [0.2, 0.08, 0.1, 0.1]
    T = 30
    white = None
    for optimizer, make, cls, name in (("MPPI", create_mpc_from_config, pHNN, "phnn_cartpole"),
                                       ("CrossEntropy", create_mpc_controller, pHNN_Canonical, "canonical_cartpole")):
        cfg = yaml.safe_load(open(CFG))
        cfg["mpc"].update(optimizer=optimizer, samples=32, lam=20.0, sigma=3.0, seed=SEED, optimizer_steps=2, elites=6,
                          noise={"type": "ar1", "rho": 0.9})
        c = make(tm._load(cls, name, torch), cfg)
        assert isinstance(c.noise, Noise) and (c.noise.H, c.noise.P) == (c.horizon, c.horizon)
        host = run_mpc_batch(BatchedCartPole(0.02), c, X, T)
        assert len(np.unique(host["controls"][:, 0, 0])) > T // 4  # fresh noise at every step
        for use_graph in (False, True):
            dev = run_mpc_batch_device(c, X, T, use_graph=use_graph)
            assert np.array_equal(dev["controls"], host["controls"])
            assert np.allclose(dev["states"], host["states"], rtol=0, atol=1e-12)
            assert np.array_equal(dev["done_step"], host["done_step"])
        c.noise = None
        white = run_mpc_batch(BatchedCartPole(0.02), c, X[:8], 3)
        assert not np.array_equal(white["controls"], host["controls"][:3, :8])
