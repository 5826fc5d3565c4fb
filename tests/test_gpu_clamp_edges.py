"""The control clamp at its edges, on every kernel that has one: a NaN stays NaN, as in torch.clamp, and one-sided,
degenerate and NaN bounds.

The reference clamps with torch.clamp, the float64 C oracle with clampr and the numpy models of the sampling solves with
np.minimum(np.maximum()): all three pass a NaN on.  fminf(fmaxf(u, lo), hi) alone does not -- IEEE fmaxf(NaN, lo) is lo,
a NaN control would silently become u_min -- so every device clamp tests u == u first.  (K1 / K2 are covered by the
nan_control_clamped poison of tests/test_gpu_heterogeneous.py, the plant by tests/test_gpu_plant_edges.py.)

  samplers   mppi_sample, cem_sample and their shaped forms (AR(1) and L = I), B = 37, K = 30, N = 20 (the float4 path) and
             77 (the ragged tail), bounds +-10: a nominal with NaN at three entries of problems 0 and B - 1 (CEM: also NaN
             in sigma at other entries) gives NaN at exactly those entries of all K samples of those problems; every other
             entry has the bits of the run with those entries set to 0.
  updates    mppi_update with a NaN in one entry of finite-cost samples: that entry of the mean is NaN, every other entry
             has the bits of the run with a finite value there, and the whole mean is within test_gpu_mppi's allowance of
             the float64 model with equal NaN positions.  cem_update through test_gpu_cem.check_update against the
             float32 model, bit for bit: NaN in an elite row's entry (mean and sigma NaN there; in a non-elite row: no
             trace), in the incoming sigma, in the incoming mean; alpha = 0.25, sigma_min = 0.05, K = 15 and 64.
  solves     solve_mppi / solve_cem with a NaN in u_init: iters = 0 returns torch.clamp(u_init) bit for bit (the NaN kept)
             and best_cost = +inf; iters = 2 equals solver.mppi_solve / cem_solve over the primitives on the NaN problem
             too, and the other problems have the bits of the run without it.
  bounds     (lo, +inf), (-inf, hi), u_min == u_max and a bound of 0 through K1 / K2 (against the float64 oracle at the
             stated tolerances; pinned controls carry gradient exactly where they sit on the bound: the inclusive mask),
             the samplers and the plant (against torch.clamp); a NaN bound is refused with PHNN_ERR_INVALID_ARG.

Comparisons are of uint32 views with every NaN given one pattern (a NaN's sign and payload are no part of the models).
Where a bound is 0 and the input +-0 the comparison is by VALUE: torch.clamp(-0., 0., 10.) returns -0, and the sign of
zero fmaxf returns is not specified.
"""
import copy

import numpy as np
import pytest

import cem_model as cm
import heterogeneous as het
import mppi_model as mm
import oracle_lib as ol
import variant_census as vc
from test_gpu_cem import check_update, spread
from test_gpu_mppi import SEED, allowance, engine, make_cost, nominal, npy, states

pytestmark = pytest.mark.gpu
QNAN = np.uint32(0x7FC00000)
B, K = 37, 30
MODEL = "phnn_cartpole"  # m = 1: N = H


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def canon(a):
    """float32 array -> its uint32 view, every NaN as one quiet NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = QNAN
    return b


def same(a, b):
    return a.shape == b.shape and bool(np.array_equal(canon(a), canon(b)))


def noise_of(kind, H):
    from phnn_mpc_amd import noise
    if kind is None:
        return {}
    return {"noise": noise.Noise(noise.ar1(H, 0.9) if kind == "ar1" else np.eye(H, dtype=np.float32))}


# ----------------------------------------------------------------------------- samplers
@pytest.mark.parametrize("kind", [None, "ar1", "eye"])
@pytest.mark.parametrize("H", [20, 77])
def test_samplers_keep_a_nan_nominal_and_a_nan_sigma(torch, H, kind):
    eng = engine(MODEL)
    N = H
    cost = make_cost(eng)
    x0 = torch.tensor(states(B, 1), device="cuda")
    u = np.clip(nominal(B, H, 1, 2), -10, 10).reshape(B, N)
    sig = spread(B, N, 3)
    at_u = [(b, e) for b in (0, B - 1) for e in (1, N // 2, N - 1)]  # N - 1 = 76: the ragged tail's only element
    at_s = [(b, e) for b in (5, B - 1) for e in (0, N - 2)]
    kw = dict(epoch=11, problem_offset=1000, **noise_of(kind, H))

    def poisoned(a, at, value):
        a = a.copy()
        for b, e in at:
            a[b, e] = value
        return a

    def dev(a):
        return torch.tensor(a.reshape(B, H, 1), device="cuda")

    for meth in ("mppi", "cem"):
        at = at_u + (at_s if meth == "cem" else [])
        out = {}
        for name, value in (("nan", np.nan), ("clean", 0.0)):
            un = poisoned(u, at_u, value)
            if meth == "mppi":
                v, x0r = eng.mppi_sample(x0, dev(un), cost, K, 2.0, SEED, 3, **kw)
            else:
                v, x0r = eng.cem_sample(x0, dev(un), dev(poisoned(sig, at_s, value)), cost, K, SEED, 3, **kw)
            out[name] = npy(v).reshape(B, K, N).copy()
            assert np.array_equal(npy(x0r), np.repeat(npy(x0), K, axis=0))
        want = np.zeros((B, K, N), bool)
        for b, e in at:
            want[b, :, e] = True
        got = np.isnan(out["nan"])
        assert np.array_equal(got, want), (meth, "NaN at", np.argwhere(got != want)[:8].tolist())
        assert np.array_equal(canon(out["nan"])[~want], canon(out["clean"])[~want]), meth
        assert np.isfinite(out["clean"]).all() and (np.abs(out["clean"]) == 10.0).any()  # the clamp is on and active


# ----------------------------------------------------------------------------- updates
@pytest.mark.parametrize("H", [20, 77])
def test_mppi_update_keeps_a_nan_sample_entry(torch, H):
    eng = engine(MODEL)
    N, lam = H, 25.0
    cost = make_cost(eng)
    rng = np.random.default_rng(H)
    u = rng.uniform(-10, 10, size=(B, N)).astype(np.float32)
    v = rng.uniform(-12, 12, size=(B, K, N)).astype(np.float32)  # weighted means past the clamp in places
    v[1] = 11.0
    s = rng.uniform(1, 50, size=(B, K)).astype(np.float32)
    s[2, ::3], s[4, 1] = np.nan, np.inf
    at = [(0, 3, N - 1), (18, K - 1, 0), (B - 1, 0, 7)]  # (problem, sample, entry), all of finite cost
    assert all(np.isfinite(s[b, k]) for b, k, _ in at)

    def run(value):
        vv = v.copy()
        for b, k, e in at:
            vv[b, k, e] = value
        ud = torch.tensor(u.reshape(B, H, 1), device="cuda")
        best_cost = torch.full((B,), float("inf"), device="cuda")
        best_u = torch.zeros(B, H, 1, device="cuda")
        eng.mppi_update(ud, torch.tensor(vv.reshape(B * K, H, 1), device="cuda"), torch.tensor(s.reshape(-1), device="cuda"), lam,
                        cost, best_cost=best_cost, best_u=best_u)
        return npy(ud).reshape(B, N), npy(best_cost), vv

    got, bc, vn = run(np.nan)
    clean, bc0, _ = run(1.25)
    want = np.zeros((B, N), bool)
    for b, _, e in at:
        want[b, e] = True
    assert np.array_equal(np.isnan(got), want), np.argwhere(np.isnan(got) != want).tolist()
    assert np.array_equal(canon(got)[~want], canon(clean)[~want])
    assert np.array_equal(bc, bc0) and np.isfinite(clean).all() and (np.abs(clean) == 10.0).any()
    with np.errstate(invalid="ignore"):
        r64 = mm.update(u, vn.reshape(B * K, N), s.reshape(-1), lam, np.float64, -10.0, 10.0)["u"]
        r32 = mm.update(u, vn.reshape(B * K, N), s.reshape(-1), lam, np.float32, -10.0, 10.0)["u"]
    assert np.array_equal(np.isnan(r64), want) and np.array_equal(np.isnan(r32), want)
    tol = allowance(np.where(want, 0, r32), np.where(want, 0, r64))
    err = float(np.abs(got - r64)[~want].max())
    print(f"\nH={H}: mppi_update |dev - f64| = {err:.3e}, allowance = {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("K", [15, 64])
@pytest.mark.parametrize("H", [20, 77])
def test_cem_update_keeps_nan_samples_sigma_and_mean(torch, H, K):
    eng = engine(MODEL)
    N, nb, E, alpha, smin = H, 5, 8, 0.25, 0.05
    cost = make_cost(eng)
    rng = np.random.default_rng(100 * H + K)
    u = rng.uniform(-10, 10, size=(nb, N)).astype(np.float32)
    sig = spread(nb, N, K)
    v = rng.uniform(-12, 12, size=(nb * K, N)).astype(np.float32)
    s = rng.uniform(1, 50, size=(nb, K)).astype(np.float32)
    s[3, 1::4] = np.nan
    at = [(0, 3), (nb - 1, N - 1)]
    none = np.zeros((nb, N), bool)
    there = none.copy()
    for b, e in at:
        there[b, e] = True

    def check(name, uu, ss, vv, nan_u, nan_sig):
        for misalign in ((False, True) if N % 4 == 0 else (False,)):
            with np.errstate(invalid="ignore"):
                r = check_update(torch, eng, cost, uu, ss, vv, s.reshape(-1), E, alpha, smin, misalign, tag=(name, H, K, misalign),
                                 bits=canon)
            assert np.array_equal(np.isnan(r["u"]), nan_u) and np.array_equal(np.isnan(r["sig"]), nan_sig), name

    vv = v.copy()
    for b, e in at:  # the third-best row of the problem: an elite, not the best sample
        vv[b * K + cm.elite_order(s[b], E)[2], e] = np.nan
    non_elite = np.flatnonzero(~cm.elite_mask(s[2:3], E)[0] & np.isfinite(s[2]))[0]
    vv[2 * K + non_elite, 5] = np.nan  # leaves no trace
    check("elite sample", u, sig, vv, there, there)
    ss = sig.copy()
    uu = u.copy()
    for b, e in at:
        ss[b, e] = uu[b, e] = np.nan
    check("incoming sigma", u, ss, v, none, there)
    check("incoming mean", uu, sig, v, there, none)
    check("clean", u, sig, v, none, none)


# ----------------------------------------------------------------------------- solves
SOLVE_B, SOLVE_BAD, SOLVE_H = 19, 7, 20
SOLVES = {"mppi": dict(lam=25.0), "cem": dict(elites=8, alpha=0.25, sigma_min=0.05)}


@pytest.mark.parametrize("meth", ["mppi", "cem"])
def test_solves_keep_a_nan_initial_control(torch, meth):
    from phnn_mpc_amd import solver
    eng = engine(MODEL)
    cost = make_cost(eng)
    nb, bad, H = SOLVE_B, SOLVE_BAD, SOLVE_H
    x0 = torch.tensor(states(nb, 4), device="cuda")
    u0 = nominal(nb, H, 1, 5)  # past the clamp in places
    u0[bad, 3, 0] = 0.0
    un = u0.copy()
    un[bad, 3, 0] = np.nan
    u0, un = torch.tensor(u0, device="cuda"), torch.tensor(un, device="cuda")
    kw = dict(samples=K, sigma=2.0, seed=SEED, epoch=2, problem_offset=7, **SOLVES[meth])
    lib, loop = getattr(eng, "solve_" + meth), getattr(solver, meth + "_solve")

    out = lib(x0, un, cost, "euler", 0.02, iters=0, **kw)
    assert same(npy(out["u_last"]), npy(torch.clamp(un, -10.0, 10.0))) and bool(torch.isnan(out["u_last"][bad, 3, 0]))
    assert int(torch.isnan(out["u_last"]).sum()) == 1
    assert bool((out["best_cost"] == float("inf")).all()) and bool((out["best_u"] == 0).all())

    a = lib(x0, un, cost, "euler", 0.02, iters=2, **kw)
    b = loop(eng, x0, un, cost, "euler", 0.02, iters=2, **kw)
    clean = lib(x0, u0, cost, "euler", 0.02, iters=2, **kw)
    keep = het.others(nb, rows=(bad,))
    assert a.keys() == b.keys() == clean.keys()
    for k in a:
        x, y, z = (npy(t[k]).T if k == "costs" else npy(t[k]) for t in (a, b, clean))
        assert same(x, y), (k, "library loop against the Python loop")
        assert same(x[keep], z[keep]), (k, "the other problems against the run without the NaN")
        assert np.isfinite(z).all(), k
    assert same(npy(a["u_last"])[bad], npy(torch.clamp(un, -10.0, 10.0))[bad])  # no finite cost: the start is kept
    assert float(a["best_cost"][bad]) == float("inf") and bool(torch.isnan(a["costs"][:, bad]).all())
    assert not same(npy(clean["u_last"])[bad], npy(torch.clamp(u0, -10.0, 10.0))[bad])  # the clean problem does move


# ----------------------------------------------------------------------------- one-sided, degenerate and NaN bounds
INF = float("inf")
BOUNDS = [(-0.5, INF), (-INF, 1.0), (vc.U_MAX, vc.U_MAX), (0.0, 10.0), (-10.0, 0.0)]


def by_value(lo, hi):
    return lo == 0.0 or hi == 0.0


def bounded(cost, lo, hi, on=1):
    c = copy.deepcopy(cost)
    c.u_min, c.u_max, c.has_u_bounds = lo, hi, on
    return c


_ROLL = {}


def roll_setup():
    """One census spec, its engine, float64 oracle and the heterogeneous batch (B = 37, H = 6; about 10 % of the controls
    sit exactly on vc.U_MIN or vc.U_MAX); a copy of the controls with the ones on U_MIN replaced by -0 and +0 in turn."""
    if not _ROLL:
        from phnn_mpc_amd.engine import RolloutEngine
        sid = het.FAMILIES[0]
        s = vc.ALL_SPECS[sid][1]
        sd = vc.build_state_dict(sid, s)
        d = het.batch(sid, s)
        Uz = d["U"].copy()
        idx = np.argwhere(Uz == np.float32(vc.U_MIN))
        for i, (b, t, c) in enumerate(idx):
            Uz[b, t, c] = -0.0 if i % 2 else 0.0
        assert len(idx) >= 4 and np.signbit(Uz[Uz == 0]).any() and not np.signbit(Uz[Uz == 0]).all()
        _ROLL.update(s=s, d=d, Uz=Uz, eng=RolloutEngine(sd, "cuda:0", **vc.engine_kwargs(s)),
                     m64=ol.OracleModel(sd, "f64", activation=s["act"]))
    return _ROLL


@pytest.mark.parametrize("lo, hi", BOUNDS)
def test_bounds_through_k1_and_k2_against_the_float64_oracle(torch, lo, hi):
    """Cost, trajectory and both gradients at the stated tolerances, against the oracle's clampr (by value: nothing here
    compares bits, so the +-0 controls at a bound of 0 are covered).  grad_u is exactly 0 where the oracle's is -- err_rows
    asks g == 0 of a row whose reference is all 0, and the mask is checked entry by entry below."""
    r = roll_setup()
    s, d, eng, m64 = r["s"], r["d"], r["eng"], r["m64"]
    U = r["Uz"] if by_value(lo, hi) else d["U"]
    cost = bounded(d["cost"], lo, hi)
    inside = (U >= np.float32(lo)) & (U <= np.float32(hi))  # the inclusive pass-through mask
    assert inside.any() and not inside.all()
    if lo == hi:
        assert 0 < inside.sum() < 0.2 * inside.size and (U[inside] == np.float32(lo)).all()  # pinned: only ON the bound
    for integ in het.INTEGRATORS:
        ref = m64.rollout(d["x0"], U, cost, integ, d["dt"], nthreads=8)
        assert (ref["grad_u"][~inside] == 0).all() and (ref["grad_u"][inside] != 0).any()
        for stash in (True, False):
            eng.use_stash = stash
            try:
                ws = {}
                c, gu, gx = eng.rollout_cost_grad(d["x0"], U, cost, integ, d["dt"], want_grad_x0=True, workspace=ws)
                c, gu, gx, tr = npy(c), npy(gu), npy(gx), npy(ws["traj"])
            finally:
                eng.use_stash = True
            e = {"cost": vc.err_cost(c, ref["cost"]) / (vc.COST_RTOL * s["tol"]), "traj": vc.err_traj(tr, ref["traj"]) / s["tol"],
                 "grad_u": vc.err_rows(gu, ref["grad_u"]) / vc.grad_tol(s), "grad_x0": vc.err_rows(gx, ref["grad_x0"]) / vc.grad_tol(s)}
            print(f"\nbounds ({lo}, {hi}) {integ} stash={stash}: error / tolerance {e}")
            assert all(v <= 1.0 for v in e.values()), (integ, stash, e)
            assert (gu[~inside] == 0).all() and np.isfinite(gu).all()
            assert np.array_equal(gu != 0, ref["grad_u"] != 0)


@pytest.mark.parametrize("lo, hi", BOUNDS)
def test_bounds_in_the_samplers_against_torch_clamp(torch, lo, hi):
    """The bounded samplers == torch.clamp of the unbounded ones (the flag is a kernel argument, the arithmetic before the
    clamp is the same): as bits, except at a bound of 0, where -0 and +0 count as equal (see the module's note)."""
    eng = engine(MODEL)
    base = make_cost(eng)
    x0 = torch.tensor(states(B, 1), device="cuda")
    for H in (20, 77):
        u = nominal(B, H, 1, 2, lim=3.0)
        u[3, :4, 0] = [0.0, -0.0, lo if np.isfinite(lo) else -20.0, hi if np.isfinite(hi) else 20.0]  # +-0, on or far past a bound
        ud = torch.tensor(u, device="cuda")
        sg = torch.tensor(spread(B, H, 3).reshape(B, H, 1), device="cuda")
        for kind in (None, "ar1"):
            kw = dict(epoch=11, problem_offset=1000, **noise_of(kind, H))
            for sample in (lambda c: eng.mppi_sample(x0, ud, c, K, 2.0, SEED, 3, **kw)[0],
                           lambda c: eng.cem_sample(x0, ud, sg, c, K, SEED, 3, **kw)[0]):
                got = sample(bounded(base, lo, hi)).clone()
                want = torch.clamp(sample(bounded(base, lo, hi, on=0)).clone(), lo, hi)
                assert bool(torch.isfinite(want).all()) and bool((want == lo).any() or (want == hi).any())
                if by_value(lo, hi):
                    assert bool((got == want).all())
                else:
                    assert same(npy(got), npy(want)), (H, kind)


@pytest.mark.parametrize("lo, hi", BOUNDS)
def test_bounds_in_the_plant_against_torch_clamp(torch, lo, hi):
    """log_controls == torch.clamp(force) (by value at a bound of 0), the state against the numpy plant driven with the
    clamped forces (1e-13: the device's double-precision sin / cos, as in test_gpu_configs)."""
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.closed_loop import BatchedCartPole
    eng = engine(MODEL)
    nb, T = 19, 3
    rng = np.random.default_rng(8)
    init = rng.uniform(-1, 1, size=(nb, 4)) * [0.5, 0.1, 0.3, 0.3]
    forces = rng.uniform(-3, 3, size=(T, nb)).astype(np.float32)
    # +-0, +-inf where that side is bounded (an unbounded side passes it on: the plant would leave the reals), far past
    forces[:, :6] = [0.0, -0.0, INF if np.isfinite(hi) else 20.0, -INF if np.isfinite(lo) else -20.0, 20.0, -20.0]
    state = torch.tensor(init, dtype=torch.float64, device="cuda")
    logc = torch.zeros(T, nb, dtype=torch.float32, device="cuda")
    host = BatchedCartPole(0.02)
    host.reset(init)
    for t in range(T):
        a = torch.tensor(forces[t], device="cuda")
        eng.plant_step(_capi.Plant.default(0.02), state, a, 1, u_min=lo, u_max=hi, step=t, log_controls=logc)
        want = torch.clamp(a, lo, hi)
        assert bool(torch.isfinite(want).all())
        if by_value(lo, hi):
            assert bool((logc[t] == want).all())
        else:
            assert same(npy(logc[t]), npy(want))
        hs, _ = host.step(npy(want).astype(np.float64))
        assert np.allclose(state.cpu().numpy(), hs, rtol=0, atol=1e-13)


def test_a_nan_bound_is_refused(torch):
    """PHNN_ERR_INVALID_ARG (-1) from every entry point that takes bounds, before anything is launched."""
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    eng = engine(MODEL)
    nb, H = 4, 20
    x0 = torch.tensor(states(nb, 1), device="cuda")
    u = torch.zeros(nb, H, 1, device="cuda")
    sg = torch.ones(nb, H, 1, device="cuda")
    v = torch.zeros(nb * 4, H, 1, device="cuda")
    s = torch.ones(nb * 4, device="cuda")
    state = torch.zeros(nb, 4, dtype=torch.float64, device="cuda")
    nan = float("nan")
    for lo, hi in ((nan, 10.0), (-10.0, nan), (nan, nan), (1.0, -1.0)):
        cost = bounded(make_cost(eng), lo, hi)
        calls = [lambda: eng.rollout_cost(x0, u, cost, "euler", 0.02),
                 lambda: eng.rollout_cost_grad(x0, u, cost, "euler", 0.02),
                 lambda: eng.mppi_sample(x0, u, cost, 4, 1.0, 0, 0),
                 lambda: eng.cem_sample(x0, u, sg, cost, 4, 0, 0),
                 lambda: eng.mppi_update(u.clone(), v, s, 1.0, cost),
                 lambda: eng.cem_update(u.clone(), sg.clone(), v, s, 2, 0.25, 0.05, cost),
                 lambda: eng.solve(x0, u, cost, "euler", 0.02, iters=1),
                 lambda: eng.solve_mppi(x0, u, cost, "euler", 0.02, iters=1, samples=4),
                 lambda: eng.solve_cem(x0, u, cost, "euler", 0.02, iters=1, samples=4, elites=2),
                 lambda: eng.plant_step(_capi.Plant.default(), state, u, H, u_min=lo, u_max=hi)]
        for i, call in enumerate(calls):
            with pytest.raises(PhnnError, match="error -1"):
                call()
            assert i >= 0
    torch.cuda.synchronize()
    assert bool((state == 0).all())
