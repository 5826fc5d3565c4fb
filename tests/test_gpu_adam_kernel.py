"""K3 pinned on the device: k_adam and k_best_cost (phnn_adam_step) == the float32 model of tests/adam_model.py bit for
bit, phnn_solve against the float64 oracle end to end, and k_shift_controls against NumPy.

  step       u, exp_avg and exp_avg_sq as uint32, the state carried over steps 1 .. 30, then steps 1000 and 100000 (where
             pow(beta2, step) underflows and the bias correction becomes 1); every shape of SHAPES x every
             hyper-parameter set of HYPER; gradients with 0, -0, +-1e-30 (g^2 underflows), denormals, +-1e20 (g^2
             overflows: the update is 0), +-inf and NaN.  NaNs must sit in the same places, every other bit is compared.
  tracking   the same shapes and steps (default hyper-parameters) with cost / best_cost / best_u: ties with best_cost,
             NaN and +inf costs, NaN and +inf in best_cost, a clamp that is active on about half the entries (and
             off), best_u pre-filled with a sentinel pattern so that a row written without an improvement shows.
  solve      phnn_solve (64 problems, 20 iterations) against the float64 oracle driven through adam_model.solve: models
             with m = 2 and m = 4 control inputs, the canonical model with RK4, the soft state barrier, a per-problem
             reference trajectory.
  shift      phnn_shift_controls for m = 1 .. 4, H = 1 and 7, ragged B; the counter-only call; overlapping buffers are
             refused.

Measured on an MI355X: device == model held bit for bit in every case of the step and the tracking, without a
per-operation exception; none is made in here.
"""
import numpy as np
import pytest

import adam_model as am
import oracle_lib as ol

pytestmark = pytest.mark.gpu

# (B, H, m): count = B*H*m = 1; < 256; a multiple of 256; = 1 and 255 mod 256; m = 1 .. 4; per = H*m = 1; many blocks
SHAPES = [(1, 1, 1), (5, 1, 1), (3, 7, 1), (16, 16, 1), (257, 1, 1), (73, 7, 1), (8, 16, 2), (37, 3, 2), (17, 5, 3),
          (1, 171, 3), (64, 1, 4), (19, 9, 4), (4096, 5, 2), (65536, 50, 1)]
HYPER = {"defaults": {}, "beta1=0": {"beta1": 0.0}, "betas=(0.5,0.9)": {"beta1": 0.5, "beta2": 0.9}, "eps=1e-3": {"eps": 1e-3},
         "lr=1": {"lr": 1.0}}
STEPS = list(range(1, 31)) + [1000, 100000]
EDGE = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-40, -3e-45, 1e20, -1e20, np.inf, -np.inf, np.nan, 3e38, 1e-19, -1e-19],
                np.float32)
SCALES = [1.0, 1e-3, 30.0, 1e3, 1e-2]
assert [b * h * m % 256 for b, h, m in SHAPES[:6]] == [1, 5, 21, 0, 1, 255] and 17 * 5 * 3 == 255 and 171 * 3 % 256 == 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


_ENGINES = {}


def engine(name="phnn_cartpole"):
    from phnn_mpc_amd.engine import RolloutEngine
    if name not in _ENGINES:
        if name.startswith(("phnn_m", "canonical_m")):
            w = ol.load_named_golden("golden_m2.npz" if "_m2" in name else "golden_m34.npz")[1][name]
        else:
            w = ol.load_weights(name)
        _ENGINES[name] = (RolloutEngine(w, "cuda:0"), w)
    return _ENGINES[name]


def engine_with(m):
    """An engine whose model has m control inputs: phnn_adam_step is handed per = H*m, and a row index that went through
    the handle's own m instead would only show on a handle with that m."""
    return engine({1: "phnn_cartpole", 2: "phnn_m2_fix", 3: "phnn_m3_fix", 4: "phnn_m4_gnet"}[m])[0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(dev, model, what):
    """NaNs in the same places, every other entry equal as bits; reports the first differing entry."""
    dev, model = np.asarray(dev, np.float32).reshape(-1), np.asarray(model, np.float32).reshape(-1)
    nd, nm = np.isnan(dev), np.isnan(model)
    bad = (nd != nm) | (~nd & ~nm & (bits(dev) != bits(model)))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {dev.size} entries differ, first at {i}: device {dev[i]!r} "
                             f"(0x{bits(dev[i:i + 1])[0]:08x}) vs model {model[i]!r} (0x{bits(model[i:i + 1])[0]:08x})")


def gradients(rng, base, k):
    """Step k's gradient: the base array rolled and rescaled (cheap at 3.3 M entries), edge values at random places."""
    g = np.roll(base.reshape(-1), 7 * k) * np.float32(SCALES[k % len(SCALES)])
    pos = rng.integers(0, g.size, size=min(g.size, 4 * EDGE.size))
    g[pos] = np.resize(EDGE, pos.size)
    if g.size < EDGE.size:  # tiny shapes: walk through the edge values over the steps
        g[0] = EDGE[k % EDGE.size]
    return g.reshape(base.shape)


def hyper(name):
    """(what the device is called with, what the model is called with: the same values as the C ABI's floats)"""
    kw = dict(dict(lr=0.015, beta1=0.9, beta2=0.999, eps=1e-8), **HYPER[name])
    return kw, {k: am.float_arg(v) for k, v in kw.items()}


def dev_step(torch, eng, state, g, k, kw, track=None):
    """One phnn_adam_step on device copies of state (u, m, v[, best_cost, best_u]); -> the new state as NumPy arrays."""
    t = [torch.tensor(a, device="cuda") for a in state]
    extra = {}
    if track is not None:
        extra = dict(cost=torch.tensor(track["cost"], device="cuda"), best_cost=t[3], best_u=t[4], u_min=track["u_min"],
                     u_max=track["u_max"])
    eng.adam_step(t[0], torch.tensor(g, device="cuda"), t[1], t[2], kw["lr"], k, beta1=kw["beta1"], beta2=kw["beta2"],
                  eps=kw["eps"], **extra)
    return [x.cpu().numpy() for x in t]


# ----------------------------------------------------------------------------------------------- a. the step
def shape_id(s):
    return "x".join(map(str, s))


# every shape with B <= 4096 under every hyper-parameter set; the one full-size case under the defaults
STEP_CASES = [(s, h) for s in SHAPES for h in HYPER if s[0] <= 4096 or h == "defaults"]


@pytest.mark.parametrize("shape,hname", STEP_CASES, ids=[f"{shape_id(s)}-{h}" for s, h in STEP_CASES])
def test_adam_step_equals_the_model_bitwise(torch, shape, hname):
    eng = engine_with(shape[2])
    kw, mkw = hyper(hname)
    lr = mkw.pop("lr")
    rng = np.random.default_rng(sum(shape))
    u = rng.normal(size=shape).astype(np.float32)
    base = rng.normal(size=shape).astype(np.float32)
    m, v = np.zeros_like(u), np.zeros_like(u)
    for k in STEPS:
        g = gradients(rng, base, k)
        du, dm, dv = dev_step(torch, eng, (u, m, v), g, k, kw)
        u, m, v = (a.reshape(shape) for a in am.step(u, g, m, v, lr, k, **mkw))
        for d, ref, what in ((du, u, "u"), (dm, m, "exp_avg"), (dv, v, "exp_avg_sq")):
            assert_same_bits(d, ref, f"{what} after step {k} {shape} {hname}")
        if k == 30:  # the late steps start from a finite state again (by now inf / NaN gradients have spread)
            u = rng.normal(size=shape).astype(np.float32)
            m, v = (0.1 * rng.normal(size=shape)).astype(np.float32), (rng.normal(size=shape) ** 2).astype(np.float32)


def test_the_model_sees_the_c_abi_floats(torch):
    """phnn_adam_step takes lr, betas and eps as C floats: the kernel's Adam is torch's with betas (float(0.9f),
    float(0.999f)).  The model fed the Python doubles instead is NOT the device (lerp weight 3 ulp, 1 - beta2 110 ulp
    away); this keeps the distinction visible."""
    eng, _ = engine()
    kw, mkw = hyper("defaults")
    rng = np.random.default_rng(1)
    shape = (16, 16, 1)
    u, g = rng.normal(size=shape).astype(np.float32), rng.normal(size=shape).astype(np.float32)
    m, v = (0.1 * rng.normal(size=shape)).astype(np.float32), (rng.normal(size=shape) ** 2).astype(np.float32)
    du, dm, dv = dev_step(torch, eng, (u, m, v), g, 3, kw)
    lr = mkw.pop("lr")
    assert_same_bits(dm, am.step(u, g, m, v, lr, 3, **mkw)[1], "exp_avg")
    assert (bits(dm) != bits(am.step(u, g, m, v, 0.015, 3)[1])).any()


# ----------------------------------------------------------------------------------------------- b. the tracking
def sentinel(count):
    """A distinct finite float32 pattern per entry (0xC0000000 | index: -2.0 and below)."""
    assert count < 1 << 22
    return (np.uint32(0xC0000000) | np.arange(count, dtype=np.uint32)).view(np.float32)


def costs_for(rng, best_cost, k):
    """Step k's costs: about a third below best_cost, a third above, exact ties, NaN, +inf; B = 1 walks through them."""
    B = best_cost.size
    with np.errstate(invalid="ignore"):
        base = np.where(np.isfinite(best_cost), best_cost, np.float32(100.0)).astype(np.float32)
        c = (base * rng.choice(np.array([0.5, 0.999999, 1.0, 1.0, 1.000001, 2.0], np.float32), size=B)).astype(np.float32)
    kind = rng.integers(0, 12, size=B) if B > 1 else np.array([k % 12])
    c[kind == 0] = np.nan
    c[kind == 1] = np.inf
    c[kind == 2] = best_cost[kind == 2]  # exact tie, also inf == inf and NaN
    return c


# the table of the step test with the clamp on; with it off the full-size case gives way to a ragged multi-block one
TRACK_CASES = [(s, True) for s in SHAPES] + [(s, False) for s in SHAPES[:-1] + [(4093, 3, 4)]]


@pytest.mark.parametrize("shape,has_bounds", TRACK_CASES,
                         ids=[f"{shape_id(s)}-{'clamp' if b else 'noclamp'}" for s, b in TRACK_CASES])
def test_tracking_equals_the_model_bitwise(torch, shape, has_bounds):
    """All of STEPS, the state carried as in the step test, under the default hyper-parameters only: the tracking reads
    the iterate, the costs and the bounds, never a hyper-parameter, and the step it is fused with is compared again."""
    eng = engine_with(shape[2])
    assert eng.m == shape[2]
    kw, mkw = hyper("defaults")
    lr = mkw.pop("lr")
    B, per = shape[0], shape[1] * shape[2]
    rng = np.random.default_rng(sum(shape) + 1)
    u = rng.normal(size=shape).astype(np.float32)
    base = rng.normal(size=shape).astype(np.float32)
    m, v = np.zeros_like(u), np.zeros_like(u)
    best_cost = rng.choice(np.array([np.inf, np.inf, 50.0, 3.0, np.nan, 7.5], np.float32), size=B).astype(np.float32)
    best_cost[0] = np.inf  # row 0 can improve, row 1 (NaN) never does
    best_cost[1:2] = np.nan
    best_u = sentinel(u.size).reshape(shape).copy()
    lo, hi = (-0.5, 0.5) if has_bounds else (None, None)
    improved = ties = kept = 0
    for k in STEPS:
        g = gradients(rng, base, k)
        cost = costs_for(rng, best_cost, k)
        with np.errstate(invalid="ignore"):
            ties += int((cost == best_cost).sum())
        du, dm, dv, dbc, dbu = dev_step(torch, eng, (u, m, v, best_cost, best_u), g, k, kw,
                                        track=dict(cost=cost, u_min=lo, u_max=hi))
        prev = best_u.copy()
        better = am.track(u, cost, best_cost, best_u.reshape(-1), per, lo, hi, has_bounds)  # on the iterate before the step
        u, m, v = (a.reshape(shape) for a in am.step(u, g, m, v, lr, k, **mkw))
        for d, ref, what in ((du, u, "u"), (dm, m, "exp_avg"), (dv, v, "exp_avg_sq"), (dbc, best_cost, "best_cost"),
                             (dbu, best_u, "best_u")):
            assert_same_bits(d, ref, f"{what} after step {k} {shape}")
        assert_same_bits(dbu[~better], prev[~better], f"best_u rows without an improvement, step {k}")
        improved, kept = improved + int(better.sum()), kept + int((~better).sum())
        if k == 30:  # as in the step test: the late steps start from a finite state
            u = rng.normal(size=shape).astype(np.float32)
            m, v = (0.1 * rng.normal(size=shape)).astype(np.float32), (rng.normal(size=shape) ** 2).astype(np.float32)
    assert improved > 0 and (B == 1 or (kept > 0 and ties > 0))
    if B > 1:
        untouched = bits(best_u.reshape(B, per)[:, 0]) == bits(sentinel(u.size).reshape(B, per)[:, 0])
        assert untouched.any() and not untouched.all()  # NaN best_cost rows keep the sentinel to the end
        if has_bounds and B > 16:
            with np.errstate(invalid="ignore"):
                w = best_u.reshape(B, per)[~untouched]
                assert (np.abs(w) == 0.5).any() and (np.abs(w) < 0.5).any()


# ----------------------------------------------------------------------------------------------- c. the solve
B_SOLVE, H_SOLVE, ITERS, LR, DT = 64, 20, 20, 0.05, 0.02
GAP, MAX_SKIPPED = 2e-5, 0.10
SOLVE_CASES = ["m2", "m4", "canonical_rk4", "barrier", "x_ref"]


def solve_case(case):
    """-> dict(name, integ, cost, x0 (B,n) float32, u0 (B,H,m) float32, x_ref (B,H+1,n) float32 | None, u_lim)"""
    from phnn_mpc_amd import _capi
    name = {"m2": "phnn_m2_fix", "m4": "phnn_m4_gnet", "canonical_rk4": "canonical_cartpole"}.get(case, "phnn_cartpole")
    eng, _ = engine(name)
    n, m = eng.n, eng.m
    rng = np.random.default_rng(SOLVE_CASES.index(case) + 100)
    x0 = (rng.uniform(-1, 1, size=(B_SOLVE, n)) * np.array([0.5, 0.1, 0.3, 0.3])).astype(np.float32)
    # A warm start with about a quarter of the controls outside the clamp: those have zero gradient, stay where they are
    # and come back clamped in best_u.  The bounds are wide against the 20 * lr = 1.0 an entry can travel, because a
    # problem whose controls all saturate repeats its cost exactly and would drop out of the best-iterate comparison.
    lim = 2.0
    u0 = rng.uniform(-1.3 * lim, 1.3 * lim, size=(B_SOLVE, H_SOLVE, m)).astype(np.float32)
    R = [0.01 * (1 + i) for i in range(m)]
    kw = {}
    if case == "barrier":  # soft state bounds inside the range the start states cover: the barrier is on from t = 0
        kw = dict(x_min=[-0.3, -0.05, -0.2, -0.2], x_max=[0.3, 0.05, 0.2, 0.2], barrier_weight=1000.0)
    cost = _capi.make_cost(n, m, [10.0, 100.0, 1.0, 10.0], R, [0.0] * n, -lim, lim, **kw)
    x_ref = None
    if case == "x_ref":
        t = np.arange(H_SOLVE + 1)[None, :, None]
        amp = rng.uniform(-1, 1, size=(B_SOLVE, 1, n)) * np.array([0.3, 0.05, 0.2, 0.2])
        x_ref = (amp * np.cos(0.1 * t + rng.uniform(0, 6, size=(B_SOLVE, 1, n)))).astype(np.float32)
    return dict(name=name, integ="rk4" if case == "canonical_rk4" else "euler", cost=cost, x0=x0, u0=u0, x_ref=x_ref,
                u_lim=lim)


def oracle_cost_grad(model, c):
    """cost_grad(u) of adam_model.solve on the CPU oracle `model` (float32 or float64).  A reference trajectory enters
    in closed form (tests/test_gpu_tracking.py): C = C0 - sum_t r_t^T (Q + Q^T) x_t + sum_t r_t^T Q r_t with C0 the cost
    about x_target = 0, gradient = the oracle's VJP with traj_bar = -(Q + Q^T) r_t and cost_bar = 1."""
    cost, integ, x0 = c["cost"], c["integ"], c["x0"].astype(model.dtype)
    if c["x_ref"] is None:
        def f(u):
            r = model.rollout(x0, u, cost, integ, DT, grad=True, traj=False, nthreads=8)
            return r["cost"], r["grad_u"]
        return f
    n = model.n
    r_ = c["x_ref"].astype(np.float64)
    Q = np.array(cost.Q[:n * n], dtype=np.float64).reshape(n, n)
    Qs = Q + Q.T
    tb = -np.einsum("ij,btj->bti", Qs, r_)
    const = np.einsum("bti,ij,btj->b", r_, Q, r_)

    def f(u):
        ro = model.rollout(x0, u, cost, integ, DT, grad=False, traj=True, nthreads=8)
        C_ = ro["cost"] - np.einsum("bti,ij,btj->b", r_, Qs, ro["traj"].astype(np.float64)) + const
        gu, _ = model.rollout_vjp(x0, u, cost, integ, DT, traj_bar=tb, cost_bar=np.ones(len(x0)))
        return C_.astype(model.dtype), gu
    return f


def model_solve(w, c, precision):
    model = ol.OracleModel(w, precision)
    u0 = c["u0"].astype(model.dtype)
    hk = {k: am.float_arg(v) for k, v in dict(beta1=0.9, beta2=0.999, eps=1e-8).items()}
    return am.solve(oracle_cost_grad(model, c), u0, am.float_arg(LR), ITERS, track_best=True, u_min=-c["u_lim"],
                    u_max=c["u_lim"], **hk)


def compare_with_float64(out, ref, what):
    """out: a float32 solve (dict of NumPy arrays), ref: the float64 one.  Cost history and best_cost rtol 1e-5, u_last
    within 0.05 lr; where the float64 run's best and second-best costs are more than GAP apart (relative) the best
    iterate must be the same one and best_u within 0.05 lr; the other problems are skipped, at most MAX_SKIPPED of them.
    -> the share skipped."""
    costs, rc = out["costs"].astype(np.float64), ref["costs"]
    print(f"{what}: max cost rel err {np.abs(costs / rc - 1).max():.2e}, max |u_last - oracle| "
          f"{np.abs(out['u_last'] - ref['u_last']).max():.2e} (lr {LR}), max best_cost rel err "
          f"{np.abs(out['best_cost'] / ref['best_cost'] - 1).max():.2e}")
    assert np.allclose(costs, rc, rtol=1e-5, atol=0), np.abs(costs / rc - 1).max()
    assert np.abs(out["u_last"] - ref["u_last"]).max() <= 0.05 * LR
    assert np.allclose(out["best_cost"], ref["best_cost"], rtol=1e-5, atol=0)
    # the iterate best_u was taken from: the first minimum of the solve's own history (strict '<')
    assert np.array_equal(out["best_cost"], out["costs"].min(axis=0))
    # k_out is where the solve's own history has its first minimum, not something read out of best_u; that best_u was
    # taken at that iterate is what the 0.05 lr comparison with the oracle's best_u below establishes (one iterate
    # earlier or later moves every unclamped, still travelling entry by about lr).
    k_out, k_ref = out["costs"].argmin(axis=0), rc.argmin(axis=0)
    srt = np.sort(rc, axis=0)
    decided = (srt[1] - srt[0]) > GAP * np.abs(srt[0])
    skipped = 1.0 - decided.mean()
    du = np.abs(out["best_u"] - ref["best_u"]).reshape(len(k_ref), -1).max(axis=1)
    print(f"{what}: {100 * skipped:.1f} % of {len(k_ref)} problems skipped (best and second-best float64 costs within "
          f"{GAP} relative); best iterate index in [{k_ref.min()}, {k_ref.max()}]; max |best_u - oracle| on the others "
          f"{du[decided].max():.2e}")
    assert skipped <= MAX_SKIPPED, skipped
    assert np.array_equal(k_out[decided], k_ref[decided]), np.flatnonzero(decided & (k_out != k_ref))
    assert du[decided].max() <= 0.05 * LR
    return skipped


@pytest.mark.parametrize("case", SOLVE_CASES)
def test_solve_against_the_float64_oracle(torch, case):
    """phnn_solve, 64 problems x 20 iterations from a warm start, track_best with an active clamp, against the float64
    oracle driven through adam_model.solve.  The float32 CPU oracle is held to the same comparison first: the seeds and
    start states keep IT inside the cap on skipped problems, so a device failure is the device's.
    Share of problems skipped (float64 gap below 2e-5; it is a property of the float64 run, the same for any float32
    side): m2 0 %, m4 0 %, canonical_rk4 0 %, barrier 3.1 % (2 of 64), x_ref 0 %.  Measured on an MI355X: cost history
    within 1.9e-6 relative (barrier; 7e-7 elsewhere), best_cost within 1.2e-6, u_last and best_u within 4.8e-6 of the
    oracle's (allowed 0.05 lr = 2.5e-3); the float32 CPU oracle: 1.5e-6 and 9e-6."""
    c = solve_case(case)
    eng, w = engine(c["name"])
    ref = model_solve(w, c, "f64")
    compare_with_float64(model_solve(w, c, "f32"), ref, f"{case}: float32 oracle")
    d = dict(device="cuda")
    rk = {} if c["x_ref"] is None else {"x_ref": torch.tensor(c["x_ref"], **d)}
    out = eng.solve(torch.tensor(c["x0"], **d), torch.tensor(c["u0"], **d), c["cost"], c["integ"], DT, lr=LR, iters=ITERS,
                    track_best=True, record_costs=True, **rk)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    compare_with_float64(out, ref, f"{case}: device")
    lim = c["u_lim"]
    assert (np.abs(out["best_u"]) == lim).any() and (np.abs(out["best_u"]) < lim).any()  # the clamp is active, not everywhere


# ----------------------------------------------------------------------------------------------- d. the warm-start shift
@pytest.mark.parametrize("H", [1, 7])
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_shift_controls_equals_numpy(torch, m, H):
    eng, _ = engine()
    step = torch.full((1,), 41, dtype=torch.int32, device="cuda")
    calls = 0
    for B in (1, 37, 300):
        rng = np.random.default_rng(B + H + m)
        src = rng.normal(size=(B, H, m)).astype(np.float32)
        want = np.concatenate([src[:, 1:], np.zeros((B, 1, m), np.float32)], axis=1)
        s = torch.tensor(src, device="cuda")
        dst = torch.full((B, H, m), float("nan"), device="cuda")
        eng.shift_controls(s, dst, step_dev=step)
        calls += 1
        assert np.array_equal(bits(dst.cpu().numpy()), bits(want)) and np.array_equal(s.cpu().numpy(), src)
        assert int(step.item()) == 41 + calls
        eng.shift_controls(s, dst)  # without a counter
        assert np.array_equal(bits(dst.cpu().numpy()), bits(want)) and int(step.item()) == 41 + calls
    eng.advance_step(step)  # the counter-only call of the closed loop (B = 0)
    assert int(step.item()) == 41 + calls + 1


def test_shift_controls_refuses_overlapping_buffers(torch):
    """src == dst and every partial overlap: PHNN_ERR_INVALID_ARG (k_shift_controls reads src[idx + m] while another
    thread writes dst[idx]); nothing is written and the counter stays.  Adjacent buffers are fine."""
    from phnn_mpc_amd.engine import PhnnError
    eng, _ = engine()
    B, H, m = 5, 7, 2
    count = B * H * m
    pool = torch.arange(3 * count, dtype=torch.float32, device="cuda")
    keep = pool.clone()
    step = torch.zeros(1, dtype=torch.int32, device="cuda")

    def view(off):
        return pool[off:off + count].view(B, H, m)

    for so, do in ((0, 0), (0, 1), (1, 0), (0, count - 1), (count - 1, 0), (count // 2, 0)):
        with pytest.raises(PhnnError, match="error -1.*overlap"):
            eng.shift_controls(view(so), view(do), step_dev=step)
        assert torch.equal(pool, keep) and int(step.item()) == 0
    eng.shift_controls(view(0), view(count), step_dev=step)  # back to back: no shared byte
    want = np.concatenate([keep[:count].cpu().numpy().reshape(B, H, m)[:, 1:], np.zeros((B, 1, m), np.float32)], axis=1)
    assert np.array_equal(view(count).cpu().numpy(), want) and torch.equal(pool[:count], keep[:count])
    assert torch.equal(pool[2 * count:], keep[2 * count:]) and int(step.item()) == 1
