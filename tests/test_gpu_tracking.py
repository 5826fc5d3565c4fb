"""Reference tracking (phnn_reference; phnn_rollout_fwd_ref / phnn_rollout_grad_ref / phnn_solve_ref): every problem of
the batch is costed about its own, possibly time-varying, reference, row(t) = min(offset + t, rows - 1).

  setpoints   one solve with per-problem setpoints == separate solves whose phnn_cost.x_target is that setpoint, bitwise
  strides     stride-0 (shared) == materialised; ref_offset k == slicing x_ref[:, k:]; rows past the end hold the
              last row; a device offset == the same host offset -- bitwise
  identity    a reference equal to the cost's x_target == the non-tracking entry points, bitwise
  float64     a time-varying reference: cost and grad_u against the float64 oracle, unchanged (the reference terms
              are added in closed form), with the tolerances of test_gpu_parity.py
  closed loop 256 plants following their own moving references for 100 steps: device loop == host loop, graph
              replay == eager, bitwise controls

B in {1, 37, 4096}: with split='auto' all three run on the split-tile kernels where the variant has them (at most two
tiles per CU), with split='never' on the whole-tile ones.
"""
import ctypes as C
import os

import numpy as np
import pytest
import yaml

import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
MODELS = ["phnn_cartpole", "canonical_cartpole", "odefunc_pendulum"]
INTEGS = ["euler", "rk4"]
BATCHES = [1, 37, 4096]
SCALE = {4: np.array([1.0, 0.3, 0.5, 0.5]), 2: np.array([1.5, 0.8])}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


_ENGINES = {}


def engine(name, split):
    from phnn_mpc_amd.engine import RolloutEngine
    if (name, split) not in _ENGINES:
        _ENGINES[(name, split)] = RolloutEngine(ol.load_weights(name), "cuda:0", split=split)
    return _ENGINES[(name, split)]


def npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


def problem(torch, eng, g, B, H, seed, rows=None):
    """x0 (B,n), U (B,H,m) partly outside the control bounds, setpoints (B,n), a per-problem trajectory (B,rows,n)."""
    rng = np.random.default_rng(seed)
    n, umax = eng.n, float(g["u_max"])
    x0 = (rng.uniform(-1, 1, size=(B, n)) * SCALE[n]).astype(np.float32)
    U = rng.uniform(-1.3 * umax, 1.3 * umax, size=(B, H, eng.m)).astype(np.float32)
    targets = (rng.uniform(-1, 1, size=(B, n)) * 0.5 * SCALE[n]).astype(np.float32)
    rows = H + 1 if rows is None else rows
    t = np.arange(rows)[None, :, None]
    traj = (targets[:, None, :] * np.cos(0.1 * t + rng.uniform(0, 6, size=(B, 1, n)))).astype(np.float32)
    d = dict(device=eng.device)
    return (torch.tensor(x0, **d), torch.tensor(U, **d), torch.tensor(targets, **d), torch.tensor(traj, **d))


def cost_with(g, x_target):
    return ol.cost_from_golden(g, x_target=np.asarray(x_target, dtype=np.float64))


def sample(B):
    return list(range(B)) if B <= 37 else sorted({0, B - 1, *np.random.default_rng(B).choice(B, 14, replace=False).tolist()})


def solve(eng, g, x0, u0, cost, integ, **kw):
    return eng.solve(x0, u0, cost, integ, float(g["dt"]), lr=0.05, iters=4, track_best=True, record_costs=True, **kw)


def assert_same_solve(torch, a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in ("u_last", "best_u", "best_cost"):
        assert torch.equal(a[k][rows_a], b[k][rows_b]), k
    assert torch.equal(a["costs"][:, rows_a], b["costs"][:, rows_b]), "costs"


# ----------------------------------------------------------------------------------------------- setpoints, bitwise
@pytest.mark.parametrize("split", ["auto", "never"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("name", MODELS)
def test_setpoints_equal_separate_solves(torch, name, integ, B, split):
    eng, g = engine(name, split), ol.load_golden(name)
    H = 10
    x0, U, targets, _ = problem(torch, eng, g, B, H, seed=B)
    u0 = (0.2 * U).contiguous()
    out = solve(eng, g, x0, u0, cost_with(g, g["x_target"]), integ, x_ref=targets[:, None, :])
    for b in sample(B):
        one = solve(eng, g, x0[b:b + 1], u0[b:b + 1], cost_with(g, npy(targets[b])), integ)
        assert_same_solve(torch, out, one, slice(b, b + 1))


# ----------------------------------------------------------------------------------------------- strides, bitwise
@pytest.mark.parametrize("split", ["auto", "never"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("name", MODELS)
def test_strides_offsets_and_the_last_row(torch, name, integ, B, split):
    eng, g = engine(name, split), ol.load_golden(name)
    H, k = 12, 5
    cost, dt = cost_with(g, g["x_target"]), float(g["dt"])
    x0, U, _, traj = problem(torch, eng, g, B, H, seed=7 + B, rows=H + 1 + k)

    def run(x_ref, off=0):
        c, gu = eng.rollout_cost_grad(x0, U, cost, integ, dt, x_ref=x_ref, ref_offset=off)
        return c.clone(), gu.clone()

    def same(a, b):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])

    shared = traj[0]
    same(run(shared), run(shared.expand(B, -1, -1).contiguous()))  # stride 0 == materialised per problem
    same(run(traj[:, :1].expand(-1, H + 1, -1)), run(traj[:, :1]))  # constant rows: stride 0 == one row
    same(run(traj, k), run(traj[:, k:].contiguous()))  # ref_offset k == slicing
    off = torch.full((1,), k, dtype=torch.int32, device=eng.device)
    same(run(traj, off), run(traj, k))  # device offset == host offset
    short = traj[:, :4]  # rows past the end hold the last row
    padded = torch.cat([short, short[:, -1:].expand(-1, H + 1 - 4, -1)], dim=1)
    same(run(short), run(padded.contiguous()))
    same(run(short, 2), run(padded[:, 2:].contiguous()))
    same(run(short, 100), run(short[:, -1:]))  # an offset beyond the rows: the last row throughout
    wide = torch.zeros(B, H + 1 + k, 2 * eng.n, device=eng.device)  # non-contiguous last dimension (copied)
    wide[..., ::2] = traj
    same(run(wide[..., ::2]), run(traj))


# ----------------------------------------------------------------------------------------------- identity, bitwise
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("name", MODELS)
def test_reference_equal_to_x_target_is_bit_identical(torch, name, integ, B):
    g = ol.load_golden(name)
    for split in ("auto", "never"):
        eng = engine(name, split)
        xt = 0.3 * SCALE[eng.n] * np.array([1.0, -0.5, 0.25, 0.1][:eng.n])
        cost, dt, H = cost_with(g, xt), float(g["dt"]), 9
        x0, U, _, _ = problem(torch, eng, g, B, H, seed=11)
        r = torch.tensor(np.array(cost.x_target[:eng.n], dtype=np.float32), device=eng.device)
        for x_ref in (r, r.expand(B, H + 1, eng.n).contiguous()):
            c0, tr0 = eng.rollout_cost(x0, U, cost, integ, dt, want_traj=True)
            c1, tr1 = eng.rollout_cost(x0, U, cost, integ, dt, want_traj=True, x_ref=x_ref)
            assert torch.equal(c0, c1) and torch.equal(tr0, tr1)
            a = [t.clone() for t in eng.rollout_cost_grad(x0, U, cost, integ, dt, want_grad_x0=True)]
            b = eng.rollout_cost_grad(x0, U, cost, integ, dt, want_grad_x0=True, x_ref=x_ref)
            assert all(torch.equal(p, q) for p, q in zip(a, b))
            assert_same_solve(torch, solve(eng, g, x0, 0.2 * U, cost, integ),
                              solve(eng, g, x0, 0.2 * U, cost, integ, x_ref=x_ref))


# ----------------------------------------------------------------------------------------------- float64 oracle
@pytest.mark.parametrize("split", ["auto", "never"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("name", MODELS)
def test_time_varying_reference_against_float64(torch, name, integ, B, split):
    """C = C0 - sum_t r_t^T (Q + Q^T) x_t + sum_t r_t^T Q r_t with C0 the oracle's cost about x_target = 0; the gradient
    is the oracle's VJP with traj_bar = -(Q + Q^T) r_t, cost_bar = 1."""
    eng, g = engine(name, split), ol.load_golden(name)
    H, dt, n = 20, float(g["dt"]), eng.n
    x0, U, _, traj = problem(torch, eng, g, B, H, seed=3 * B + 1, rows=H + 4)
    k = 2
    cost0 = cost_with(g, np.zeros(n))
    c, gu = eng.rollout_cost_grad(x0, U, cost0, integ, dt, x_ref=traj, ref_offset=k)
    idx = sample(B) if B <= 37 else sample(B)[:16]
    m64 = ol.OracleModel(ol.load_weights(name), "f64")
    x0s, Us, r = npy(x0)[idx], npy(U)[idx], npy(traj)[idx][:, k:k + H + 1]
    assert r.shape[1] == H + 1
    Q = np.array(cost0.Q[:n * n], dtype=np.float64).reshape(n, n)
    Qs = Q + Q.T
    ref = m64.rollout(x0s, Us, cost0, integ, dt, grad=False, traj=True)
    X = ref["traj"]
    C = ref["cost"] - np.einsum("bti,ij,btj->b", r, Qs, X) + np.einsum("bti,ij,btj->b", r, Q, r)
    gu64, _ = m64.rollout_vjp(x0s, Us, cost0, integ, dt, traj_bar=-np.einsum("ij,btj->bti", Qs, r), cost_bar=np.ones(len(idx)))
    cg, gg = npy(c)[idx], npy(gu)[idx]
    assert np.allclose(cg, C, rtol=1e-5, atol=0), np.abs(cg / C - 1).max()
    gmax = np.abs(gu64).max(axis=(1, 2), keepdims=True)
    assert np.all(np.abs(gg - gu64) <= 1e-4 * gmax), (np.abs(gg - gu64) / gmax).max()


# ----------------------------------------------------------------------------------------------- closed loop
def _controllers(torch):
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
    cfg = yaml.safe_load(open(CFG))
    out = []
    for cls, name, make in ((pHNN, "phnn_cartpole", create_mpc_from_config),
                            (pHNN_Canonical, "canonical_cartpole", create_mpc_controller)):
        m = cls(CFG)
        m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights(name).items()})
        c = make(m, cfg)
        if hasattr(c, "optimizer_steps"):
            c.optimizer_steps = 6
        else:
            c.max_iterations = 6
        out.append(c)
    return out


def test_closed_loop_follows_moving_references(torch):
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch, run_mpc_batch_device
    B, T = 256, 100
    rng = np.random.default_rng(21)
    X0 = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.05, 0.1, 0.1]
    for c in _controllers(torch):
        H = c.horizon
        s = np.arange(T + H + 1)[None, :] * c.dt
        amp, w = rng.uniform(0.1, 0.4, size=(B, 1)), rng.uniform(0.5, 2.0, size=(B, 1))
        ref = np.zeros((B, T + H + 1, 4), np.float32)
        ref[:, :, 0], ref[:, :, 2] = amp * np.sin(w * s), amp * w * np.cos(w * s)
        ref_dev = torch.tensor(ref, device=c.engine.device)
        host = run_mpc_batch(BatchedCartPole(0.02), c, X0, T, x_ref=ref_dev)
        untracked = run_mpc_batch(BatchedCartPole(0.02), c, X0[:8], 3)
        assert not np.array_equal(untracked["controls"], host["controls"][:3, :8])  # the reference is in effect
        runs = [run_mpc_batch_device(c, X0, T, use_graph=ug, x_ref=ref_dev) for ug in (False, True)]
        for dev in runs:
            assert np.array_equal(dev["controls"], host["controls"])
            assert np.allclose(dev["states"], host["states"], rtol=0, atol=1e-9)
            assert np.array_equal(dev["done_step"], host["done_step"])
        assert np.array_equal(runs[0]["states"], runs[1]["states"])
        # a host-side step that slices the window equals the offset form (ref_offset = step)
        u_off = c.compute_control_batch(X0[:16].astype(np.float32), x_ref=ref_dev[:16], ref_offset=7) \
            if not hasattr(c, "control_batch") else c.control_batch(X0[:16].astype(np.float32), x_ref=ref_dev[:16], ref_offset=7)[0]
        u_sl = c.compute_control_batch(X0[:16].astype(np.float32), x_ref=ref_dev[:16, 7:]) \
            if not hasattr(c, "control_batch") else c.control_batch(X0[:16].astype(np.float32), x_ref=ref_dev[:16, 7:])[0]
        assert np.array_equal(u_off, u_sl)


def test_graphed_solve_tracks_the_reference(torch):
    """GraphedSolve copies the reference (and a device offset) into its static buffers per call: == the eager solve."""
    for c in _controllers(torch):
        rng = np.random.default_rng(5)
        B, H = 37, c.horizon
        X0 = (rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.05, 0.1, 0.1]).astype(np.float32)
        ref = torch.tensor(rng.uniform(-0.3, 0.3, size=(B, H + 9, 4)).astype(np.float32), device=c.engine.device)
        batch = (lambda **kw: c.optimize_control_batch(X0, **kw)) if hasattr(c, "control_batch") else \
            (lambda **kw: c.solve_batch(X0, record_costs=True, **kw))
        c.use_graph = False
        eager = [batch(x_ref=ref, ref_offset=k) for k in (0, 3)]
        c.use_graph = True
        off = torch.zeros(1, dtype=torch.int32, device=c.engine.device)
        for k in (0, 3):
            off.fill_(k)
            for o in (k, off):
                got = batch(x_ref=ref, ref_offset=o)
                for key in eager[k // 3]:
                    if eager[k // 3][key] is not None:
                        assert torch.equal(got[key], eager[k // 3][key]), key
        ref.mul_(0.5)  # updated in place: the next call sees it
        c.use_graph = False
        want = batch(x_ref=ref, ref_offset=3)
        c.use_graph = True
        assert torch.equal(batch(x_ref=ref, ref_offset=3)["u_last"], want["u_last"])
        c.use_graph = False


# ----------------------------------------------------------------------------------------------- argument checks
def test_argument_checks(torch):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import PhnnError
    name = "phnn_cartpole"
    eng, g = engine(name, "auto"), ol.load_golden(name)
    lib, B, H, n = eng.lib, 4, 5, eng.n
    cost = cost_with(g, g["x_target"])
    x0 = torch.zeros(B, n, device=eng.device)
    U = torch.zeros(B, H, 1, device=eng.device)
    r = torch.zeros(B, H + 1, n, device=eng.device)
    c = torch.empty(B, device=eng.device)
    p = C.c_void_p

    def fwd(ref):
        return lib.phnn_rollout_fwd_ref(eng.h, p(x0.data_ptr()), p(U.data_ptr()), B, H, C.byref(cost), ref, 0, 0.02,
                                        p(c.data_ptr()), None, None, None)

    def good():
        ref = _capi.Reference()
        ref.x_ref, ref.batch_stride, ref.time_stride, ref.rows = r.data_ptr(), (H + 1) * n, n, H + 1
        return ref

    assert fwd(C.byref(good())) == 0
    torch.cuda.synchronize()
    assert fwd(None) == -1 and b"NULL" in lib.phnn_last_error(eng.h)
    for field, value, word in (("x_ref", None, b"x_ref"), ("rows", 0, b"rows"), ("batch_stride", -4, b"stride"),
                               ("time_stride", -1, b"stride"), ("offset_host", -1, b"offset")):
        ref = good()
        setattr(ref, field, value)
        assert fwd(C.byref(ref)) == -1  # PHNN_ERR_INVALID_ARG
        assert word in lib.phnn_last_error(eng.h), (field, lib.phnn_last_error(eng.h))
        gu = torch.empty(B, H, 1, device=eng.device)
        tr = torch.empty(B, H + 1, n, device=eng.device)
        assert lib.phnn_rollout_grad_ref(eng.h, p(x0.data_ptr()), p(U.data_ptr()), B, H, C.byref(cost), C.byref(ref), 0,
                                         0.02, p(tr.data_ptr()), None, p(gu.data_ptr()), None, None) == -1
    # the Python surface
    with pytest.raises(ValueError):
        eng.rollout_cost(x0, U, cost, x_ref=torch.zeros(B + 1, H, n, device=eng.device))
    with pytest.raises(ValueError):
        eng.rollout_cost(x0, U, cost, x_ref=r, ref_offset=torch.zeros(1, device=eng.device))  # float32 offset
    with pytest.raises(PhnnError):
        eng.rollout_cost(x0, U, cost, x_ref=r, ref_offset=-1)
    with pytest.raises(PhnnError):
        eng.solve(x0, U, cost, x_ref=r, ref_offset=-2, iters=2)
