"""CPU tests (no GPU) of the stated-order Gauss-Newton kernels (tests/gn_model.py, what k_gn_direction, k_gn_candidates
and k_gn_select are pinned against), and of the whole solve (solver.gn_solve) and the controllers' routing on the
oracle-backed engine.

Bounds.  On linear-quadratic data with mu = 0 one Gauss-Newton step is the exact minimiser; two float64 orderings of a
well-conditioned solve differ by rounding only, a wrong formula by O(1).  Each bound is the worst figure measured on
the test's own inputs (printed by the test; DESIGN.md section 18 repeats them) times 64, and never above 1e-8:
  u + du against the dense condensed-QP minimiser, worst of the nine (n, m, H) cases, relative to max|u*|: 3.1e-15 -> 2.0e-13
  -dV against g . du (g the dense gradient at u), relative:                                               6.4e-16 -> 4.1e-14
  predicted change -dV/2 against the true change of the quadratic cost at alpha = 1, relative:            1.2e-15 -> 7.7e-14
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gn_model as gm
import oracle_lib as ol
import tvlqr_model as tm
import variant_census as vc
from phnn_mpc_amd import _capi, solver
from phnn_mpc_amd.models import pHNN, pHNN_Canonical
from phnn_mpc_amd.mpc_controller import MPCController
from phnn_mpc_amd.mpc_controller_canonical import MPCControllerCanonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")

MARGIN, CEILING = 64.0, 1e-8
MEASURED_U, MEASURED_SLOPE, MEASURED_PRED = 3.1e-15, 6.4e-16, 1.2e-15
SHAPES = vc.NM_PAIRS  # every (n, m) a handle can have
HORIZONS = [1, 6, 50]
NB = 5


def bound(measured):
    return min(MARGIN * measured, CEILING)


def seed_of(n, m, H):
    return 1000 * n + 100 * m + H


def flat_gradients(nb, H, n, m, Lxx):
    """No barrier, lx = lu = 0: the cost gradients direction_core takes, given directly."""
    return np.broadcast_to(np.diag(Lxx), (nb, H + 1, n)).copy(), np.zeros((nb, H + 1, n)), np.zeros((nb, H, m))


# ----------------------------------------------------------------------------- against tvlqr_model
@pytest.mark.parametrize("H", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_zero_gradients_give_the_gains_of_tvlqr_bit_for_bit(n, m, H):
    A, Bm, Q, R = tm.seeded_problem(seed_of(n, m, H), NB, H, n, m)
    Lxx, Luu = tm.cost_matrices(Q, R, n, m)
    for mu in (0.0, 0.125):
        ref = tm.tvlqr(A, Bm, Lxx, Luu, mu)
        r = gm.direction_core(A, Bm, Lxx, Luu, *flat_gradients(NB, H, n, m, Lxx), mu)
        assert np.array_equal(r["status"], ref["status"]) and not r["status"].any()
        assert tm.same_floats(r["K"], ref["K"]) and tm.same_floats(r["P"], ref["P"])
        assert np.all(r["du"] == 0) and np.all(r["du64"] == 0) and np.all(r["dV"] == 0)


# ----------------------------------------------------------------------------- exact minimiser on linear-quadratic data
def lq_problem(n, m, H):
    """A seeded LTV system rolled out by itself in float64 from a seeded x0 under seeded controls, and the dense
    (condensed) form of its quadratic cost: x = Phi x0 + Gam U stacked over t = 0 .. H."""
    A, Bm, Q, R = tm.seeded_problem(seed_of(n, m, H) + 7, NB, H, n, m)
    Lxx, Luu = tm.cost_matrices(Q, R, n, m)
    rng = np.random.default_rng(seed_of(n, m, H) + 8)
    x0 = rng.uniform(-1, 1, size=(NB, n))
    U = rng.uniform(-1, 1, size=(NB, H, m))
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    X = np.empty((NB, H + 1, n))
    X[:, 0] = x0
    for t in range(H):
        X[:, t + 1] = np.einsum("bij,bj->bi", A64[:, t], X[:, t]) + np.einsum("bij,bj->bi", B64[:, t], U[:, t])
    dense = []
    for b in range(NB):
        Phi = np.zeros(((H + 1) * n, n))
        Gam = np.zeros(((H + 1) * n, H * m))
        Phi[:n] = np.eye(n)
        for t in range(H):
            Phi[(t + 1) * n:(t + 2) * n] = A64[b, t] @ Phi[t * n:(t + 1) * n]
            Gam[(t + 1) * n:(t + 2) * n] = A64[b, t] @ Gam[t * n:(t + 1) * n]
            Gam[(t + 1) * n:(t + 2) * n, t * m:(t + 1) * m] += B64[b, t]
        Qs, Rs = np.kron(np.eye(H + 1), Lxx), np.kron(np.eye(H), Luu)  # the cost is 1/2 (x^T Qs x + u^T Rs u)
        Hs = Gam.T @ Qs @ Gam + Rs
        u = U[b].reshape(-1)
        g = Gam.T @ Qs @ (Phi @ x0[b] + Gam @ u) + Rs @ u
        dense.append((Hs, g))
    return A, Bm, Lxx, Luu, X, U, dense


@pytest.mark.parametrize("H", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_one_step_is_the_exact_minimiser_of_a_linear_quadratic_problem(n, m, H):
    A, Bm, Lxx, Luu, X, U, dense = lq_problem(n, m, H)
    # the cost gradients in float64, given directly: lx = Lxx x_t, lu = Luu u_t
    ldiag = np.broadcast_to(np.diag(Lxx), (NB, H + 1, n)).copy()
    lx, lu = np.einsum("ij,btj->bti", Lxx, X), np.einsum("ij,btj->bti", Luu, U)
    r = gm.direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, 0.0)
    assert not r["status"].any()
    eu = es = ep = 0.0
    for b, (Hs, g) in enumerate(dense):
        u = U[b].reshape(-1)
        star = u - np.linalg.solve(Hs, g)
        du = r["du64"][b].reshape(-1)
        eu = max(eu, np.abs(u + du - star).max() / np.abs(star).max())
        es = max(es, abs(-r["dV"][b] - g @ du) / abs(g @ du))
        change = g @ du + 0.5 * du @ Hs @ du  # of 1/2 (x^T Qs x + u^T Rs u), the cost the gradients above belong to
        ep = max(ep, abs(-0.5 * r["dV"][b] - change) / abs(change))
        assert r["dV"][b] > 0
    print(f"\n(n={n}, m={m}, H={H}): u + du {eu:.2e}, slope {es:.2e}, predicted change {ep:.2e} relative")
    assert eu <= bound(MEASURED_U) and es <= bound(MEASURED_SLOPE) and ep <= bound(MEASURED_PRED)
    # the float32 output is that step rounded once
    assert np.array_equal(r["du"], r["du64"].astype(np.float32))


# ----------------------------------------------------------------------------- failure semantics
def _case(n, m, H, seed=3, nb=3):
    A, Bm, Q, R = tm.seeded_problem(seed, nb, H, n, m)
    rng = np.random.default_rng(seed + 1)
    traj = rng.uniform(-1, 1, size=(nb, H + 1, n)).astype(np.float32)
    u = rng.uniform(-1, 1, size=(nb, H, m)).astype(np.float32)
    return A, Bm, Q, R, traj, u


def check_failed(r, clean, b, status):
    assert r["status"][b] == status
    assert np.all(r["du"][b] == 0) and np.isnan(r["dV"][b])
    for o in range(r["du"].shape[0]):
        if o != b:
            assert r["status"][o] == 0 and tm.same_floats(r["du"][o], clean["du"][o]) and r["dV"][o] == clean["dV"][o]
            assert np.isfinite(r["dV"][o]) and np.any(r["du"][o] != 0)


@pytest.mark.parametrize("n,m", SHAPES)
def test_failure_semantics(n, m):
    H = 6
    A, Bm, Q, R, traj, u = _case(n, m, H)
    cost = _capi.make_cost(n, m, Q, R)
    clean = gm.direction(A, Bm, traj, u, cost, n, m, 0.0)
    assert not clean["status"].any() and np.isfinite(clean["dV"]).all()
    # NaN in A_t reaches the pivot of step t - 1; in B_t the pivot of step t: the status of tvlqr_model
    for what, t, status in (("A", 3, 3), ("B", 2, 3)):
        A1, B1 = A.copy(), Bm.copy()
        (A1 if what == "A" else B1)[1, t, 0, 0] = np.nan
        r = gm.direction(A1, B1, traj, u, cost, n, m, 0.0)
        assert np.array_equal(r["status"], tm.tvlqr(A1, B1, *tm.cost_matrices(Q, R, n, m))["status"])
        check_failed(r, clean, 1, status)
    # NaN in A_0 enters no pivot, NaN in a trajectory row none either: status 0, and still no step.  (Row 0 is the fixed
    # initial state: its cost gradient reaches p_0 only, which no control reads -- on the device a NaN x_0 comes with a
    # NaN A_0.)
    A1 = A.copy()
    A1[1, 0, 0, 0] = np.nan
    check_failed(gm.direction(A1, Bm, traj, u, cost, n, m, 0.0), clean, 1, 0)
    for row in (1, 2, H):
        t1 = traj.copy()
        t1[1, row, n - 1] = np.nan
        check_failed(gm.direction(A, Bm, t1, u, cost, n, m, 0.0), clean, 1, 0)
    u1 = u.copy()
    u1[1, 4, 0] = np.nan
    check_failed(gm.direction(A, Bm, traj, u1, cost, n, m, 0.0), clean, 1, 0)
    # a negative definite R fails every problem at the last step
    bad = _capi.make_cost(n, m, Q, -R - np.eye(m, dtype=np.float32))
    r = gm.direction(A, Bm, traj, u, bad, n, m, 0.0)
    assert (r["status"] == H).all() and np.all(r["du"] == 0) and np.isnan(r["dV"]).all()
    # and a large enough mu repairs it
    r = gm.direction(A, Bm, traj, u, bad, n, m, 50.0)
    assert not r["status"].any() and np.isfinite(r["dV"]).all()


# ----------------------------------------------------------------------------- barrier
def test_barrier_changes_lxx_and_lx_as_stated_and_an_inactive_one_leaves_the_bits():
    n, m, H = 4, 1, 6
    A, Bm, Q, R, traj, u = _case(n, m, H, seed=9)
    plain = _capi.make_cost(n, m, Q, R)
    wide = _capi.make_cost(n, m, Q, R, x_min=[-5.0] * 4, x_max=[5.0] * 4)  # never active: |x| <= 1
    a, b = gm.direction(A, Bm, traj, u, plain, n, m, 1e-3), gm.direction(A, Bm, traj, u, wide, n, m, 1e-3)
    for k in ("du", "dV", "K", "k", "P"):
        assert tm.same_floats(a[k], b[k]), k
    lo, hi = [-5.0, -0.25, -5.0, -5.0], [5.0, 5.0, 0.5, 5.0]
    cost = _capi.make_cost(n, m, Q, R, x_min=lo, x_max=hi, barrier_weight=1000.0)
    ldiag, lx, lu = gm.gradients(traj, u, cost, n, m)
    l0, x0_, _ = gm.gradients(traj, u, plain, n, m)
    Lxx, _ = tm.cost_matrices_of(cost, n, m)
    x = traj.astype(np.float64)
    below, above = (np.float64(np.float32(-0.25)) - x[:, :, 1]) > 0, (x[:, :, 2] - np.float64(np.float32(0.5))) > 0
    assert below.any() and above.any() and not below.all() and not above.all()
    assert np.array_equal(ldiag[:, :, 1], np.where(below, Lxx[1][1] + 2000.0, Lxx[1][1]))
    assert np.array_equal(ldiag[:, :, 2], np.where(above, Lxx[2][2] + 2000.0, Lxx[2][2]))
    assert np.array_equal(ldiag[:, :, 0], l0[:, :, 0]) and np.array_equal(ldiag[:, :, 3], l0[:, :, 3])
    assert np.array_equal(lx[:, :, 1], np.where(below, x0_[:, :, 1] - 2000.0 * (np.float64(np.float32(-0.25)) - x[:, :, 1]), x0_[:, :, 1]))
    assert np.array_equal(lx[:, :, 2], np.where(above, x0_[:, :, 2] + 2000.0 * (x[:, :, 2] - np.float64(np.float32(0.5))), x0_[:, :, 2]))
    assert np.array_equal(lx[:, :, 0], x0_[:, :, 0]) and np.array_equal(lx[:, :, 3], x0_[:, :, 3])
    r = gm.direction(A, Bm, traj, u, cost, n, m, 1e-3)
    assert not r["status"].any() and not tm.same_floats(r["du"], a["du"])


def test_reference_rows_replace_the_target():
    n, m, H = 2, 1, 4
    A, Bm, Q, R, traj, u = _case(n, m, H, seed=13)
    target = np.array([0.25, -0.5], np.float32)
    cost = _capi.make_cost(n, m, Q, R, x_target=target)
    a = gm.direction(A, Bm, traj, u, cost, n, m, 0.0)
    b = gm.direction(A, Bm, traj, u, _capi.make_cost(n, m, Q, R), n, m, 0.0, ref=gm.reference_rows(target, 0, H, 3, n))
    assert tm.same_floats(a["du"], b["du"]) and tm.same_floats(a["dV"], b["dV"])
    ref = np.arange(3 * 3 * n, dtype=np.float32).reshape(3, 3, n)
    rows = gm.reference_rows(ref, 1, H, 3, n)  # rows 1, 2, then the last one held; an offset past the end is clamped
    assert np.array_equal(rows[:, 0], ref[:, 1]) and np.array_equal(rows[:, 1], ref[:, 2]) and np.array_equal(rows[:, H], ref[:, 2])
    assert np.array_equal(gm.reference_rows(ref, 99, H, 3, n)[:, 0], ref[:, 2])


# ----------------------------------------------------------------------------- candidates and select
def test_candidates_are_exact_power_of_two_steps_clamped():
    cost = _capi.make_cost(2, 1, [1.0, 1.0], 0.1, u_min=-1.0, u_max=1.0)
    tiny = np.float32(3 * 2.0 ** -149)  # subnormal: halving rounds to even
    u = np.array([[[0.5], [0.0], [np.nan], [0.9]]], np.float32)
    du = np.array([[[1.0], [tiny], [1.0], [np.inf]]], np.float32)
    L = 4
    v = gm.candidates(u, du, L, cost).reshape(L, 4)
    assert np.array_equal(v[:, 0], np.float32([1.0, 1.0, 0.75, 0.625]))  # 1.5 clamped
    assert np.array_equal(v[:, 1], np.float32([3, 2, 1, 0]) * np.float32(2.0 ** -149))  # 1.5 -> 2, 0.75 -> 1, 0.375 -> 0
    assert np.isnan(v[:, 2]).all() and np.array_equal(v[:, 3], np.float32([1.0] * 4))
    # for a normal du whose scaled value stays normal, alpha_j * du is exact
    rng = np.random.default_rng(0)
    d = rng.normal(size=(3, 5, 2)).astype(np.float32)
    free = _capi.make_cost(2, 2, [1.0, 1.0], [0.1, 0.1])
    c = gm.candidates(np.zeros_like(d), d, 32, free).reshape(3, 32, 5, 2)
    for j in range(32):
        assert np.array_equal(c[:, j].astype(np.float64), d.astype(np.float64) * 2.0 ** -j)
    assert np.array_equal(gm.alphas(32).astype(np.float64), 2.0 ** -np.arange(32.0))


def _select(s, cost_b, status, mu, **kw):
    nb, L = s.shape
    u, traj = np.zeros((nb, 2, 1), np.float32), np.zeros((nb, 3, 2), np.float32)
    cand = np.arange(nb * L * 2, dtype=np.float32).reshape(nb * L, 2, 1) + 1
    ctraj = -np.arange(nb * L * 6, dtype=np.float32).reshape(nb * L, 3, 2) - 1
    opt = dict(mu_min=1e-3, mu_max=10.0, mu_up=10.0, mu_down=0.1)
    opt.update(kw)
    r = gm.select(u, traj, np.float32(cost_b), np.float64(mu), np.zeros(nb, np.int32), cand, s, ctraj, np.int32(status), L, **opt)
    return r, cand.reshape(nb, L, 2, 1), ctraj.reshape(nb, L, 3, 2)


def test_select_ties_non_finite_status_and_mu_saturation():
    inf, nan = np.inf, np.nan
    s = np.float32([[3.0, 1.0, 1.0, 2.0],     # a tie: the lowest j
                    [nan, inf, -inf, nan],    # nothing finite: reject
                    [1.0, 0.5, 0.25, 0.125],  # status != 0: reject
                    [5.0, 5.0, 5.0, 5.0],     # equal to the current cost: strict '<' rejects
                    [nan, 4.0, inf, 4.5],     # the lowest finite
                    [0.0, -0.0, 1.0, 1.0]])   # -0 == +0: j = 0
    r, cand, ctraj = _select(s, [2.0, 2.0, 2.0, 5.0, 5.0, 1.0], [0, 0, 2, 0, 0, 0], [1.0, 1.0, 5.0, 5e-3, 5e-3, 1.0])
    assert list(r["accepts"]) == [1, 0, 0, 0, 1, 1]
    assert list(r["alpha_row"]) == [0.5, 0.0, 0.0, 0.0, 0.5, 1.0]
    assert list(r["cost"]) == [1.0, 2.0, 2.0, 5.0, 4.0, 0.0] and list(r["costs_row"]) == [2.0, 2.0, 2.0, 5.0, 5.0, 1.0]
    for b, j in ((0, 1), (4, 1), (5, 0)):
        assert np.array_equal(r["u"][b], cand[b, j]) and np.array_equal(r["traj"][b], ctraj[b, j])
    for b in (1, 2, 3):
        assert not r["u"][b].any() and not r["traj"][b].any()
    # mu: times mu_down on accept with floor mu_min, times mu_up on reject with cap mu_max
    assert list(r["mu"]) == [1.0 * 0.1, 10.0, 10.0, 5e-3 * 10.0, 1e-3, 1.0 * 0.1]
    # a NaN current cost never accepts
    r, _, _ = _select(np.float32([[1.0, 2.0]]), [nan], [0], [1.0])
    assert r["accepts"][0] == 0 and np.isnan(r["cost"][0])


# ----------------------------------------------------------------------------- the whole solve on the CPU
class Recording(gm.GnOracleEngine):
    """Keeps (u before, u after, alpha row) of every gn_select and every candidate tensor."""

    def __init__(self, w):
        super().__init__(w)
        self.steps, self.cands = [], []

    def gn_candidates(self, *a, **k):
        out = super().gn_candidates(*a, **k)
        self.cands.append(out[0].clone())
        return out

    def gn_select(self, u, *a, **k):
        before = u.clone()
        super().gn_select(u, *a, **k)
        row = k.get("alpha_row")
        self.steps.append((before, u.clone(), None if row is None else row.clone()))


def _model(cls, name):
    w = ol.load_weights(name)
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    eng = Recording(w)
    return m.set_engine(eng), eng


X0 = (np.array([[0.3, 0.1, 0.2, -0.1], [-0.5, 0.05, -0.3, 0.2], [0.1, -0.15, 0.4, 0.3], [0.8, 0.19, -0.2, -0.4]]).astype(np.float32))


def _check_solve(eng, cost, m, u_lim):
    B, H, L, iters = 4, 10, 4, 6
    x0 = torch.tensor(X0)
    u0 = torch.zeros(B, H, m)
    u0[3] = 3.0 * u_lim  # starts outside the bounds: the set-up clamps it
    out = solver.gn_solve(eng, x0, u0, cost, "euler", 0.02, iters, line_steps=L, mu_init=1e-6)
    costs = out["costs"].numpy()
    assert costs.shape == (iters, B) and np.isfinite(costs).all()
    chain = np.vstack([costs, out["cost"].numpy()[None]])
    assert np.all(chain[1:] <= chain[:-1]), "the cost of a problem never rises"
    assert np.all(chain[-1] < chain[0]), "and it falls on every one of these problems"
    alpha = out["alpha_hist"].numpy()
    assert np.array_equal(out["accepts"].numpy(), (alpha > 0).sum(axis=0))
    assert len(eng.steps) == iters
    for it, (before, after, arow) in enumerate(eng.steps):
        assert np.array_equal(arow.numpy(), alpha[it])
        rej = alpha[it] == 0
        assert torch.equal(before[rej], after[rej]), "a rejected iteration leaves u bit-identical"
        assert np.array_equal(chain[it + 1][rej], chain[it][rej]) and np.all(chain[it + 1][~rej] < chain[it][~rej])
        assert bool((after.abs() <= u_lim).all()) and bool((eng.cands[it].abs() <= u_lim).all())
    assert bool((out["u_last"].abs() <= u_lim).all()) and torch.equal(out["u_last"], eng.steps[-1][1])
    # the cost reported is the cost of the iterate returned
    c = eng.rollout_cost(x0, out["u_last"], cost, "euler", 0.02)
    assert torch.equal(c, out["cost"])
    assert eng.calls.count("gn_direction") == iters and eng.calls.count("rollout_linearize") == iters
    return out


def test_whole_solve_on_the_golden_cartpole_phnn():
    model, eng = _model(pHNN, "phnn_cartpole")
    ctl = MPCController(phnn_model=model, horizon=10, dt=0.02, Q=[10.0, 100.0, 1.0, 10.0], R=0.01, u_min=-10.0, u_max=10.0,
                        x_min=[-0.7, -10.0, -10.0, -10.0], x_max=[0.7, 10.0, 10.0, 10.0])
    _check_solve(eng, ctl._cost(), 1, 10.0)


def test_whole_solve_on_the_canonical_model():
    model, eng = _model(pHNN_Canonical, "canonical_cartpole")
    ctl = MPCControllerCanonical(model, horizon=10, dt=0.02)
    _check_solve(eng, ctl._cost(), ctl.input_dim, 10.0)


def test_both_controllers_route_gauss_newton_and_refuse_unknown_names():
    model, eng = _model(pHNN, "phnn_cartpole")
    ctl = MPCController(phnn_model=model, horizon=10, dt=0.02, Q=[10.0, 100.0, 1.0, 10.0], R=0.01, u_min=-10.0, u_max=10.0,
                        optimizer_type="GaussNewton", max_iterations=3, gn_line_steps=4)
    assert ctl.gn_options() == dict(iters=3, line_steps=4, mu_init=1e-6, mu_min=1e-9, mu_max=1e6, mu_up=10.0, mu_down=0.1)
    out = ctl.solve_batch(X0, record_costs=True)
    ref = solver.gn_solve(eng, torch.tensor(X0), torch.zeros(4, 10, 1), ctl._cost(), "euler", 0.02, **ctl.gn_options())
    assert torch.equal(out["u_last"], ref["u_last"]) and torch.equal(out["costs"], ref["costs"])
    u = ctl.compute_control_batch(X0)
    assert u.shape == (4, 1) and np.array_equal(u, ref["u_last"][:, 0].numpy())
    assert ctl.compute_control(X0[0]).shape == (1,)
    ctl.optimizer_type = "Newton"
    with pytest.raises(ValueError, match="Unknown optimizer type"):
        ctl.solve_batch(X0)
    assert MPCController(phnn_model=model, horizon=10, dt=0.02, Q=[1.0] * 4, R=0.01).gn_line_steps == 8

    model, eng = _model(pHNN_Canonical, "canonical_cartpole")
    can = MPCControllerCanonical(model, horizon=10, dt=0.02, optimizer="GaussNewton", optimizer_steps=3, gn_line_steps=4)
    out = can.optimize_control_batch(X0)
    ref = solver.gn_solve(eng, torch.tensor(X0), torch.zeros(4, 10, can.input_dim), can._cost(), "euler", 0.02, **can.gn_options())
    assert torch.equal(out["best_u"], ref["u_last"]) and torch.equal(out["best_cost"], ref["cost"]) and torch.equal(out["costs"], ref["costs"])
    u, info = can.control(X0[1])
    assert u.shape == (can.input_dim,) and info["optimization"]["num_steps"] == 3 and len(info["optimization"]["costs"]) == 3
    assert info["optimization"]["final_cost"] <= info["optimization"]["costs"][-1]
    with pytest.raises(ValueError, match="Unknown optimizer type"):
        MPCControllerCanonical(model, horizon=10, dt=0.02, optimizer="Newton")
    with pytest.raises(ValueError, match="Unknown optimizer type"):
        MPCControllerCanonical(model, horizon=10, dt=0.02, optimizer="CEM")


# ----------------------------------------------------------------------------- options
def test_options_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} phnn_gn_options;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _capi.GnOptions._fields_]
    # 2 x int32, 5 x double, int32[4]
    assert C.sizeof(_capi.GnOptions) == 64
    o = _capi.GnOptions
    assert (o.line_steps.offset, o.mu_init.offset, o.mu_down.offset, o.reserved.offset) == (4, 8, 40, 48)
    for name in ("phnn_gn_workspace_bytes", "phnn_gn_direction", "phnn_gn_candidates", "phnn_gn_select", "phnn_solve_gn"):
        assert name in _capi.EXPORTED and re.search(r"\b%s\(" % name, header)
    assert _capi.load_library().phnn_version() >= 280


# ----------------------------------------------------------------------------- the slope identity, measured on the oracle
def test_slope_identity_on_the_float32_and_float64_oracle():
    """sum(grad_u * du) = -dV.  What the float32 oracle's own rounding leaves of it is the figure the GPU cross-check
    with K2 starts from (gn_model.SLOPE_F32_ORACLE); printed, then asserted at the recorded value."""
    import linearize_model as lm
    import variant_census as vc
    worst = {"f32": 0.0, "f64": 0.0}
    for sid in gm.SLOPE_SPECS:
        s, c = vc.CENSUS[sid], gm.slope_case(sid)
        sd = vc.build_state_dict(sid, s)
        for prec in worst:
            M = ol.OracleModel(sd, prec)
            r = M.rollout(c["x0"], c["u"], c["cost"], "euler", c["dt"], grad=True, traj=True)
            traj = r["traj"].astype(np.float32)
            A, Bm = lm.oracle_linearize(M, traj.astype(M.dtype), c["u"], c["cost"], "euler", c["dt"])
            d = gm.direction(A.astype(np.float32), Bm.astype(np.float32), traj, c["u"], c["cost"], s["n"], s["m"], 0.0)
            assert not d["status"].any()
            miss, _ = gm.slope_mismatch(r["grad_u"], d["du64"], d["dV"])
            worst[prec] = max(worst[prec], float((miss / d["dV"]).max()))
    print(f"\nslope identity, worst |sum(g du) + dV| / dV: float32 oracle {worst['f32']:.2e}, float64 oracle {worst['f64']:.2e}")
    assert worst["f32"] <= gm.SLOPE_F32_ORACLE and worst["f64"] <= gm.SLOPE_F32_ORACLE


# ----------------------------------------------------------------------------- convergence, as DESIGN.md section 18 tabulates it
@pytest.mark.parametrize("name", ["phnn_cartpole", "canonical_cartpole"])
def test_two_iterations_reach_below_the_adam_solve_of_the_reference_configuration(name):
    x0, cost, H, lr, iters = gm.convergence_case()
    eng = gm.GnOracleEngine(ol.load_weights(name), "f64")
    x0t, u0 = torch.tensor(x0), torch.zeros(x0.shape[0], H, 1)
    adam = solver.shooting_solve(eng, x0t, u0, cost, "euler", 0.02, lr, iters, track_best=True, u_min=-15.0, u_max=15.0)
    gn = solver.gn_solve(eng, x0t, u0, cost, "euler", 0.02, gm.CONVERGENCE_ITERS)
    print(f"\n{name}: Adam best of {iters} {adam['best_cost'].numpy()}, Gauss-Newton after {gm.CONVERGENCE_ITERS} {gn['cost'].numpy()}")
    assert bool((gn["cost"] <= adam["best_cost"]).all())
