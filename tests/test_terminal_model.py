"""CPU tests (no GPU) of the terminal cost (tests/terminal_model.py, what k_terminal_cost, k_dare and the terminal start
of k_gn_direction / k_gn_direction_box are pinned against), of the solves with it on the oracle-backed engine, and of the
controllers' routing.

Bounds.  As in test_gn_model.py: the worst figure measured on the test's own inputs (printed by the test; DESIGN.md
section 22 repeats them) times 64, under a ceiling.
  float64 figures, ceiling 1e-8:
    converged P/2 of dare against scipy.linalg.solve_discrete_are, relative to max|P|, worst of the cases:    1.2e-10 -> 7.7e-9
    the gain of dare's last step against the LQR gain formed from scipy's P, relative to max|K|:              8.4e-11 -> 5.4e-9
    one step with a terminal weight against the dense condensed-QP minimiser, relative to max|u*|:            2.4e-13 -> 1.5e-11
  figures through the float32 W, ceiling 1e-4 (W = (float)(0.5 (P - Lxx)) is P rounded to 24 bits, a perturbation of
  P_H of at most 2^-24 = 6e-8 relative per entry; a Riccati step at the fixed point maps it through the closed loop,
  A_cl^T dP A_cl, whose norm -- unlike its spectral radius -- may exceed one, here by an order of magnitude; a wrong
  formula is off by O(1)):
    P_0 of the direction with the terminal W against the DARE's P, relative to max|P|, worst of H = 1, 6, 50: 5.0e-7 -> 3.2e-5
    its first gain against the DARE's K, relative to max|K|:                                                 7.7e-7 -> 4.9e-5
  float32 kernel arithmetic (test_cost_and_gradient): the term and row H of traj_bar against float64, per entry at most
  (2 n + 2) 2^-24 sum_j |W_ij + W_ji| |e_j| (n products, n additions and the rounded weight sum, first order).
"""
import os
import re

import numpy as np
import pytest
import scipy.linalg
import torch

import gn_box_model as gb
import gn_model as gm
import oracle_lib as ol
import terminal_model as trm
import tvlqr_model as tm
from phnn_mpc_amd import _capi, solver
from phnn_mpc_amd.models import pHNN, pHNN_Canonical
from phnn_mpc_amd.mpc_controller import MPCController, create_mpc_from_config
from phnn_mpc_amd.mpc_controller_canonical import MPCControllerCanonical, create_mpc_controller
from phnn_mpc_amd.terminal import DARE_MAX_ITERS, TerminalCost
from test_gn_model import CFG, HORIZONS, NB, ROOT, SHAPES, X0, lq_problem, seed_of

MARGIN, CEILING, CEILING_F32 = 64.0, 1e-8, 1e-4
MEASURED_SCIPY, MEASURED_SCIPY_K, MEASURED_DENSE = 1.2e-10, 8.4e-11, 2.4e-13
MEASURED_P0, MEASURED_K0 = 5.0e-7, 7.7e-7
TOL = 1e-12


def bound(measured, ceiling=CEILING):
    return min(MARGIN * measured, ceiling)


def lti(n, m, seed, nb=NB):
    """A seeded constant (A, B) per problem and its cost matrices."""
    A, Bm, Q, R = tm.seeded_problem(seed, nb, 1, n, m)
    return A[:, 0], Bm[:, 0], Q, R, tm.cost_matrices(Q, R, n, m)


# ----------------------------------------------------------------------------- dare against tvlqr_model
@pytest.mark.parametrize("N", [1, 7, 40])
@pytest.mark.parametrize("n,m", SHAPES)
def test_dare_after_n_steps_is_tvlqr_on_n_copies_bit_for_bit(n, m, N):
    A, Bm, _, _, (Lxx, Luu) = lti(n, m, seed_of(n, m, N) + 21)
    for mu in (0.0, 0.125):
        r = trm.dare(A, Bm, Lxx, Luu, N, 0.0, mu)  # tol 0: never converged before a fixed point
        ref = tm.tvlqr(np.repeat(A[:, None], N, 1), np.repeat(Bm[:, None], N, 1), Lxx, Luu, mu)
        assert np.all(r["iters"] == N) and np.all(r["status"] == 2) and not ref["status"].any()
        assert np.array_equal(r["P"], ref["P0"]) and np.array_equal(r["K"], ref["K"][:, 0])
        assert np.array_equal(r["W"], (0.5 * (ref["P0"] - Lxx)).astype(np.float32))


# ----------------------------------------------------------------------------- dare against scipy
# the converging rows of the step-count table, each fixture with its own cost and dt
GOLDEN_CASES = [("phnn_cartpole_trained", "euler", 127), ("phnn_cartpole_trained", "rk4", 73),
                ("phnn_pendulum", "euler", 119), ("phnn_pendulum", "rk4", 119)]


def test_converged_dare_agrees_with_scipy():
    worst = worst_k = 0.0
    cases = [trm.linearize_at_target(name, integ) + (iters,) for name, integ, iters in GOLDEN_CASES]
    for n, m in SHAPES:
        A, Bm, Q, R, _ = lti(n, m, seed_of(n, m, 3) + 22)
        cases.append((A, Bm, _capi.make_cost(n, m, Q, R), None))
    for A, Bm, cost, iters in cases:
        n, m = A.shape[1], Bm.shape[2]
        Lxx, Luu = tm.cost_matrices_of(cost, n, m)
        r = trm.dare(A, Bm, Lxx, Luu, DARE_MAX_ITERS, TOL)
        assert not r["status"].any()
        if iters is not None:  # the counts of the issue's table
            assert r["iters"].tolist() == [iters]
        for b in range(A.shape[0]):
            P = scipy.linalg.solve_discrete_are(A[b].astype(np.float64), Bm[b].astype(np.float64), 0.5 * Lxx, 0.5 * Luu)
            worst = max(worst, np.abs(0.5 * r["P"][b] - P).max() / np.abs(P).max())
            # the gain of the last step is the LQR gain of that P
            K = -np.linalg.solve(0.5 * Luu + Bm[b].T.astype(np.float64) @ P @ Bm[b], Bm[b].T.astype(np.float64) @ P @ A[b])
            worst_k = max(worst_k, np.abs(r["K"][b] - K).max() / np.abs(K).max())
    print(f"\nconverged P/2 against scipy.linalg.solve_discrete_are: {worst:.2e} relative, the gain against scipy's: {worst_k:.2e}")
    assert worst <= bound(MEASURED_SCIPY) and worst_k <= bound(MEASURED_SCIPY_K)


def test_default_max_iters_covers_the_slowest_model_of_the_family():
    assert DARE_MAX_ITERS >= 2 * 62000  # the seed-0 phnn_cartpole needs some 62 000 steps at tol 1e-12


# ----------------------------------------------------------------------------- dare's status 2 and status 1
def test_max_iters_reached_returns_the_last_iterate_bit_for_bit():
    A, Bm, cost = trm.linearize_at_target("phnn_cartpole", "euler")
    Lxx, Luu = tm.cost_matrices_of(cost, 4, 1)
    r = trm.dare(A, Bm, Lxx, Luu, 64, TOL)
    ref = tm.tvlqr(np.repeat(A[:, None], 64, 1), np.repeat(Bm[:, None], 64, 1), Lxx, Luu)
    assert r["status"].tolist() == [2] and r["iters"].tolist() == [64]
    assert np.array_equal(r["P"], ref["P0"]) and np.array_equal(r["K"], ref["K"][:, 0]) and np.all(np.isfinite(r["W"]))


@pytest.mark.parametrize("n,m", SHAPES)
def test_a_singular_quu_fails_with_nan_outputs(n, m):
    A, _, Q, _, _ = lti(n, m, 5)
    Lxx, Luu = tm.cost_matrices(Q, np.zeros((m, m), np.float32), n, m)
    r = trm.dare(A, np.zeros((NB, n, m), np.float32), Lxx, Luu, 50, TOL)
    assert np.all(r["status"] == 1) and np.all(r["iters"] == 1)
    assert np.isnan(r["P"]).all() and np.isnan(r["K"]).all() and np.isnan(r["W"]).all()
    # one failing problem leaves its neighbours alone
    A2, B2, Q2, R2, (Lxx2, Luu2) = lti(n, m, 6)
    B2 = B2.copy()
    B2[1] = np.nan
    r = trm.dare(A2, B2, Lxx2, Luu2, 2000, TOL)
    assert r["status"].tolist() == [0, 1, 0, 0, 0] and np.isnan(r["W"][1]).all() and np.isfinite(r["W"][[0, 2, 3, 4]]).all()


# ----------------------------------------------------------------------------- k_terminal_cost's statement
@pytest.mark.parametrize("n", [2, 4])
def test_cost_and_gradient_against_float64(n):
    rng = np.random.default_rng(40 + n)
    nb, H = 37, 6
    traj = rng.normal(size=(nb, H + 1, n)).astype(np.float32)
    W = rng.normal(size=(nb, n, n)).astype(np.float32)  # not symmetric: the gradient takes W + W^T
    r = rng.normal(size=(nb, n)).astype(np.float32)
    c0 = rng.uniform(0, 10, size=nb).astype(np.float32)
    tb0 = np.full((nb, H + 1, n), np.nan, np.float32)
    tb0.view(np.uint32)[:] = 0xFFFFFFFF
    c, tb = trm.terminal_cost(traj, W, r, c0, tb0)
    e = traj[:, H].astype(np.float64) - r
    W64 = W.astype(np.float64)
    term = np.einsum("bi,bij,bj->b", e, W64, e)
    mag = np.einsum("bi,bij,bj->b", np.abs(e), np.abs(W64), np.abs(e))
    u = 2.0 ** -24
    assert np.all(np.abs(c.astype(np.float64) - (c0 + term)) <= (2 * n + 2) * u * mag + u * np.abs(c0 + term))
    g = trm.terminal_gradient64(traj, W, r)
    gmag = np.einsum("bij,bj->bi", np.abs(W64 + np.swapaxes(W64, 1, 2)), np.abs(e))
    assert np.all(np.abs(tb[:, H] - g) <= (2 * n + 2) * u * gmag)
    # rows t < H keep their bits; without a cotangent the cost is the same
    assert np.all(tb[:, :H].view(np.uint32) == 0xFFFFFFFF)
    assert np.array_equal(trm.terminal_cost(traj, W, r, c0)[0], c)
    # a NaN state: a NaN cost and a NaN row, for that rollout alone
    traj[3, H, 1] = np.nan
    c2, tb2 = trm.terminal_cost(traj, W, r, c0, tb0)
    assert np.isnan(c2[3]) and np.isnan(tb2[3, H]).all() and np.array_equal(np.delete(c2, 3), np.delete(c, 3))
    # a symmetric W counted once: e^T W e with W = I is |e|^2, and its gradient 2 e
    c3, tb3 = trm.terminal_cost(traj[:3], np.broadcast_to(np.eye(n, dtype=np.float32), (3, n, n)), r[:3], np.zeros(3, np.float32),
                                np.zeros((3, H + 1, n), np.float32))
    assert np.allclose(c3, (e[:3] ** 2).sum(1), rtol=1e-6) and np.allclose(tb3[:, H], 2 * e[:3], rtol=1e-6)


def test_weights_and_rows_follow_group_and_the_reference_rule():
    W = np.arange(3 * 4).reshape(3, 2, 2).astype(np.float32)
    assert np.array_equal(trm.weights_of(W, 6, 2, group=2), W[[0, 0, 1, 1, 2, 2]])
    assert trm.weights_of(TerminalCost(W[0]), 5, 2).shape == (5, 2, 2)
    cost = _capi.make_cost(2, 1, [1.0, 1.0], 0.1, [0.5, -0.5])
    assert np.array_equal(trm.target_rows(cost, 2, 3, 6), np.float32([[0.5, -0.5]] * 3))
    ref = np.arange(2 * 5 * 2).reshape(2, 5, 2).astype(np.float32)
    assert np.array_equal(trm.target_rows(cost, 2, 2, 6, ref, 0), ref[:, 4])  # min(0 + 6, 4): clamped at rows - 1
    assert np.array_equal(trm.target_rows(cost, 2, 2, 2, ref, 1), ref[:, 3])


# ----------------------------------------------------------------------------- the direction's terminal start
@pytest.mark.parametrize("n,m", SHAPES)
def test_without_a_terminal_weight_the_core_is_gn_models_bit_for_bit(n, m):
    H = 6
    A, Bm, Lxx, Luu, X, U, _ = lq_problem(n, m, H)
    ldiag = np.broadcast_to(np.diag(Lxx), (NB, H + 1, n)).copy()
    lx, lu = np.einsum("ij,btj->bti", Lxx, X), np.einsum("ij,btj->bti", Luu, U)
    inf = np.full((NB, H, m), np.inf)
    r = trm.direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, 0.25, -inf, inf)
    ref = gm.direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, 0.25)
    for k in ("du", "du64", "dV", "status", "K", "k", "P"):
        assert tm.same_floats(r[k], ref[k]), k
    lo, hi = -0.05 - 0 * U, 0.05 + 0 * U  # tight: steps get clamped
    r = trm.direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, 0.25, lo, hi)
    ref = gb.direction_box_core(A, Bm, Lxx, Luu, ldiag, lx, lu, 0.25, lo, hi)
    assert ref["nclamp"].sum() > 0
    for k in ("du", "du64", "dV", "status", "nclamp", "K", "k", "P"):
        assert tm.same_floats(r[k], ref[k]), k


@pytest.mark.parametrize("H", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_one_step_with_a_terminal_weight_is_the_exact_minimiser(n, m, H):
    """lq_problem's dense cost 1/2 (x^T Qs x + u^T Rs u) gains 1/2 x_H^T Tf x_H."""
    A, Bm, Lxx, Luu, X, U, dense = lq_problem(n, m, H)
    rng = np.random.default_rng(seed_of(n, m, H) + 9)
    M = rng.normal(size=(NB, n, n))
    W = (np.einsum("bij,bkj->bik", M, M) + 0.3 * rng.normal(size=(NB, n, n))).astype(np.float32)  # not symmetric
    ldiag = np.broadcast_to(np.diag(Lxx), (NB, H + 1, n)).copy()
    lx, lu = np.einsum("ij,btj->bti", Lxx, X), np.einsum("ij,btj->bti", Luu, U)
    Tf, te = trm.terminal_init(W, X[:, H])
    assert np.array_equal(Tf, W.astype(np.float64) + np.swapaxes(W, 1, 2).astype(np.float64))
    inf = np.full((NB, H, m), np.inf)
    r = trm.direction_core(A, Bm, Lxx, Luu, ldiag, lx, lu, 0.0, -inf, inf, Tf, te)
    assert not r["status"].any()
    A64, B64 = A.astype(np.float64), Bm.astype(np.float64)
    worst = 0.0
    for b, (Hs, g) in enumerate(dense):
        GamH = np.zeros((n, H * m))  # x_H = Phi_H x0 + GamH u
        for t in range(H):
            GamH = A64[b, t] @ GamH
            GamH[:, t * m:(t + 1) * m] += B64[b, t]
        Hs2 = Hs + GamH.T @ Tf[b] @ GamH
        g2 = g + GamH.T @ Tf[b] @ X[b, H]
        u = U[b].reshape(-1)
        star = u - np.linalg.solve(Hs2, g2)
        worst = max(worst, np.abs(u + r["du64"][b].reshape(-1) - star).max() / np.abs(star).max())
        assert np.array_equal(r["P"][b, H], Lxx + Tf[b])
    print(f"\n(n={n}, m={m}, H={H}): u + du with a terminal weight {worst:.2e} relative")
    assert worst <= bound(MEASURED_DENSE)


@pytest.mark.parametrize("n,m", SHAPES)
def test_with_the_lqr_weight_the_cost_to_go_does_not_depend_on_the_horizon(n, m):
    A, Bm, _, _, (Lxx, Luu) = lti(n, m, seed_of(n, m, 0) + 23)
    d = trm.dare(A, Bm, Lxx, Luu, DARE_MAX_ITERS, TOL)
    assert not d["status"].any()
    Tf, _ = trm.terminal_init(d["W"], np.zeros((NB, n)))
    ep = ek = 0.0
    for H in HORIZONS:
        AH, BH = np.repeat(A[:, None], H, 1), np.repeat(Bm[:, None], H, 1)
        ldiag = np.broadcast_to(np.diag(Lxx), (NB, H + 1, n)).copy()
        inf = np.full((NB, H, m), np.inf)
        r = trm.direction_core(AH, BH, Lxx, Luu, ldiag, np.zeros((NB, H + 1, n)), np.zeros((NB, H, m)), 0.0, -inf, inf, Tf,
                               np.zeros((NB, n)))
        assert not r["status"].any()
        for b in range(NB):
            ep = max(ep, np.abs(r["P"][b, 0] - d["P"][b]).max() / np.abs(d["P"][b]).max())
            if H == 1:  # the first gain of a one-step horizon is the DARE gain
                ek = max(ek, np.abs(r["K"][b, 0] - d["K"][b]).max() / np.abs(d["K"][b]).max())
    print(f"\n(n={n}, m={m}): P_0 for H = 1, 6, 50 against the DARE's P {ep:.2e}, first gain at H = 1 {ek:.2e} relative")
    assert ep <= bound(MEASURED_P0, CEILING_F32) and ek <= bound(MEASURED_K0, CEILING_F32)


# ----------------------------------------------------------------------------- the solves and the controllers
def _model(cls, name, precision="f32"):
    w = ol.load_weights(name)
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    eng = trm.TerminalOracleEngine(w, precision)
    return m.set_engine(eng), eng


W4 = np.float32([[40.0, 3.0, 2.0, 0.0], [1.0, 90.0, 0.0, 4.0], [0.0, 0.0, 6.0, 1.0], [0.0, 2.0, 0.0, 9.0]])  # not symmetric


def test_controllers_route_the_terminal_weight():
    import yaml
    model, eng = _model(pHNN, "phnn_cartpole")
    term = TerminalCost(W4)
    kw = dict(phnn_model=model, horizon=8, dt=0.02, Q=[10.0, 100.0, 1.0, 10.0], R=0.01, u_min=-3.0, u_max=3.0, lr=0.05,
              max_iterations=3)
    plain, ctl = MPCController(**kw), MPCController(**kw, terminal=term)
    eng.calls.clear()
    ref0 = plain.solve_batch(X0, record_costs=True)
    assert "terminal_cost" not in eng.calls and plain.terminal_cost() is None
    out = ctl.solve_batch(X0, record_costs=True)
    assert eng.calls.count("terminal_cost") == 3 and eng.calls.count("rollout_vjp") == 3
    ref = solver.shooting_solve(eng, torch.tensor(X0), torch.zeros(4, 8, 1), ctl._cost(), "euler", 0.02, 0.05, 3, u_min=-3.0,
                                u_max=3.0, terminal=term)
    assert torch.equal(out["u_last"], ref["u_last"]) and torch.equal(out["costs"], ref["costs"])
    # the first iterate is the same (zeros): its total cost is the stage cost plus the term, and the step differs
    traj = eng.rollout_cost(torch.tensor(X0), torch.zeros(4, 8, 1), ctl._cost(), "euler", 0.02, want_traj=True)[1].numpy()
    e = traj[:, 8].astype(np.float64)
    assert np.allclose(out["costs"][0].numpy() - ref0["costs"][0].numpy(), np.einsum("bi,ij,bj->b", e, W4, e), rtol=1e-4)
    assert not torch.equal(out["u_last"], ref0["u_last"])

    gkw = dict(kw, optimizer_type="GaussNewton", gn_line_steps=4)
    for box in (False, True):
        gctl = MPCController(**gkw, gn_box=box, terminal=term)
        assert gctl.gn_options()["terminal"] is term and "terminal" not in MPCController(**gkw).gn_options()
        eng.calls.clear()
        out = gctl.solve_batch(X0, record_costs=True)
        assert eng.calls.count("terminal_cost") == 1 + 3
        ref = solver.gn_solve(eng, torch.tensor(X0), torch.zeros(4, 8, 1), gctl._cost(), "euler", 0.02, **gctl.gn_options())
        assert torch.equal(out["u_last"], ref["u_last"]) and torch.equal(out["cost"], ref["cost"])
        costs = torch.cat([out["costs"], out["cost"][None]]).numpy()
        assert np.all(np.diff(costs, axis=0) <= 0) and out["accepts"].sum() > 0  # the TOTAL cost never rises
        assert not torch.equal(out["u_last"], MPCController(**gkw, gn_box=box).solve_batch(X0)["u_last"])

    # a captured solve keys its graph by the TerminalCost object: a raw matrix is refused before anything is captured
    for graphed, args in ((solver.GraphedSolve(eng), (0.05, 3)), (solver.GraphedGN(eng), (3,))):
        with pytest.raises(TypeError, match="TerminalCost"):
            graphed(eng, torch.tensor(X0), torch.zeros(4, 8, 1), ctl._cost(), "euler", 0.02, *args, terminal=W4)

    # the solves without a terminal term refuse, never ignore
    for opt in ("LBFGS", "MPPI", "CrossEntropy"):
        bad = MPCController(**dict(kw, optimizer_type=opt), terminal=term)
        with pytest.raises(ValueError, match="terminal"):
            bad.solve_batch(X0)
        with pytest.raises(ValueError, match="terminal"):
            bad.compute_control(X0[0])

    cmodel, ceng = _model(pHNN_Canonical, "canonical_cartpole")
    can = MPCControllerCanonical(cmodel, horizon=8, dt=0.02, u_min=-3.0, u_max=3.0, optimizer_steps=3, learning_rate=0.05, terminal=term)
    out = can.optimize_control_batch(X0)
    ref = solver.shooting_solve(ceng, torch.tensor(X0), torch.zeros(4, 8, 1), can._cost(), "euler", 0.02, 0.05, 3, track_best=True,
                                u_min=-3.0, u_max=3.0, terminal=term)
    assert torch.equal(out["best_u"], ref["best_u"]) and torch.equal(out["best_cost"], ref["best_cost"])
    gcan = MPCControllerCanonical(cmodel, horizon=8, dt=0.02, u_min=-3.0, u_max=3.0, optimizer="GaussNewton", optimizer_steps=2,
                                  gn_line_steps=4, terminal=term)
    ceng.calls.clear()
    gcan.optimize_control_batch(X0)
    assert ceng.calls.count("terminal_cost") == 3
    for opt in ("MPPI", "CrossEntropy"):
        with pytest.raises(ValueError, match="terminal"):
            MPCControllerCanonical(cmodel, horizon=8, dt=0.02, optimizer=opt, terminal=term).optimize_control_batch(X0)

    # the config section
    cfg = yaml.safe_load(open(CFG))
    assert create_mpc_controller(cmodel, cfg).terminal is None and create_mpc_from_config(model, cfg).terminal is None
    cfg["mpc"]["terminal"] = {"type": "matrix", "W": W4.tolist()}
    c1, c2 = create_mpc_controller(cmodel, cfg), create_mpc_from_config(model, cfg)
    assert np.array_equal(c1.terminal_cost().W, W4) and np.array_equal(c2.terminal_cost().W, W4)
    cfg["mpc"]["terminal"] = {"type": "nope"}
    with pytest.raises(ValueError, match="terminal"):
        create_mpc_controller(cmodel, cfg).terminal_cost()
    # an engine without the terminal cost is refused, and never handed the keyword without one
    plain_eng = gb.GnBoxOracleEngine(ol.load_weights("phnn_cartpole"))
    with pytest.raises(NotImplementedError, match="terminal"):
        solver.gn_solve(plain_eng, torch.tensor(X0), torch.zeros(4, 8, 1), ctl._cost(), "euler", 0.02, 1, terminal=term)
    solver.gn_solve(plain_eng, torch.tensor(X0), torch.zeros(4, 8, 1), ctl._cost(), "euler", 0.02, 1)


def test_lqr_weight_of_the_trained_model_on_the_oracle_engine():
    """TerminalCost.lqr: rollout_linearize at (x_target, 0) with H = 1, then dare; {type: lqr} in a config resolves to it."""
    import yaml
    model, eng = _model(pHNN, "phnn_cartpole_trained", "f64")
    cost = gm.convergence_case()[1]
    term = TerminalCost.lqr(eng, cost, None, "euler", 0.02)
    A, Bm, _ = trm.linearize_at_target("phnn_cartpole_trained", "euler")
    Lxx, Luu = tm.cost_matrices_of(cost, 4, 1)
    ref = trm.dare(A, Bm, Lxx, Luu, DARE_MAX_ITERS, TOL)
    assert term.info["iters"].tolist() == [127] and np.array_equal(term.W, ref["W"][0]) and not term.per_problem
    assert np.all(np.linalg.eigvalsh(term.W.astype(np.float64) + term.W.T) > 0)
    per = TerminalCost.lqr(eng, cost, np.zeros((3, 4), np.float32), "euler", 0.02)
    assert per.per_problem and np.array_equal(per.W, np.broadcast_to(term.W, (3, 4, 4)))
    with pytest.raises(RuntimeError, match="max_iters = 64"):
        TerminalCost.lqr(eng, cost, None, "euler", 0.02, max_iters=64)
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"]["terminal"] = {"type": "lqr"}
    ctl = create_mpc_from_config(model, cfg)
    got = ctl.terminal_cost()
    assert isinstance(got, TerminalCost) and ctl.terminal_cost() is got  # resolved once
    with pytest.raises(ValueError):
        TerminalCost(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        term.check(4, 2)


def test_entry_points_match_the_header():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    lib = _capi.load_library()
    for name in ("phnn_terminal_cost", "phnn_dare", "phnn_gn_direction_term", "phnn_solve_term", "phnn_solve_gn_term",
                 "phnn_rollout_vjp_ref"):
        assert name in _capi.EXPORTED
        text = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        params = [p for p in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
        assert len(getattr(lib, name).argtypes) == len(params), name
    assert [f for f, _ in _capi.Terminal._fields_] == ["W_dev", "batch_stride", "group"]
    assert [f for f, _ in _capi.DareOptions._fields_] == ["max_iters", "tol", "mu", "reserved"]
    for field in ("W_dev", "batch_stride", "group"):
        assert re.search(r"typedef struct \{[^}]*\b%s;[^}]*\} phnn_terminal;" % field, header)
