"""CPU tests (no GPU) of the box-constrained LQ step (tests/gn_box_model.py, what k_gn_direction_box is pinned against),
of the solve with it (solver.gn_solve(box=True)) on the oracle-backed engine, and of the controllers' routing.

Bounds.  As in test_gn_model.py: the worst figure measured on the test's own inputs (printed by the test; DESIGN.md
section 19 repeats them) times 64, and never above 1e-8.
  KKT residual |x - clip(x - g, lo, hi)| / max(|x|, 1) of the box-QP, worst of m = 1 .. 4, 400 QPs each:      1.2e-15 -> 7.7e-14
  u + du against the dense box-QP minimiser (projected gradient run to a fixed point), relative to max(|u*|, 1),
  worst of H = 1 (every problem) and H = 6 (the problems whose active set the sweep reproduces):               6.0e-16 -> 3.9e-14
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gn_box_model as gb
import gn_model as gm
import oracle_lib as ol
import tvlqr_model as tm
from phnn_mpc_amd import _capi, solver
from phnn_mpc_amd.models import pHNN, pHNN_Canonical
from phnn_mpc_amd.mpc_controller import MPCController, create_mpc_from_config
from phnn_mpc_amd.mpc_controller_canonical import MPCControllerCanonical, create_mpc_controller
from test_gn_model import CFG, HORIZONS, NB, ROOT, SHAPES, X0, lq_problem, seed_of

MARGIN, CEILING = 64.0, 1e-8
MEASURED_KKT, MEASURED_U = 1.2e-15, 6.0e-16


def bound(measured):
    return min(MARGIN * measured, CEILING)


# ----------------------------------------------------------------------------- KKT of the box-QP
def seeded_qp(rng, m):
    """A well-conditioned SPD Q (eigenvalues >= 0.5), q of a size that clamps about half of the QPs, lo <= 0 <= hi."""
    M = rng.normal(size=(m, m))
    Q = M.T @ M + 0.5 * np.eye(m)
    return Q, rng.normal(size=m), -rng.uniform(0.0, 1.0, size=m), rng.uniform(0.0, 1.0, size=m)


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_box_qp_satisfies_the_kkt_conditions(m):
    rng = np.random.default_rng(40 + m)
    count, worst, clamped, free, failed = 400, 0.0, 0, 0, 0
    for _ in range(count):
        Q, q, lo, hi = seeded_qp(rng, m)
        r = gb.box_qp(Q, q, lo, hi)
        if r["x"] is None:
            failed += 1
            continue
        x = r["x"]
        g = q + Q @ x
        worst = max(worst, np.abs(x - np.clip(x - g, lo, hi)).max() / max(np.abs(x).max(), 1.0))
        assert np.all(lo <= x) and np.all(x <= hi)
        free += r["free"]
        clamped += any(r["digits"])
        assert r["free"] == (not any(r["digits"]))
        for i, dgt in enumerate(r["digits"]):
            assert dgt == 0 or x[i] == (lo[i] if dgt == 1 else hi[i])
    print(f"\nm={m}: KKT residual {worst:.2e}, {clamped} of {count} with a clamped component, {free} all-free, {failed} failed")
    assert failed == 0, "these seeds are well-conditioned: every QP has an active set that passes"
    assert clamped >= count // 4 and free >= count // 10
    assert worst <= bound(MEASURED_KKT)


def test_masked_factorisation_equals_the_factorisation_of_the_free_block():
    """The identity rows and columns of the fixed components leave the free block's L and D those of the sub-matrix."""
    rng = np.random.default_rng(7)
    for _ in range(50):
        m = 4
        Q, q, lo, hi = seeded_qp(rng, m)
        Ql = [[np.float64(Q[i][j]) for j in range(i + 1)] for i in range(m)]
        for c in (1, 5, 30, 46, 79):
            dg = [(c // 3 ** i) % 3 for i in range(m)]
            F = [i for i in range(m) if dg[i] == 0]
            M = [[(Ql[i][j] if dg[i] == 0 and dg[j] == 0 else np.float64(i == j)) for j in range(i + 1)] for i in range(m)]
            L, D, bad = gb._ldl(M, m)
            Ls, Ds, bads = gb._ldl([[Ql[F[a]][F[b]] for b in range(a + 1)] for a in range(len(F))], len(F))
            assert not bad and not bads
            for a, i in enumerate(F):
                assert D[i] == Ds[a]
                for b in range(a):
                    assert L[i][F[b]] == Ls[a][b]
            for i in range(m):
                if dg[i]:
                    assert D[i] == 1.0 and all(L[i][j] == 0.0 for j in range(i)) and all(L[k][i] == 0.0 for k in range(i + 1, m))


# ----------------------------------------------------------------------------- the degenerate case
def _case(n, m, H, seed=3, nb=NB):
    A, Bm, Q, R = tm.seeded_problem(seed, nb, H, n, m)
    rng = np.random.default_rng(seed + 1)
    traj = rng.uniform(-1, 1, size=(nb, H + 1, n)).astype(np.float32)
    u = rng.uniform(-1, 1, size=(nb, H, m)).astype(np.float32)
    return A, Bm, Q, R, traj, u


@pytest.mark.parametrize("H", HORIZONS)
@pytest.mark.parametrize("n,m", SHAPES)
def test_without_active_bounds_the_step_is_the_plain_one_bit_for_bit(n, m, H):
    A, Bm, Q, R, traj, u = _case(n, m, H, seed=seed_of(n, m, H))
    for cost in (_capi.make_cost(n, m, Q, R), _capi.make_cost(n, m, Q, R, None, -1e6, 1e6)):
        for mu in (0.0, 0.125):
            a, b = gm.direction(A, Bm, traj, u, cost, n, m, mu), gb.direction_box(A, Bm, traj, u, cost, n, m, mu)
            assert not a["status"].any() and not b["nclamp"].any() and not b["clipped"].any()
            for k in ("du", "du64", "dV", "status", "K", "k", "P"):
                assert tm.same_floats(a[k], b[k]), (k, mu)
    # and with them off a NaN anywhere fails exactly as the plain step does (status included)
    free = _capi.make_cost(n, m, Q, R)
    u1 = u.copy()
    u1[1, H - 1, 0] = np.nan
    a, b = gm.direction(A, Bm, traj, u1, free, n, m, 0.0), gb.direction_box(A, Bm, traj, u1, free, n, m, 0.0)
    for k in ("du", "dV", "status"):
        assert tm.same_floats(a[k], b[k]), k
    assert np.isnan(b["dV"][1]) and b["status"][1] == 0


# ----------------------------------------------------------------------------- the exact constrained minimiser
def projected_gradient(Hs, g, lo, hi):
    """min 1/2 d^T Hs d + g^T d over lo <= d <= hi from d = 0, run until d no longer changes by more than its last bit
    (float64; the iteration can end in a cycle of neighbouring floats)."""
    step = 1.0 / np.linalg.eigvalsh(Hs).max()
    d = np.zeros_like(g)
    for _ in range(100000):
        nd = np.clip(d - step * (Hs @ d + g), lo, hi)
        if np.abs(nd - d).max() <= 2.0 ** -52 * np.abs(d).max():
            return nd
        d = nd
    raise AssertionError("no fixed point")


STEP_LIMIT = 0.5  # every control may move this far: binds on about two thirds of the components


@pytest.mark.parametrize("H", [1, 6])
@pytest.mark.parametrize("n,m", SHAPES)
def test_one_step_is_the_exact_minimiser_inside_the_box(n, m, H):
    A, Bm, Lxx, Luu, X, U, dense = lq_problem(n, m, H)
    ldiag = np.broadcast_to(np.diag(Lxx), (NB, H + 1, n)).copy()
    lx, lu = np.einsum("ij,btj->bti", Lxx, X), np.einsum("ij,btj->bti", Luu, U)
    c = STEP_LIMIT
    r = gb.direction_box_core(A, Bm, Lxx, Luu, ldiag, lx, lu, 0.0, np.full(U.shape, -c), np.full(U.shape, c))
    assert not r["status"].any()
    worst, compared, bound_hits, free_hits, predicted = 0.0, 0, 0, 0, 0
    for b, (Hs, g) in enumerate(dense):
        star = projected_gradient(Hs, g, np.full(g.shape, -c), np.full(g.shape, c))
        du = r["du64"][b].reshape(-1)
        assert np.all(np.abs(du) <= c)
        # the sweep is exact where its backward pass held exactly the minimiser's active set: no clip in the forward
        # sweep (which would hold a component the gains did not know of), and the same components on the bounds
        same_set = np.array_equal(np.abs(star) == c, np.abs(du) == c) and not r["clipped"][b].any()
        if H == 1:
            assert same_set
        if same_set:
            compared += 1
            bound_hits += int((np.abs(star) == c).sum())
            free_hits += int((np.abs(star) != c).sum())
            u = U[b].reshape(-1)
            worst = max(worst, np.abs(du - star).max() / max(np.abs(u + star).max(), 1.0))
            # the predicted change -dV/2 is the change of the quadratic cost along du
            change = g @ du + 0.5 * du @ Hs @ du
            predicted += 1
            assert abs(-0.5 * r["dV"][b] - change) <= 1e-9 * abs(change)
    print(f"\n(n={n}, m={m}, H={H}): {compared} of {NB} compared, {bound_hits} components on a bound and {free_hits} free, "
          f"u + du {worst:.2e}")
    assert compared >= (NB if H == 1 else 1) and bound_hits > 0 and predicted > 0
    assert worst <= bound(MEASURED_U)
    assert np.array_equal(r["du"], r["du64"].astype(np.float32))


# ----------------------------------------------------------------------------- failure semantics
def check_failed(r, clean, b, status):
    assert r["status"][b] == status and r["nclamp"][b] == 0
    assert np.all(r["du"][b] == 0) and np.isnan(r["dV"][b])
    for o in range(r["du"].shape[0]):
        if o != b:
            assert r["status"][o] == 0 and tm.same_floats(r["du"][o], clean["du"][o]) and r["dV"][o] == clean["dV"][o]
            assert r["nclamp"][o] == clean["nclamp"][o]


# a 2 x 2 box-QP on a degenerate vertex (found by a seeded search over such problems) that no active set passes
NO_SET = dict(Q=[["0x1.3b36d810b92c5p+0", "-0x1.66456e8bd3ff4p-1"], ["-0x1.66456e8bd3ff4p-1", "0x1.0e23090e5c597p+0"]],
              q=["0x1.815a2385ba1d8p-1", "-0x1.6c15404063b02p-1"], lo=["-0x1.a37114fb7c63bp-1", "-0x1.cdd4da2bb6a03p-1"],
              hi=["0x1.f5e9e400a51e0p-1", "0x1.b94b85ef33860p-2"])


# the control bound of test_failure_semantics.  At (3, 1) the step of the seeded case stays inside +-0.5 in every
# component (a property of that input, not of the model), so the clean step would hold nothing: its box is +-0.25
FAILURE_BOUND = {(3, 1): 0.25}


@pytest.mark.parametrize("n,m", SHAPES)
def test_failure_semantics(n, m):
    H = 6
    c = FAILURE_BOUND.get((n, m), 0.5)
    A, Bm, Q, R, traj, u = _case(n, m, H, nb=3)
    cost = _capi.make_cost(n, m, Q, R, None, -c, c)
    u = np.clip(u, -c, c).astype(np.float32)
    clean = gb.direction_box(A, Bm, traj, u, cost, n, m, 0.0)
    assert not clean["status"].any() and np.isfinite(clean["dV"]).all() and clean["nclamp"].sum() > 0
    # an infeasible nominal and a NaN control fail at their step, like a pivot
    for value, t in ((1.5 * c, 4), (-1.5 * c, 0), (np.nan, 2)):
        u1 = u.copy()
        u1[1, t, m - 1] = value
        check_failed(gb.direction_box(A, Bm, traj, u1, cost, n, m, 0.0), clean, 1, t + 1)
    # a bad pivot: the status of gn_model
    B1 = Bm.copy()
    B1[1, 2, 0, 0] = np.nan
    r = gb.direction_box(A, B1, traj, u, cost, n, m, 0.0)
    assert r["status"][1] == gm.direction(A, B1, traj, u, cost, n, m, 0.0)["status"][1] == 3
    check_failed(r, clean, 1, 3)
    bad = _capi.make_cost(n, m, Q, -R - np.eye(m, dtype=np.float32), None, -c, c)
    r = gb.direction_box(A, Bm, traj, u, bad, n, m, 0.0)
    assert (r["status"] == H).all() and np.all(r["du"] == 0) and np.isnan(r["dV"]).all() and not r["nclamp"].any()
    # a NaN that reaches no pivot and no bound: status 0, and still no step
    t1 = traj.copy()
    t1[1, 2, n - 1] = np.nan
    check_failed(gb.direction_box(A, Bm, t1, u, cost, n, m, 0.0), clean, 1, 0)


def test_no_accepted_active_set_fails_the_step():
    f = {k: np.array([[float.fromhex(v) for v in row] if isinstance(row, list) else float.fromhex(row) for row in val])
         for k, val in NO_SET.items()}
    r = gb.box_qp(f["Q"], f["q"], f["lo"], f["hi"])
    assert r["x"] is None and not r["bad"] and not r["free"]
    # the same QP as step 0 of a one-step problem: B = 0 makes Quu = Luu + mu and qu = lu
    n, m, H, nb = 2, 2, 1, 2
    A = np.broadcast_to(np.eye(n, dtype=np.float32), (nb, H, n, n)).copy()
    Bm = np.zeros((nb, H, n, m), np.float32)
    Lxx = np.eye(n)
    ldiag, lx = np.ones((nb, H + 1, n)), np.zeros((nb, H + 1, n))
    lu = np.stack([f["q"], 0.1 * f["q"]])[:, None]
    lo, hi = np.broadcast_to(f["lo"], (nb, H, m)), np.broadcast_to(f["hi"], (nb, H, m))
    r = gb.direction_box_core(A, Bm, Lxx, f["Q"], ldiag, lx, lu, 0.0, lo, hi)
    assert list(r["status"]) == [1, 0] and np.all(r["du"][0] == 0) and np.isnan(r["dV"][0]) and r["nclamp"][0] == 0
    assert np.isfinite(r["dV"][1]) and np.any(r["du"][1] != 0)
    # the Levenberg-Marquardt answer to a failed step -- a larger mu -- moves it off the degenerate vertex
    r = gb.direction_box_core(A, Bm, Lxx, f["Q"], ldiag, lx, lu, 1e-6, lo, hi)
    assert not r["status"].any() and np.isfinite(r["dV"]).all() and np.any(r["du"][0] != 0)


# ----------------------------------------------------------------------------- convergence (DESIGN.md section 19's table)
@pytest.fixture(scope="module")
def solves():
    """{(name, H): (plain, box)} of the zero start, 8 iterations, default options, float64 oracle; computed once."""
    _, cost, _, _, _ = gm.convergence_case()
    x0 = gb.convergence_x0()
    out = {}
    for name in ("phnn_cartpole", "canonical_cartpole"):
        eng = gb.GnBoxOracleEngine(ol.load_weights(name), "f64")
        for H in (20, 50):
            u0 = torch.zeros(x0.shape[0], H, 1)
            out[name, H] = tuple(solver.gn_solve(eng, torch.tensor(x0), u0, cost, "euler", 0.02, 8, box=box) for box in (False, True))
    return out


def chain_of(out):
    return np.vstack([out["costs"].numpy(), out["cost"].numpy()[None]])


@pytest.mark.parametrize("H", [20, 50])
@pytest.mark.parametrize("name", ["phnn_cartpole", "canonical_cartpole"])
def test_box_solve_never_rises_stays_in_bounds_and_ends_no_higher_than_the_plain_solve(solves, name, H):
    plain, box = solves[name, H]
    chain = chain_of(box)
    assert np.isfinite(chain).all() and np.all(chain[1:] <= chain[:-1]), "non-increasing bit for bit"
    assert bool((box["u_last"].abs() <= 15.0).all())
    assert box["nclamp_hist"].shape == (8, 9) and box["nclamp_hist"].dtype == torch.int32 and "nclamp_hist" not in plain
    ratio = box["cost"].numpy().astype(np.float64) / plain["cost"].numpy().astype(np.float64)
    print(f"\n{name} H={H}: cost_box / cost_plain {np.array2string(ratio, precision=6)}")
    assert np.all(ratio <= 1.0 + 1e-5)
    # where the box step never clamped anything the two solves are the same solve
    for b in np.flatnonzero(box["nclamp_hist"].numpy().sum(axis=0) == 0):
        if np.array_equal(chain[:, b], chain_of(plain)[:, b]):
            assert torch.equal(box["u_last"][b], plain["u_last"][b])


@pytest.mark.parametrize("name,H,row", [("canonical_cartpole", 50, 8), ("canonical_cartpole", 50, 5), ("canonical_cartpole", 20, 8)])
def test_box_solve_ends_lower_where_the_bounds_are_active(solves, name, H, row):
    """x0 (-2, 0.2, 1, 2) is row 8 of the set and (0, 0.3, 0, 0) row 5.  Measured: 0.434, 0.821 and 0.826 of the plain
    solve's cost."""
    plain, box = solves[name, H]
    assert np.array_equal(gb.convergence_x0()[row], np.float32([-2.0, 0.2, 1.0, 2.0] if row == 8 else [0.0, 0.3, 0.0, 0.0]))
    ratio = float(box["cost"][row]) / float(plain["cost"][row])
    print(f"\n{name} H={H} x0 {gb.convergence_x0()[row]}: {float(box['cost'][row]):.6g} against {float(plain['cost'][row]):.6g} ({ratio:.3f})")
    assert ratio < 0.99


def test_saturated_start_stays_in_bounds_and_never_rises():
    _, cost, H, _, _ = gm.convergence_case()
    x0 = gb.convergence_x0()
    eng = gb.GnBoxOracleEngine(ol.load_weights("phnn_cartpole"), "f64")
    out = solver.gn_solve(eng, torch.tensor(x0), torch.full((9, H, 1), 30.0), cost, "euler", 0.02, 8, box=True)
    chain = chain_of(out)
    assert np.all(chain[1:] <= chain[:-1]) and bool((out["u_last"].abs() <= 15.0).all()) and np.all(chain[-1] < chain[0])
    assert int(out["nclamp_hist"][0].min()) > 0  # every nominal starts on the upper bound


# ----------------------------------------------------------------------------- plumbing
def _model(cls, name):
    w = ol.load_weights(name)
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    eng = gb.GnBoxOracleEngine(w)
    return m.set_engine(eng), eng


def test_controllers_route_gn_box():
    import yaml
    x0 = X0 * np.float32([1.0, 2.0, 1.0, 4.0])
    model, eng = _model(pHNN, "phnn_cartpole")
    kw = dict(phnn_model=model, horizon=10, dt=0.02, Q=[10.0, 100.0, 1.0, 10.0], R=0.01, u_min=-3.0, u_max=3.0,
              optimizer_type="GaussNewton", max_iterations=3, gn_line_steps=4)
    plain_ctl, ctl = MPCController(**kw), MPCController(**kw, gn_box=True)
    assert not plain_ctl.gn_box and "box" not in plain_ctl.gn_options() and ctl.gn_options()["box"] is True
    out = ctl.solve_batch(x0, record_costs=True)
    ref = solver.gn_solve(eng, torch.tensor(x0), torch.zeros(4, 10, 1), ctl._cost(), "euler", 0.02, **ctl.gn_options())
    assert torch.equal(out["u_last"], ref["u_last"]) and torch.equal(out["nclamp_hist"], ref["nclamp_hist"])
    assert int(out["nclamp_hist"].sum()) > 0 and "nclamp_hist" not in plain_ctl.solve_batch(x0)
    assert not torch.equal(out["u_last"], plain_ctl.solve_batch(x0)["u_last"])

    model, eng = _model(pHNN_Canonical, "canonical_cartpole")
    can = MPCControllerCanonical(model, horizon=10, dt=0.02, u_min=-3.0, u_max=3.0, optimizer="GaussNewton", optimizer_steps=3,
                                 gn_line_steps=4, gn_box=True)
    out = can.optimize_control_batch(x0)
    ref = solver.gn_solve(eng, torch.tensor(x0), torch.zeros(4, 10, can.input_dim), can._cost(), "euler", 0.02, **can.gn_options())
    assert torch.equal(out["best_u"], ref["u_last"]) and torch.equal(out["nclamp_hist"], ref["nclamp_hist"])
    assert not MPCControllerCanonical(model, horizon=10, dt=0.02).gn_box
    # the config key, next to gn_line_steps
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(optimizer="GaussNewton", gn_line_steps=4, gn_box=True)
    assert create_mpc_controller(model, cfg).gn_box and create_mpc_from_config(_model(pHNN, "phnn_cartpole")[0], cfg).gn_box
    del cfg["mpc"]["gn_box"]
    assert not create_mpc_controller(model, cfg).gn_box
    # an engine without the box step is never handed the keyword
    plain_eng = gm.GnOracleEngine(ol.load_weights("canonical_cartpole"))
    solver.gn_solve(plain_eng, torch.tensor(x0), torch.zeros(4, 10, can.input_dim), can._cost(), "euler", 0.02, 1)
    with pytest.raises(TypeError):
        solver.gn_solve(plain_eng, torch.tensor(x0), torch.zeros(4, 10, can.input_dim), can._cost(), "euler", 0.02, 1, box=True)


def test_flags_and_entry_points_match_the_header():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    assert int(re.search(r"#define PHNN_GN_BOX (\d+)", header).group(1)) == _capi.PHNN_GN_BOX == 1
    for name in ("phnn_gn_direction_box", "phnn_solve_gn_ex"):
        assert name in _capi.EXPORTED and re.search(r"\b%s\(" % name, header)
    lib = _capi.load_library()
    assert lib.phnn_version() == 290
    # the new entry points take the old ones' arguments with nclamp / flags and nclamp_hist added where the header puts them
    def params(name):
        text = re.search(r"\bint %s\((.*?)\);" % name, header, re.S).group(1)
        return [p.split()[-1].lstrip("*") for p in re.sub(r"/\*.*?\*/", "", text, flags=re.S).split(",")]
    d, dbox = params("phnn_gn_direction"), params("phnn_gn_direction_box")
    assert dbox == d[:13] + ["nclamp_dev"] + d[13:] and len(lib.phnn_gn_direction_box.argtypes) == len(dbox)
    s, sex = params("phnn_solve_gn"), params("phnn_solve_gn_ex")
    assert sex == s[:-1] + ["flags", "nclamp_hist_dev", "stream"] and len(lib.phnn_solve_gn_ex.argtypes) == len(sex)
    assert lib.phnn_solve_gn_ex.argtypes[-3] is C.c_int32
