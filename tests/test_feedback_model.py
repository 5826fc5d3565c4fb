"""Tracking the plan between solves without a GPU: the stated law (feedback_model.control) against
the LQ optimum it must reproduce, the feedback continuation against the open-loop one, the exact special cases,
feedback.Tracking and the closed loop with track= on the CPU stand-in, the refusals, the `tracking:` config section and
the prototypes against the header."""
import os
import re

import numpy as np
import pytest
import torch

import feedback_model as fm
import oracle_lib as ol
import variant_census as vc
from phnn_mpc_amd import _capi
from phnn_mpc_amd.closed_loop import BatchedCartPole, PlantScenario, run_mpc_batch
from phnn_mpc_amd.estimation import EKF
from phnn_mpc_amd.feedback import Tracking
from phnn_mpc_amd.models import pHNN, pHNN_Canonical
from phnn_mpc_amd.mpc_controller import MPCController
from phnn_mpc_amd.mpc_controller_canonical import MPCControllerCanonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")

# DESIGN.md section 18's rule: the deviation measured on the test's own inputs (printed by the tests), asserted at 64 x
# that figure.  The control deviates from the optimum at float32 level because the plan's rows are stored as float32:
# never above 1e-5 of max |u|.  The cost of the feedback continuation deviates from the optimal cost-to-go at second
# order in that: never above 1e-8 relative.
MARGIN = 64.0
MEASURED_U, CEILING_U = 1.2e-7, 1e-5      # |control - K_j x_j| / max |u*|, worst over the grid (the test prints 1.10e-07)
MEASURED_V, CEILING_V = 3.8e-15, 1e-8     # |feedback cost - 1/2 x^T P_j x| / that, worst over the grid (prints 3.79e-15)
GRID = [(n, m, H) for (n, m) in vc.NM_PAIRS for H in (1, 6, 50)]
SEEDS = (7, 11)
NB = 9


def _perturbed(p, j, seed):
    """The plan's nominal row j moved off the plan by 0.1 N(0,1), as the float32 state the law is handed."""
    rng = np.random.default_rng(seed + 31 * j)
    return (p["traj"][:, j].astype(np.float64) + 0.1 * rng.normal(size=p["traj"][:, j].shape)).astype(np.float32)


# ----------------------------------------------------------------------------- the law against the LQ optimum
@pytest.mark.parametrize("n,m,H", GRID)
def test_the_law_returns_the_optimum_of_the_perturbed_problem(n, m, H):
    worst = 0.0
    for seed in SEEDS:
        p = fm.lq_plan(seed, NB, H, n, m)
        scale = np.abs(p["u"]).max()
        for j in range(H):
            x = _perturbed(p, j, seed)
            r = fm.control(x, p["u"], p["traj"], p["K"], j)
            assert not r["status"].any()
            opt = np.einsum("bki,bi->bk", p["K"][:, j], x.astype(np.float64))  # u* of the problem that starts at x
            worst = max(worst, float(np.abs(r["u"].astype(np.float64) - opt).max() / scale))
            assert np.array_equal(r["u"], r["v64"].astype(np.float32)), "rounded once"
            assert np.array_equal(r["dev"], np.abs(x.astype(np.float64) - p["traj"][:, j]).max(axis=1))
    print(f"\n(n, m, H) = ({n}, {m}, {H}): |control - optimum| / max|u| = {worst:.2e}")
    assert worst <= min(MARGIN * MEASURED_U, CEILING_U)


# ----------------------------------------------------------------------------- feedback against open loop
@pytest.mark.parametrize("n,m,H", GRID)
def test_the_feedback_continuation_is_optimal_and_cheaper_than_the_open_loop_one(n, m, H):
    worst, ratios = 0.0, []
    for seed in SEEDS:
        p = fm.lq_plan(seed, NB, H, n, m)
        for j in sorted({0, H // 2}):
            x = _perturbed(p, j, seed).astype(np.float64)
            feedback = fm.lq_cost_to_go(p, x, j, lambda xt, t: fm.control(xt.astype(np.float32), p["u"], p["traj"], p["K"], t)["u"])
            open_loop = fm.lq_cost_to_go(p, x, j, lambda xt, t: p["u"][:, t])
            optimal = 0.5 * np.einsum("bi,bij,bj->b", x, p["P"][:, j], x)
            worst = max(worst, float((np.abs(feedback - optimal) / optimal).max()))
            # strictness on the costs themselves and on the exact cost-to-go: at H = 1 the margin goes down to 1.6e-8
            # relative, far above the deviation asserted below and far below anything a ratio threshold could state
            assert np.all(feedback < open_loop) and np.all(optimal < open_loop)
            ratios.append(feedback / open_loop)
    r = np.concatenate(ratios)
    print(f"\n(n, m, H) = ({n}, {m}, {H}): |feedback - cost-to-go| relative {worst:.2e}, feedback / open loop "
          f"{r.min():.3g} .. {r.max():.12g}")
    assert worst <= min(MARGIN * MEASURED_V, CEILING_V)


# ----------------------------------------------------------------------------- exact cases
def _case(nb=6, H=4, n=4, m=2, seed=3):
    p = fm.lq_plan(seed, nb, H, n, m)
    rng = np.random.default_rng(seed)
    x = (p["traj"][:, 1] + 0.1 * rng.normal(size=(nb, n))).astype(np.float32)
    return p, x


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_no_deviation_returns_the_plan_control_bits():
    p, _ = _case()
    p["u"][0, 2, 0] = -0.0
    p["u"][1, 2, 1] = 0.0
    for bounds in (None, (-5.0, 5.0)):
        r = fm.control(p["traj"][:, 2], p["u"], p["traj"], p["K"], 2, bounds)
        assert np.array_equal(_bits(r["u"]), _bits(fm.clampf(p["u"][:, 2], -5.0, 5.0, bounds is not None)))
        assert not r["status"].any() and not r["dev"].any()
    assert _bits(r["u"])[0, 0] == 0x80000000 and _bits(r["u"])[1, 1] == 0


def test_gains_that_are_not_finite_give_status_1_and_the_plan_control():
    p, x = _case()
    ref = fm.control(x, p["u"], p["traj"], p["K"], 1, (-5.0, 5.0))
    K = p["K"].copy()
    K[1, 1, 0, 2] = np.nan
    K[4, 1, 1, 0] = np.inf
    K[2, 0, 0, 0] = np.nan  # another row of the plan: not looked at
    r = fm.control(x, p["u"], p["traj"], K, 1, (-5.0, 5.0))
    assert list(r["status"]) == [0, 1, 0, 0, 1, 0]
    un = fm.clampf(p["u"][:, 1], -5.0, 5.0, True)
    for b in (1, 4):
        assert np.array_equal(_bits(r["u"][b]), _bits(un[b])) and r["dev"][b] == ref["dev"][b]
    for b in (0, 2, 3, 5):
        assert np.array_equal(_bits(r["u"][b]), _bits(ref["u"][b]))


def test_a_deviation_that_is_not_finite_gives_status_2_and_the_plan_control():
    p, x = _case()
    ref = fm.control(x, p["u"], p["traj"], p["K"], 1)
    x[0, 3] = np.nan
    x[5, 0] = np.inf
    traj = p["traj"].copy()
    traj[3, 1, 2] = np.nan
    traj[2, 2, 0] = np.nan  # another row
    K = p["K"].copy()
    K[0, 1, 0, 0] = np.nan  # status 2 goes first
    r = fm.control(x, p["u"], traj, K, 1)
    assert list(r["status"]) == [2, 0, 0, 2, 0, 2]
    for b in (0, 3, 5):
        assert np.array_equal(_bits(r["u"][b]), _bits(p["u"][b, 1])) and np.isnan(r["dev"][b])
    for b in (1, 2, 4):
        assert np.array_equal(_bits(r["u"][b]), _bits(ref["u"][b])) and r["dev"][b] == ref["dev"][b]


def test_a_nan_plan_control_stays_nan_and_the_bounds_act_on_both_clamps():
    p, x = _case()
    p["u"][2, 1, 0] = np.nan
    r = fm.control(x, p["u"], p["traj"], p["K"], 1, (-0.05, 0.05))
    assert np.isnan(r["u"][2, 0]) and not np.isnan(r["u"][2, 1]) and r["status"][2] == 0
    ok = ~np.isnan(r["u"])
    assert np.all(np.abs(r["u"][ok]) <= np.float32(0.05))
    # the clamp of the plan's control: a control far outside the bounds enters the sum as the bound
    p["u"][:, 1, :] = 100.0
    un = np.float32(0.05)
    r = fm.control(x, p["u"], p["traj"], p["K"], 1, (-0.05, 0.05))
    s = np.einsum("bki,bi->bk", p["K"][:, 1], x.astype(np.float64) - p["traj"][:, 1])
    assert np.array_equal(r["u"], fm.clampf((np.float64(un) + s).astype(np.float32), -0.05, 0.05, True))
    assert np.any(r["u"] < un), "the feedback moves a clamped control back inside"
    # the clamp of the result, and none without bounds
    free = fm.control(x, p["u"], p["traj"], 50.0 * p["K"], 1)
    tight = fm.control(x, p["u"], p["traj"], 50.0 * p["K"], 1, (-200.0, 100.5))
    assert np.abs(free["u"]).max() > 100.5 and np.array_equal(tight["u"], np.clip(free["u"], -200.0, np.float32(100.5)))


def test_the_plan_row_comes_from_a_host_step_or_a_counter():
    p, x = _case(H=5)
    eng = fm.FeedbackOracleEngine(ol.load_weights("phnn_cartpole"))
    args = [torch.tensor(a) for a in (x, p["u"], p["traj"], p["K"])]
    for k in (1, 2, 5):  # solve_every = H included
        for step in (0, 1, 4, 7, 10):
            ref = fm.control(x, p["u"], p["traj"], p["K"], step % k)
            a = eng.feedback_control(*args, None, k, step=step)
            b = eng.feedback_control(*args, None, k, step_dev=torch.tensor([step], dtype=torch.int32))
            for r in (a, b):
                assert fm.same_floats(r["u"].numpy(), ref["u"]) and np.array_equal(r["status"].numpy(), ref["status"])
                assert fm.same_floats(r["dev"].numpy(), ref["dev"])


# ----------------------------------------------------------------------------- Tracking and the loop on the stand-in
X0 = np.array([[0.3, 0.1, 0.2, -0.1], [-0.5, 0.05, -0.3, 0.2], [0.1, -0.15, 0.4, 0.3], [0.8, 0.19, -0.2, -0.4]])


def _model(cls=pHNN, name="phnn_cartpole"):
    w = ol.load_weights(name)
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    eng = fm.FeedbackOracleEngine(w)
    return m.set_engine(eng), eng


def _controller(model, **kw):
    return MPCController(phnn_model=model, horizon=5, dt=0.02, Q=[10.0, 100.0, 1.0, 10.0], R=0.01, u_min=-10.0, u_max=10.0,
                         optimizer_type="Adam", lr=0.1, max_iterations=3, **kw)


def test_tracking_plan_is_the_three_step_methods_and_equals_the_model():
    model, eng = _model()
    ctl = _controller(model)
    cost = ctl._cost()
    x = torch.tensor(X0.astype(np.float32))
    u = torch.tensor(np.random.default_rng(0).uniform(-15, 15, size=(4, 5, 1)).astype(np.float32))  # some outside the bounds
    eng.calls.clear()
    pl = Tracking(2, mu=1e-3).plan(eng, x, u, cost, "euler", 0.02)
    assert eng.calls == ["rollout_linearize", "tvlqr"]
    ref = fm.plan(eng, X0, u.numpy(), cost, "euler", 0.02, mu=1e-3)
    assert np.array_equal(pl["traj"].numpy(), ref["traj"]) and fm.same_floats(pl["K"].numpy(), ref["K"])
    assert np.array_equal(pl["status"].numpy(), ref["status"]) and not ref["status"].any()
    assert np.array_equal(pl["traj"][:, 0].numpy(), X0.astype(np.float32)), "row 0 of the nominal is the state itself"
    # the control at j = 0 from that state is the clamped plan control
    r = Tracking(2).control(eng, x, u, pl, cost, step=4)
    assert torch.equal(r["u"], u[:, 0].clamp(-10.0, 10.0)) and not r["status"].any() and not r["dev"].any()


def test_solve_every_1_is_the_loop_without_tracking_bit_for_bit():
    model, eng = _model()
    ctl = _controller(model)
    sc = PlantScenario(meas_sigma=0.01, force_sigma=0.3, seed=5)
    a = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 4, scenario=sc)
    b = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 4, scenario=sc, track=Tracking(1))
    for k in ("states", "controls", "done_step", "disturbance"):
        assert np.array_equal(a[k], b[k]), k
    assert "track_status" not in a and b["track_status"].shape == (4, 4) and not b["track_status"].any()
    assert b["track_dev"].shape == (4, 4) and not b["track_dev"].any()
    assert run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, track=Tracking(1, log=False))["track_dev"] is None
    # with an estimator, too
    ekf = EKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-4)
    a = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 3, scenario=sc, estimator=ekf)
    b = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 3, scenario=sc, estimator=ekf, track=Tracking(1))
    for k in ("states", "controls", "estimates", "nis"):
        assert np.array_equal(a[k], b[k]), k


def test_solve_every_3_follows_the_stated_schedule():
    model, eng = _model()
    ctl = _controller(model)
    cost = ctl._cost()
    sc = PlantScenario(force_sigma=0.5, meas_sigma=0.005, seed=9)
    steps, k = 7, 3
    tr = Tracking(k)
    eng.calls.clear()
    out = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, steps, scenario=sc, track=tr)
    assert eng.calls.count("tvlqr") == 3 and eng.calls.count("feedback_control") == steps  # solves at steps 0, 3, 6
    # the loop restated: measurement -> (solve, plan) every third step -> control -> plant
    sim = BatchedCartPole(0.02, scenario=sc)
    sim.reset(X0)
    for s in range(steps):
        x32 = sim.measurement()
        if s % k == 0:
            seq = ctl.solve_batch(x32)["u_last"]
            pl = fm.plan(eng, x32, seq.numpy(), cost, "euler", 0.02)
        r = fm.control(x32, seq.numpy(), pl["traj"], pl["K"], s % k, (-10.0, 10.0))
        x, _ = sim.step(r["u"])
        assert np.array_equal(out["controls"][s], r["u"].astype(np.float64)) and np.array_equal(out["states"][s + 1], x)
        assert np.array_equal(out["track_status"][s], r["status"]) and np.array_equal(out["track_dev"][s], r["dev"])
    assert not out["track_status"].any()
    # the measurement noise shows as a deviation between the solves only: the solve steps start their plan at x
    assert not out["track_dev"][0::k].any() and np.all(out["track_dev"][1::k] > 0) and np.all(out["track_dev"][2::k] > 0)
    # the feedback acts: the tracking steps differ from the plan's own rows
    assert np.any(out["controls"][1] != np.clip(ctl.solve_batch(X0.astype(np.float32))["u_last"][:, 1].numpy(), -10, 10))


def test_canonical_warm_start_is_k_shifts_of_the_previous_best_sequence():
    model, eng = _model(pHNN_Canonical, "canonical_cartpole")
    ctl = MPCControllerCanonical(model, horizon=5, dt=0.02, optimizer_steps=2)
    seen = []
    solve = ctl.optimize_control_batch

    def spy(x0, u_init=None, **kw):
        out = solve(x0, u_init, **kw)
        seen.append((None if u_init is None else u_init.clone(), out["best_u"].clone()))
        return out

    ctl.optimize_control_batch = spy
    out = run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 5, track=Tracking(2))
    assert len(seen) == 3 and seen[0][0] is None  # solves at steps 0, 2, 4
    for (u_init, _), (_, prev) in zip(seen[1:], seen[:-1]):
        want = prev
        for _ in range(2):  # phnn_shift_controls twice: dst[t] = src[t+1], zeros in the last row
            want = torch.cat([want[:, 1:], torch.zeros(want.shape[0], 1, want.shape[2])], dim=1)
        assert np.array_equal(_bits(u_init.numpy()), _bits(want.numpy()))
    assert np.array_equal(out["controls"][0], seen[0][1][:, 0].numpy().astype(np.float64))


def test_refusals():
    model, eng = _model()
    ctl = _controller(model)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="solve_every"):
            Tracking(bad)
    for mu in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="mu"):
            Tracking(2, mu=mu)
    with pytest.raises(ValueError, match="horizon"):
        run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, track=Tracking(6))  # horizon 5
    run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 1, track=Tracking(5))
    with pytest.raises(ValueError, match="dt"):
        run_mpc_batch(BatchedCartPole(0.01), ctl, X0, 2, track=Tracking(2))
    import ekf_model
    ctl.model.set_engine(ekf_model.EkfOracleEngine(ol.load_weights("phnn_cartpole")))  # no feedback_control
    with pytest.raises(NotImplementedError, match="feedback_control"):
        run_mpc_batch(BatchedCartPole(0.02), ctl, X0, 2, track=Tracking(2))


def test_from_config_reads_the_optional_tracking_section():
    assert Tracking.from_config({"mpc": {}}) is None
    t = Tracking.from_config({"tracking": {"solve_every": 4, "mu": 1e-3}})
    assert (t.solve_every, t.mu, t.log) == (4, 1e-3, True)
    assert Tracking.from_config({"tracking": {"solve_every": 2, "log": False}}).log is False
    with pytest.raises(ValueError, match="unknown key"):
        Tracking.from_config({"tracking": {"solve_every": 2, "every": 3}})
    with pytest.raises(ValueError, match="solve_every"):
        Tracking.from_config({"tracking": {"mu": 0.0}})
    import yaml
    for name in os.listdir(os.path.join(ROOT, "configs")):
        if name.endswith((".yaml", ".yml")):  # no shipped configuration has the section
            assert Tracking.from_config(yaml.safe_load(open(os.path.join(ROOT, "configs", name))) or {}) is None


def _parameters(header, name):
    proto = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, header, re.S | re.M).group(1)
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")]


def test_prototypes_match_the_header_and_the_symbols_are_exported():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    lib = _capi.load_library()
    for name, nargs in (("phnn_feedback_workspace_bytes", 3), ("phnn_feedback_plan", 15), ("phnn_feedback_control", 17)):
        assert name in _capi.EXPORTED and hasattr(lib, name)
        params = _parameters(header, name)
        assert len(params) == nargs == len(getattr(lib, name).argtypes), name
    names = [a.split()[-1].lstrip("*") for a in _parameters(header, "phnn_feedback_control")]
    assert names == ["h", "x_dev", "u_dev", "traj_dev", "K_dev", "B", "H", "cost", "solve_every", "step_dev", "step_host", "u_out",
                     "status_out", "dev_out", "log_status_dev", "log_dev_dev", "stream"]
    names = [a.split()[-1].lstrip("*") for a in _parameters(header, "phnn_feedback_plan")]
    assert names == ["h", "x0_dev", "u_dev", "B", "H", "cost", "integrator", "dt", "opt", "workspace", "workspace_size", "traj_dev",
                     "K_dev", "status_dev", "stream"]
    assert lib.phnn_version() == 290
