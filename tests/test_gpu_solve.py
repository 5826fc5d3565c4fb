"""phnn_solve (include/phnn_mpc.h): the optimisation loop of MPCController.compute_control /
MPCControllerCanonical.optimize_control as one library call.  It must agree bit for bit with the Python loop over
K1 / K2 / K3 (solver.shooting_solve, itself pinned to the reference's controllers by G5 / G6)."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("needs a GPU")
    return t


def problem(rng, n, B, H, umax):
    x0 = (rng.uniform(-1, 1, size=(B, n)) * ([1.0, 0.3, 0.5, 0.5] if n == 4 else [1.5, 0.8])).astype(np.float32)
    u0 = (rng.uniform(-0.2, 0.2, size=(B, H, 1)) * umax).astype(np.float32)
    return x0, u0


@pytest.mark.parametrize("name,integ", [("phnn_cartpole", "euler"), ("phnn_cartpole", "rk4"), ("canonical_cartpole", "euler"),
                                        ("phnn_pendulum", "euler")])
@pytest.mark.parametrize("B", [1, 19, 600])
def test_library_solve_equals_the_python_loop_bitwise(torch, name, integ, B):
    from phnn_mpc_amd.engine import RolloutEngine
    from phnn_mpc_amd.solver import shooting_solve
    g, w = ol.load_golden(name), ol.load_weights(name)
    eng = RolloutEngine(w)
    cost = ol.cost_from_golden(g)
    rng = np.random.default_rng(B)
    H, iters = (20, 30) if B == 1 else (12, 7)
    x0, u0 = problem(rng, eng.n, B, H, float(g["u_max"]))
    x0t, u0t = torch.tensor(x0, device=eng.device), torch.tensor(u0, device=eng.device)
    ref = shooting_solve(eng, x0t, u0t, cost, integ, float(g["dt"]), 0.015, iters, track_best=True,
                         u_min=float(g["u_min"]), u_max=float(g["u_max"]), record_costs=True)
    out = eng.solve(x0t, u0t, cost, integ, float(g["dt"]), lr=0.015, iters=iters, track_best=True, record_costs=True)
    for k in ("u_last", "costs", "best_u", "best_cost"):
        assert torch.equal(out[k], ref[k]), (k, (out[k] - ref[k]).abs().max())
    # without best-iterate tracking and cost history (MPCController's use)
    out = eng.solve(x0t, u0t, cost, integ, float(g["dt"]), lr=0.015, iters=iters, track_best=False, record_costs=False)
    assert torch.equal(out["u_last"], ref["u_last"]) and out["costs"] is None and "best_u" not in out


def test_solve_argument_checks(torch):
    from phnn_mpc_amd.engine import RolloutEngine
    from phnn_mpc_amd.solver import shooting_solve
    g = ol.load_golden("phnn_cartpole")
    eng = RolloutEngine(ol.load_weights("phnn_cartpole"))
    cost = ol.cost_from_golden(g)
    x0, u0 = torch.zeros(2, 4, device=eng.device), torch.ones(2, 5, 1, device=eng.device)
    out = eng.solve(x0, u0, cost, "euler", 0.02, iters=0)  # nothing to do: the initial iterate comes back
    assert torch.equal(out["u_last"], u0)
    out = eng.solve(x0, u0, cost, "euler", 0.02, iters=0, track_best=True)  # and no best iterate yet: shooting_solve's
    ref = shooting_solve(eng, x0, u0, cost, "euler", 0.02, 0.015, 0, track_best=True)
    for k in ("u_last", "best_u", "best_cost", "costs"):
        assert torch.equal(out[k], ref[k]), k
    assert torch.isinf(out["best_cost"]).all() and not out["best_u"].any()
    with pytest.raises(ValueError):
        eng.solve(x0, u0, cost, "leapfrog", 0.02, iters=3)
