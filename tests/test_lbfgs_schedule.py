"""The fixed slot schedule of the batched L-BFGS solve (phnn_solve_lbfgs), restated on the CPU (lbfgs_reference.py),
equals B separate torch.optim.LBFGS runs bit for bit: iterates, orig_loss of every step(), n_iter and func_evals.

Covered: a smooth seeded tanh-quadratic cost and the oracle engine's MPC cost / gradient (the G13 configuration); every
break reason forced through the options (opt_cond at the start of step(), lack of progress, loss change, the eval
limit, gtd, max_iter), dropped history updates (ys <= 1e-10), a wrapped history and mixed batches.
"""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from phnn_mpc_amd import _capi
from lbfgs_reference import lbfgs_schedule, tanh_quadratic, torch_lbfgs


def _same(a, b):
    assert torch.equal(a["u_last"], b["u_last"]), (a["u_last"] - b["u_last"]).abs().max()
    assert torch.equal(a["costs"], b["costs"])
    assert torch.equal(a["n_iter"], b["n_iter"]), (a["n_iter"], b["n_iter"])
    assert torch.equal(a["func_evals"], b["func_evals"]), (a["func_evals"], b["func_evals"])


def _run(evaluate, u0, **kw):
    a = lbfgs_schedule(evaluate, u0, **kw)
    _same(a, torch_lbfgs(evaluate, u0, **kw))
    return a


def test_smooth_cost_default_options():
    B, N = 5, 20
    ev = tanh_quadratic(B, N, seed=1)
    a = _run(ev, torch.zeros(B, N), lr=1.0, outer_steps=3)
    assert a["reasons"]["push"] > 0 and int(a["n_iter"].min()) > 3


def test_opt_cond_at_start():
    B, N = 4, 12
    a = _run(tanh_quadratic(B, N, seed=2), torch.zeros(B, N), lr=0.5, outer_steps=3, tolerance_grad=1e6)
    assert a["reasons"]["opt_cond_start"] == 3 * B
    assert a["n_iter"].tolist() == [0] * B and a["func_evals"].tolist() == [3] * B


def test_lack_of_progress_and_loss_change():
    B, N = 6, 16
    a = _run(tanh_quadratic(B, N, seed=3), torch.zeros(B, N), lr=0.2, outer_steps=2, tolerance_change=3e-2)
    assert a["reasons"]["small_step"] > 0 or a["reasons"]["loss_change"] > 0, a["reasons"]
    b = _run(tanh_quadratic(B, N, seed=3), torch.zeros(B, N), lr=1.0, outer_steps=2, tolerance_change=1e-3)
    assert b["reasons"]["loss_change"] + b["reasons"]["small_step"] > 0, b["reasons"]


def test_eval_limit():
    B, N = 4, 10
    a = _run(tanh_quadratic(B, N, seed=4), torch.zeros(B, N), lr=0.5, outer_steps=3, max_iter=20, max_eval=4)
    assert a["reasons"]["max_eval"] == 3 * B
    assert a["func_evals"].tolist() == [12] * B


def test_gtd_break():
    B, N = 3, 8
    a = _run(tanh_quadratic(B, N, seed=5), torch.randn(B, N), lr=1.0, outer_steps=3, tolerance_change=1e4)
    assert a["reasons"]["gtd"] == 3 * B and a["n_iter"].tolist() == [3] * B  # one iteration per step, never moves


def test_max_iter_break():
    B, N = 3, 8
    a = _run(tanh_quadratic(B, N, seed=6), torch.zeros(B, N), lr=0.1, outer_steps=2, max_iter=4,
             tolerance_change=0.0, tolerance_grad=0.0)
    assert a["reasons"]["max_iter"] == 2 * B and a["n_iter"].tolist() == [8] * B


def test_skipped_history_update():
    # a weak quadratic under a strong tanh: negative curvature along the path drops updates (ys <= 1e-10)
    B, N = 6, 6
    a = _run(tanh_quadratic(B, N, seed=7, scale=0.02), 0.3 * torch.randn(B, N), lr=1.0, outer_steps=3)
    assert a["reasons"]["skip_update"] > 0, a["reasons"]


def test_history_wraps():
    B, N = 3, 10
    a = _run(tanh_quadratic(B, N, seed=8), torch.zeros(B, N), lr=0.05, outer_steps=1, max_iter=40, max_eval=60,
             history_size=3, tolerance_change=0.0, tolerance_grad=0.0)
    assert a["reasons"]["push"] > 3 * B and a["n_iter"].tolist() == [40] * B


def test_mixed_batch_paths():
    # problems of very different curvature reach the tolerances at different iterations
    B, N = 8, 12
    ev_parts = [tanh_quadratic(B, N, seed=9, scale=s) for s in (0.05, 1.0, 20.0)]

    def ev(u, rows):
        c, g = torch.empty(u.shape[0]), torch.empty_like(u)
        for j, b in enumerate(rows):
            cj, gj = ev_parts[b % 3](u[j:j + 1], [b])
            c[j], g[j] = cj[0], gj[0]
        return c, g

    a = _run(ev, torch.zeros(B, N), lr=1.0, outer_steps=3, tolerance_change=1e-5, max_iter=10)
    assert len(set(a["n_iter"].tolist())) > 1 and len([k for k in a["reasons"] if k != "push"]) > 1, a


def test_oracle_engine_cost_g13():
    """The MPC closure of the G13 controller (H = 20, lr = 0.5, 3 steps) on the CPU oracle, per problem."""
    from oracle_engine import OracleEngine
    eng = OracleEngine(ol.load_weights("phnn_cartpole"))
    cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], 0.01, [0.0] * 4, -15.0, 15.0)
    rng = np.random.default_rng(0)
    B, H = 3, 20
    x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.1, 0.3, 0.3])).astype(np.float32))

    def ev(u, rows):
        c, g = torch.empty(u.shape[0]), torch.empty_like(u)
        for j, b in enumerate(rows):
            cj, gj = eng.rollout_cost_grad(x0[b:b + 1], u[j].reshape(1, H, 1), cost, "euler", 0.02)
            c[j], g[j] = cj[0], gj.reshape(-1)
        return c, g

    _run(ev, torch.zeros(B, H), lr=0.5, outer_steps=3)


@pytest.mark.parametrize("B", [1, 7])
def test_restatement_does_not_depend_on_batch(B):
    ev = tanh_quadratic(7, 9, seed=10)
    full = lbfgs_schedule(ev, torch.zeros(7, 9), lr=1.0, outer_steps=2)
    rows = list(range(B))
    part = lbfgs_schedule(lambda u, r: ev(u, [rows[i] for i in r]), torch.zeros(B, 9), lr=1.0, outer_steps=2)
    assert torch.equal(part["u_last"], full["u_last"][:B])
