#!/usr/bin/env python3
"""Timing and closed-loop probe of the terminal cost.  One mode per run:
  MODE=kernels          k_terminal_cost alone at B = 65 536, H = 50 (cost and row H of the cotangent), and k_dare at B = 1
                        and B = 4096 on the trained cart-pole model linearised at the target (127 Riccati steps)
  MODE=iter SOLVER=adam|gn TERM=0|1
                        one iteration of the solve, device time by events over ITERS iterations, REPS calls: Adam at
                        B = 65 536, H = 50 (the benchmark's shape), Gauss-Newton at B = 4096, H = 20, L = 8
  MODE=k2bar            K2 alone at the Adam shape, on the K1 -> K2 workspace: without a cotangent and with a zero
                        (B, H+1, n) one -- what reading it costs
  MODE=loop SOLVER=adam|gn TERM=0|1
                        recorded, not asserted: DeviceClosedLoop, PLANTS plants x STEPS control steps on the TRAINED
                        fixture, H = 20, the config's cost, metrics on; TERM=1: terminal {type: lqr}.  The mean closed-loop
                        cost, the count of stable plants, the survivors
MODE=iter with TERM=0 and MODE=k2bar use only what the parent commit has, so that the same file times the parent's tree:
PROBE_ROOT names the tree whose package and library are loaded (default: this one) and TREE_LABEL what the result calls it
(default: PROBE_ROOT relative to this tree).  One JSON line per result."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(os.environ.get("PROBE_ROOT", HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol  # noqa: E402
from phnn_mpc_amd import _capi, closed_loop  # noqa: E402
from phnn_mpc_amd.engine import RolloutEngine  # noqa: E402

mode = os.environ.get("MODE", "kernels")
reps = int(os.environ.get("REPS", 20))
solver = os.environ.get("SOLVER", "adam")
with_term = os.environ.get("TERM", "0") == "1"
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
dev = "cuda:0"
COST = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], 0.01, None, -15.0, 15.0)


def device_us(fn, n=reps):
    """Median and minimum device time of fn() in microseconds, by events around each call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return float(np.median(out)), float(np.min(out))


def inputs(B, H, seed=0):
    rng = np.random.default_rng(seed)
    x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.2, 0.3, 0.3])).astype(np.float32), device=dev)
    u = torch.tensor(rng.uniform(-5, 5, size=(B, H, 1)).astype(np.float32), device=dev)
    return x0, u


def lqr_weight(eng):
    from phnn_mpc_amd.terminal import TerminalCost
    return TerminalCost.lqr(eng, COST, None, "euler", 0.02)


res = dict(mode=mode, tree=os.environ.get("TREE_LABEL") or os.path.relpath(ROOT, HERE))
if mode == "kernels":
    eng = RolloutEngine(ol.load_weights("phnn_cartpole_trained"), dev)
    B, H = int(os.environ.get("B", 65536)), 50
    x0, u = inputs(B, H)
    c, traj = eng.rollout_cost(x0, u, COST, "euler", 0.02, want_traj=True)
    term = lqr_weight(eng)
    tb = torch.zeros_like(traj)
    med, mn = device_us(lambda: eng.terminal_cost(traj, COST, term, c, traj_bar=tb))
    res.update(B=B, H=H, terminal_cost_us=med, terminal_cost_us_min=mn, dare_iters=int(term.info["iters"][0]))
    med, mn = device_us(lambda: eng.terminal_cost(traj, COST, term, c))
    res.update(terminal_cost_only_us=med, terminal_cost_only_us_min=mn)
    xt = torch.zeros(1, 4, device=dev)
    A, Bm, _ = eng.rollout_linearize(xt, torch.zeros(1, 1, 1, device=dev), COST, "euler", 0.02)
    for nb in (1, 4096):
        An, Bn = A[:, 0].expand(nb, 4, 4).contiguous(), Bm[:, 0].expand(nb, 4, 1).contiguous()
        med, mn = device_us(lambda: eng.dare(An, Bn, COST))
        res[f"dare_B{nb}_us"], res[f"dare_B{nb}_us_min"] = med, mn
elif mode == "iter":
    eng = RolloutEngine(ol.load_weights("phnn_cartpole_trained"), dev)
    iters = int(os.environ.get("ITERS", 10))
    kw = dict(terminal=lqr_weight(eng)) if with_term else {}
    ws = {}
    if solver == "adam":
        B, H = int(os.environ.get("B", 65536)), 50
        x0, u = inputs(B, H)
        fn = lambda: eng.solve(x0, u, COST, "euler", 0.02, lr=0.015, iters=iters, record_costs=False, workspace=ws, **kw)  # noqa: E731
    else:
        B, H = int(os.environ.get("B", 4096)), 20
        x0, u = inputs(B, H)
        fn = lambda: eng.solve_gn(x0, u, COST, "euler", 0.02, iters=iters, line_steps=8, record_costs=False, workspace=ws, **kw)  # noqa: E731
    med, mn = device_us(fn)
    res.update(solver=solver, terminal=with_term, B=B, H=H, iters=iters, us_per_iter=med / iters, us_per_iter_min=mn / iters)
elif mode == "k2bar":
    eng = RolloutEngine(ol.load_weights("phnn_cartpole_trained"), dev)
    B, H = int(os.environ.get("B", 65536)), 50
    x0, u = inputs(B, H)
    f = dict(dtype=torch.float32, device=dev)
    c, traj, g = torch.empty(B, **f), torch.empty(B, H + 1, 4, **f), torch.empty(B, H, 1, **f)
    stash = torch.empty(eng.workspace_bytes(B, H, 0), dtype=torch.uint8, device=dev)
    zero = torch.zeros(B, H + 1, 4, **f)
    p = eng._p
    rc = eng.lib.phnn_rollout_fwd(eng.h, p(x0), p(u), B, H, C.byref(COST), 0, 0.02, p(c), p(traj), p(stash), eng._stream())
    assert rc == 0

    def k2(bar):
        assert eng.lib.phnn_rollout_vjp(eng.h, p(x0), p(u), B, H, C.byref(COST), 0, 0.02, p(traj), p(stash), p(bar), None, p(g),
                                        None, eng._stream()) == 0

    for tag, bar in (("k2_us", None), ("k2_zero_bar_us", zero), ("k2_again_us", None), ("k2_zero_bar_again_us", zero)):
        res[tag], res[tag + "_min"] = device_us(lambda: k2(bar))
    res.update(B=B, H=H)
elif mode == "loop":
    import yaml
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    B, T = int(os.environ.get("PLANTS", 4096)), int(os.environ.get("STEPS", 300))
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"]["optimizer"] = {"adam": "Adam", "gn": "GaussNewton"}[solver]
    if solver == "gn":
        cfg["mpc"]["optimizer_steps"] = int(os.environ.get("GN_ITERS", 4))
    if with_term:
        cfg["mpc"]["terminal"] = {"type": "lqr"}
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(w) for k, w in ol.load_weights("phnn_cartpole_trained").items()})
    c = create_mpc_from_config(m, cfg)
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    closed_loop.DeviceClosedLoop(c, X[:64], 7, metrics=True).run()  # warm-up: kernels loaded, workspaces sized
    loop = closed_loop.DeviceClosedLoop(c, X, T, use_graph=True, metrics=cfg.get("stability", True), log=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = loop.run()
    res.update(solver=solver, terminal=with_term, plants=B, steps=T, horizon=c.horizon, iters=c.max_iterations,
               run_s=time.perf_counter() - t0, mean_cost=float(np.mean(out["cost"])), median_cost=float(np.median(out["cost"])),
               stable=int(out["stable"].sum()), surviving=int((out["done_step"] < 0).sum()),
               mean_longest_run_s=float(np.mean(out["longest_run_s"])))
    if with_term:
        res.update(dare_iters=int(c.terminal_cost().info["iters"][0]))
else:
    raise SystemExit(f"unknown MODE {mode}")
print(json.dumps(res), flush=True)
