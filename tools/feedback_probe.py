#!/usr/bin/env python3
"""Timing and closed-loop probe of tracking the plan between solves.  One mode per run, so that a
`rocprofv3 --kernel-trace --stats` trace holds one setting:
  MODE=control         k_feedback_control alone: B = 65 536 problems, n = 4, m = 1, H = 20, bounds on
  MODE=plan            phnn_feedback_plan (K1 with trajectories, the linearisation, the LQ backward pass): B = 4096, H = 20
  MODE=loop K=0|k      DeviceClosedLoop, 4096 plants x 100 control steps (the config's Adam controller, graph per control
                       step), K=0 without tracking, else track=Tracking(k); wall time of run(), RUNS runs, and a hash of the
                       controls
  MODE=cost K=k GAINS=1|0   recorded, not asserted: the same loop under a PlantScenario (force_sigma 0.5, +-20 % spread of
                       the masses and the length), metrics on; the mean closed-loop cost and the count of stable plants.
                       GAINS=0 zeroes the gains after every plan: open-loop tracking of the plan between the solves
B, REPS, PLANTS, STEPS, RUNS from the environment.  One JSON line per result."""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol  # noqa: E402
from phnn_mpc_amd import _capi, closed_loop  # noqa: E402
from phnn_mpc_amd.engine import RolloutEngine  # noqa: E402
from phnn_mpc_amd.feedback import Tracking  # noqa: E402

mode = os.environ.get("MODE", "control")
reps = int(os.environ.get("REPS", 20))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
dev = "cuda:0"


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def controller(weights):
    import yaml
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    m = pHNN(CFG)
    m.load_state_dict({k: torch.tensor(w) for k, w in ol.load_weights(weights).items()})
    return create_mpc_from_config(m, yaml.safe_load(open(CFG)))


if mode in ("control", "plan"):
    B, H = int(os.environ.get("B", 65536 if mode == "control" else 4096)), 20
    eng = RolloutEngine(ol.load_weights("phnn_cartpole"), dev)
    rng = np.random.default_rng(0)
    cost = _capi.make_cost(4, 1, [10.0, 100.0, 1.0, 10.0], 0.01, None, -10.0, 10.0)
    x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.2, 0.3, 0.3])).astype(np.float32), device=dev)
    u = torch.tensor(rng.uniform(-5, 5, size=(B, H, 1)).astype(np.float32), device=dev)
    ws = {}
    if mode == "plan":
        us = timed(lambda: eng.feedback_plan(x0, u, cost, "euler", 0.02, workspace=ws))
        res = dict(mode=mode, B=B, H=H, host_us_per_plan=us, failed=int((ws["fb_status"] != 0).sum()),
                   workspace_bytes=eng.feedback_workspace_bytes(B, H))
    else:
        pl = eng.feedback_plan(x0, u, cost, "euler", 0.02, workspace=ws)
        x = pl["traj"][:, 3] + 0.01 * torch.randn(B, 4, device=dev)
        out = torch.empty(B, 1, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        dv = torch.empty(B, dtype=torch.float64, device=dev)
        us = timed(lambda: eng.feedback_control(x, u, pl["traj"], pl["K"], cost, 5, step=3, u_out=out, status=status, dev=dv))
        res = dict(mode=mode, B=B, H=H, n=4, m=1, host_us_per_launch=us, open_loop=int((status != 0).sum()))
    print(json.dumps(res), flush=True)
elif mode in ("loop", "cost"):
    B, T = int(os.environ.get("PLANTS", 4096)), int(os.environ.get("STEPS", 100))
    k, runs = int(os.environ.get("K", 0)), int(os.environ.get("RUNS", 3))
    gains = os.environ.get("GAINS", "1") == "1"
    c = controller("phnn_cartpole")
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    kw = {}
    if k:
        kw["track"] = Tracking(k)
    warm = dict(kw)
    if mode == "cost":
        params = closed_loop.PlantScenario.spread(B, dict(masscart=0.2, masspole=0.2, length=0.2), np.random.default_rng(1))
        for d, p in ((kw, params), (warm, params[:64])):
            d.update(scenario=closed_loop.PlantScenario(params=p, force_sigma=0.5, seed=0x9E3779B97F4A7C15), metrics=True)
    if not gains:  # open-loop tracking: the plan's gains are zeroed right after every plan (inside the captured step)
        plan = c.engine.feedback_plan

        def zeroed(*a, **kwargs):
            r = plan(*a, **kwargs)
            r["K"].zero_()
            return r

        c.engine.feedback_plan = zeroed
    closed_loop.DeviceClosedLoop(c, X[:64], 7, **warm).run()  # warm-up: kernels loaded, workspaces sized
    run_s = []
    for _ in range(runs):
        loop = closed_loop.DeviceClosedLoop(c, X, T, use_graph=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run()
        run_s.append(time.perf_counter() - t0)
    res = dict(mode=mode, solve_every=k, gains=gains, plants=B, steps=T, iters=c.max_iterations, run_s=float(np.median(run_s)),
               run_s_all=run_s, controls_sha=hashlib.sha256(out["controls"].tobytes()).hexdigest()[:16],
               surviving=float((out["done_step"] < 0).mean()))
    if k:
        res.update(open_loop_steps=int((out["track_status"] != 0).sum()), mean_dev=float(np.nanmean(out["track_dev"])))
    if mode == "cost":
        res.update(mean_cost=float(np.mean(out["cost"])), median_cost=float(np.median(out["cost"])), stable=int(out["stable"].sum()))
    print(json.dumps(res), flush=True)
else:
    raise SystemExit(f"unknown MODE {mode}")
