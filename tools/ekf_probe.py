#!/usr/bin/env python3
"""Timing and demonstration probe of the batched extended Kalman filter.  One mode per run, so
that a `rocprofv3 --kernel-trace --stats` trace holds one setting:
  MODE=update          k_ekf_update alone: B = 65 536 problems, n = 4, two measured components
  MODE=step            phnn_ekf_step (k_ekf_controls, K1 with H = 1, the linearisation, k_ekf_update): B = 4096
  MODE=loop EST=0|1    DeviceClosedLoop, 4096 plants x 100 control steps (the config's Adam controller, graph per control
                       step, measurement noise on), without / with the estimator; wall time of run(), three runs
  MODE=demo            recorded, not asserted: the trained cart-pole fixture in a 256-plant loop of 100 steps, (a) noisy
                       velocities with every component measured, (b) positions only; the RMS error of `estimates` against
                       the true states next to that of the raw measurement, over all plant-steps and over those up to a
                       plant's termination (the loop does not freeze: a plant past its limits keeps diverging)
B, REPS, PLANTS, STEPS from the environment.  One JSON line per result."""
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
from phnn_mpc_amd.estimation import EKF  # noqa: E402

mode = os.environ.get("MODE", "update")
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


if mode in ("update", "step"):
    B = int(os.environ.get("B", 65536 if mode == "update" else 4096))
    eng = RolloutEngine(ol.load_weights("phnn_cartpole"), dev)
    rng = np.random.default_rng(0)
    ekf = EKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[1e-4, 2.5e-5], P0=1e-3)
    opt = ekf.options(4)
    x = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.2, 0.3, 0.3])).astype(np.float32), device=dev)
    y = x + 0.01 * torch.randn(B, 4, device=dev)
    P0 = torch.tensor(ekf.initial(np.zeros((B, 4)))[1], device=dev)
    if mode == "update":
        A = torch.tensor((np.eye(4) + 0.02 * rng.normal(size=(B, 4, 4))).astype(np.float32), device=dev)
        P, xhat = P0.clone(), torch.empty_like(x)
        nis = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        us = timed(lambda: eng.ekf_update(x, A, y, P, opt, xhat=xhat, nis=nis, innov=False, status=status))
        res = dict(mode=mode, B=B, n=4, measured=2, host_us_per_launch=us, failed=int((status != 0).sum()))
    else:
        u = torch.tensor(rng.uniform(-5, 5, size=(B, 20, 1)).astype(np.float32), device=dev)
        cost = _capi.make_cost(4, 1, [10.0, 100.0, 1.0, 10.0], 0.01, None, -10.0, 10.0)
        P, xhat, ws = P0.clone(), x.clone(), {}
        nis = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        us = timed(lambda: eng.ekf_step(xhat, P, u, 20, y, cost, "euler", 0.02, opt, nis=nis, status=status, workspace=ws))
        res = dict(mode=mode, B=B, host_us_per_step=us, failed=int((status != 0).sum()), workspace_bytes=eng.ekf_workspace_bytes(B))
    print(json.dumps(res), flush=True)
elif mode == "loop":
    B, T, est = int(os.environ.get("PLANTS", 4096)), int(os.environ.get("STEPS", 100)), os.environ.get("EST", "0") == "1"
    c = controller("phnn_cartpole")
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    sc = closed_loop.PlantScenario(meas_sigma=[0.002, 0.002, 0.05, 0.05], seed=0x9E3779B97F4A7C15)
    kw = dict(scenario=sc)
    if est:
        kw["estimator"] = EKF(measured=(0, 1, 2, 3), Qn=[1e-8, 1e-8, 1e-5, 1e-5], Rn=[4e-6, 4e-6, 2.5e-3, 2.5e-3], P0=1e-4)
    closed_loop.DeviceClosedLoop(c, X[:64], 3, **kw).run()  # warm-up: kernels loaded, workspaces sized
    run_s = []
    for _ in range(3):
        loop = closed_loop.DeviceClosedLoop(c, X, T, use_graph=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run()
        run_s.append(time.perf_counter() - t0)
    print(json.dumps(dict(mode=mode, estimator=est, plants=B, steps=T, iters=c.max_iterations, run_s=float(np.median(run_s)),
                          run_s_all=run_s, surviving=float((out["done_step"] < 0).mean()))), flush=True)
elif mode == "demo":
    B, T = int(os.environ.get("PLANTS", 256)), int(os.environ.get("STEPS", 100))
    c = controller("phnn_cartpole_trained")
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    cases = {
        "velocity noise, all measured": (
            [0.002, 0.002, 0.1, 0.1], EKF(measured=(0, 1, 2, 3), Qn=[1e-8, 1e-8, 1e-4, 1e-4], Rn=[4e-6, 4e-6, 1e-2, 1e-2], P0=1e-4)),
        "positions only": (
            [0.002, 0.002, 0.0, 0.0], EKF(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-4, 1e-4], Rn=[4e-6, 4e-6], P0=1e-4)),
    }
    for name, (sigma, ekf) in cases.items():
        sc = closed_loop.PlantScenario(meas_sigma=sigma, seed=0xE57)
        out = closed_loop.run_mpc_batch_device(c, X, T, scenario=sc, estimator=ekf)
        err = out["estimates"][1:].astype(np.float64) - out["states"][1:]
        ds = out["done_step"]  # row t + 1 is the state after step t: alive while no plant limit has been passed before it
        alive = (ds[None, :] < 0) | (np.arange(T)[:, None] <= ds[None, :])
        # the raw measurement's RMS error is its noise level by construction (0: that component is not measured at all)
        print(json.dumps(dict(mode=mode, case=name, plants=B, steps=T, rms_measurement=[float(v) for v in sc.meas_sigma],
                              rms_estimate=[float(v) for v in np.sqrt((err ** 2).mean(axis=(0, 1)))],
                              rms_estimate_until_termination=[float(v) for v in np.sqrt((err[alive] ** 2).mean(axis=0))],
                              plant_steps_until_termination=int(alive.sum()),
                              mean_nis_over_p_until_termination=float(np.nanmean(out["nis"][alive]) / len(ekf.measured)),
                              mean_nis_over_p=float(np.nanmean(out["nis"]) / len(ekf.measured)),
                              ekf_failed=int((out["ekf_status"] == 2).sum()), surviving=float((out["done_step"] < 0).mean()))), flush=True)
else:
    raise SystemExit(f"unknown MODE {mode}")
