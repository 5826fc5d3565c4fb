#!/usr/bin/env python3
"""Timing and demonstration probe of the batched unscented Kalman filter.  One mode per run, so
that a `rocprofv3 --kernel-trace --stats` trace holds one setting:
  MODE=sigma           k_ukf_sigma<4> alone: B = 65 536 problems, with control rows
  MODE=moments         k_ukf_moments<4> alone: B = 65 536 problems, Y read in place from a (B S, 2, n) trajectory
  MODE=step FILTER=ukf|ekf INTEG=euler|rk4
                       phnn_ukf_step (k_ukf_sigma, K1 with H = 1 on 9 B rollouts, k_ukf_moments, k_ekf_update) or
                       phnn_ekf_step (k_ekf_controls, K1, the linearisation, k_ekf_update): B = 4096
  MODE=loop EST=0|1|2  DeviceClosedLoop, 4096 plants x 100 control steps (the config's Adam controller, graph per control
                       step, measurement noise on): no estimator / EKF / UKF; wall time of run(), three runs, and a hash
                       of the controls.  PACKAGE_ROOT: the tree whose package is imported (default: this one), so that
                       the same probe times another checkout of the library
  MODE=demo            recorded, not asserted: the trained cart-pole fixture in a 256-plant loop of 100 steps, positions
                       measured; RMS estimate error and nis / p of the EKF and the UKF at the same Qn / Rn
B, REPS, PLANTS, STEPS from the environment.  One JSON line per result."""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("PACKAGE_ROOT", HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol  # noqa: E402
from phnn_mpc_amd import _capi, closed_loop  # noqa: E402
from phnn_mpc_amd.engine import RolloutEngine  # noqa: E402
from phnn_mpc_amd import estimation  # noqa: E402

mode = os.environ.get("MODE", "sigma")
reps = int(os.environ.get("REPS", 20))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
dev = "cuda:0"
KW = dict(Qn=[1e-8, 1e-8, 1e-5, 1e-5], P0=1e-4)


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


if mode in ("sigma", "moments", "step"):
    B = int(os.environ.get("B", 4096 if mode == "step" else 65536))
    which, integ = os.environ.get("FILTER", "ukf"), os.environ.get("INTEG", "euler")
    eng = RolloutEngine(ol.load_weights("phnn_cartpole"), dev)
    rng = np.random.default_rng(0)
    cls = estimation.UKF if which == "ukf" else estimation.EKF
    est = cls(measured=(0, 1), Rn=[1e-4, 2.5e-5], **dict(KW, P0=1e-3))
    opt = est.options(4)
    x = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.2, 0.3, 0.3])).astype(np.float32), device=dev)
    y = x + 0.01 * torch.randn(B, 4, device=dev)
    P = torch.tensor(est.initial(np.zeros((B, 4)))[1], device=dev)
    u = torch.tensor(rng.uniform(-5, 5, size=(B, 20, 1)).astype(np.float32), device=dev)
    if mode == "sigma":
        chi = torch.empty(B, 9, 4, dtype=torch.float32, device=dev)
        ctrl = torch.empty(B, 9, 1, 1, dtype=torch.float32, device=dev)
        us = timed(lambda: eng.ukf_sigma(x, P, opt, u=u, u_stride=20, chi=chi, ctrl=ctrl))
        res = dict(mode=mode, B=B, n=4, host_us_per_launch=us, failed=int(torch.isnan(chi).any(dim=2).any(dim=1).sum()))
    elif mode == "moments":
        traj = torch.tensor(rng.normal(size=(B * 9, 2, 4)).astype(np.float32), device=dev)
        xm = torch.empty(B, 4, dtype=torch.float32, device=dev)
        Pm, eye = torch.empty(B, 4, 4, dtype=torch.float64, device=dev), torch.empty(B, 4, 4, dtype=torch.float32, device=dev)
        us = timed(lambda: eng.ukf_moments(traj.reshape(-1)[4:], B, opt, Y_stride=8, xm=xm, Pm=Pm, eye=eye))
        res = dict(mode=mode, B=B, n=4, host_us_per_launch=us)
    else:
        cost = _capi.make_cost(4, 1, [10.0, 100.0, 1.0, 10.0], 0.01, None, -10.0, 10.0)
        xhat, ws = x.clone(), {}
        nis = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        step = eng.ukf_step if which == "ukf" else eng.ekf_step
        us = timed(lambda: step(xhat, P, u, 20, y, cost, integ, 0.02, opt, nis=nis, status=status, workspace=ws))
        size = eng.ukf_workspace_bytes(B) if which == "ukf" else eng.ekf_workspace_bytes(B)
        res = dict(mode=mode, filter=which, integrator=integ, B=B, host_us_per_step=us, failed=int((status != 0).sum()), workspace_bytes=size)
    print(json.dumps(res), flush=True)
elif mode == "loop":
    B, T, est = int(os.environ.get("PLANTS", 4096)), int(os.environ.get("STEPS", 100)), int(os.environ.get("EST", "0"))
    c = controller("phnn_cartpole")
    rng = np.random.default_rng(0)
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    sc = closed_loop.PlantScenario(meas_sigma=[0.002, 0.002, 0.05, 0.05], seed=0x9E3779B97F4A7C15)
    kw = dict(scenario=sc)
    rn = dict(measured=(0, 1, 2, 3), Rn=[4e-6, 4e-6, 2.5e-3, 2.5e-3])
    if est == 1:
        kw["estimator"] = estimation.EKF(**rn, **KW)
    elif est == 2:
        kw["estimator"] = estimation.UKF(**rn, **KW)
    closed_loop.DeviceClosedLoop(c, X[:64], 3, **kw).run()  # warm-up: kernels loaded, workspaces sized
    run_s = []
    for _ in range(3):
        loop = closed_loop.DeviceClosedLoop(c, X, T, use_graph=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run()
        run_s.append(time.perf_counter() - t0)
    failed = int((out["ekf_status"] == 2).sum()) if est else 0
    print(json.dumps(dict(mode=mode, root=os.path.relpath(ROOT, HERE), estimator=est, plants=B, steps=T, iters=c.max_iterations,
                          run_s=float(np.median(run_s)), run_s_all=run_s, surviving=float((out["done_step"] < 0).mean()),
                          filter_failed=failed,
                          controls_sha1=hashlib.sha1(np.ascontiguousarray(out["controls"]).tobytes()).hexdigest()[:16])), flush=True)
elif mode == "demo":
    B, T = int(os.environ.get("PLANTS", 256)), int(os.environ.get("STEPS", 100))
    c = controller("phnn_cartpole_trained")
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    pos = dict(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-4, 1e-4], Rn=[4e-6, 4e-6], P0=1e-4)
    for name, est in (("EKF", estimation.EKF(**pos)), ("UKF", estimation.UKF(**pos))):
        sc = closed_loop.PlantScenario(meas_sigma=[0.002, 0.002, 0.0, 0.0], seed=0xE57)
        out = closed_loop.run_mpc_batch_device(c, X, T, scenario=sc, estimator=est)
        err = out["estimates"][1:].astype(np.float64) - out["states"][1:]
        ds = out["done_step"]  # row t + 1 is the state after step t: alive while no plant limit has been passed before it
        alive = (ds[None, :] < 0) | (np.arange(T)[:, None] <= ds[None, :])
        ok = alive & np.isfinite(err).all(axis=2)
        print(json.dumps(dict(mode=mode, case=name, plants=B, steps=T,
                              rms_estimate_until_termination=[float(v) for v in np.sqrt((err[ok] ** 2).mean(axis=0))],
                              plant_steps_until_termination=int(alive.sum()), of_them_finite=int(ok.sum()),
                              mean_nis_over_p_until_termination=float(np.nanmean(out["nis"][ok]) / 2),
                              filter_failed=int((out["ekf_status"] == 2).sum()), surviving=float((out["done_step"] < 0).mean()))), flush=True)
else:
    raise SystemExit(f"unknown MODE {mode}")
