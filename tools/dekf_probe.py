#!/usr/bin/env python3
"""Timing and demonstration probe of the disturbance-augmented filter.  One mode per run, so that a
`rocprofv3 --kernel-trace --stats` trace holds one setting:
  MODE=update          k_dekf_update<4,1> alone: B = 65 536 problems, two measured components
  MODE=step            phnn_dekf_step (k_dekf_controls, K1 with H = 1, the linearisation, k_dekf_update): B = 4096
  MODE=loop EST=0|1|2  DeviceClosedLoop, 4096 plants x 100 control steps (the config's Adam controller, graph per control
                       step, measurement noise on): no estimator / the plain EKF / the DisturbanceEKF with compensation;
                       wall time of run(), three runs, and a hash of the controls.  PACKAGE_ROOT: the tree whose package
                       is imported (default: this one), so that the same probe times another checkout of the library
  MODE=demo            recorded, not asserted: the trained cart-pole fixture in a 256-plant loop of 100 steps, a force
                       bias of -2 .. +2 N per plant, positions measured: dhat against the injected bias, closed-loop cost
                       and stable-plant count with compensation on / off, with the plain EKF and with no estimator
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

mode = os.environ.get("MODE", "update")
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


if mode in ("update", "step"):
    B = int(os.environ.get("B", 65536 if mode == "update" else 4096))
    eng = RolloutEngine(ol.load_weights("phnn_cartpole"), dev)
    rng = np.random.default_rng(0)
    ekf = estimation.DisturbanceEKF(measured=(0, 1), Rn=[1e-4, 2.5e-5], Qd=1e-8, Pd0=1.0, **dict(KW, P0=1e-3))
    opt = ekf.options(4, 1)
    x = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.2, 0.3, 0.3])).astype(np.float32), device=dev)
    y = x + 0.01 * torch.randn(B, 4, device=dev)
    _, d0, Pz0 = ekf.initial(np.zeros((B, 4)), 1)
    Pz, dhat = torch.tensor(Pz0, device=dev), torch.tensor(d0, device=dev)
    nis = torch.empty(B, dtype=torch.float64, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    if mode == "update":
        A = torch.tensor((np.eye(4) + 0.02 * rng.normal(size=(B, 4, 4))).astype(np.float32), device=dev)
        Bm = torch.tensor((0.02 * rng.normal(size=(B, 4, 1))).astype(np.float32), device=dev)
        xhat = torch.empty_like(x)
        us = timed(lambda: eng.dekf_update(x, A, Bm, y, Pz, dhat, opt, xhat=xhat, nis=nis, innov=False, status=status))
        res = dict(mode=mode, B=B, n=4, m=1, measured=2, host_us_per_launch=us, failed=int((status != 0).sum()))
    else:
        u = torch.tensor(rng.uniform(-5, 5, size=(B, 20, 1)).astype(np.float32), device=dev)
        cost = _capi.make_cost(4, 1, [10.0, 100.0, 1.0, 10.0], 0.01, None, -10.0, 10.0)
        xhat, ws = x.clone(), {}
        us = timed(lambda: eng.dekf_step(xhat, dhat, Pz, u, 20, y, cost, "euler", 0.02, opt, nis=nis, status=status, workspace=ws))
        res = dict(mode=mode, B=B, host_us_per_step=us, failed=int((status != 0).sum()), workspace_bytes=eng.dekf_workspace_bytes(B))
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
        kw["estimator"] = estimation.DisturbanceEKF(Qd=1e-8, Pd0=1.0, **rn, **KW)
    closed_loop.DeviceClosedLoop(c, X[:64], 3, **kw).run()  # warm-up: kernels loaded, workspaces sized
    run_s = []
    for _ in range(3):
        loop = closed_loop.DeviceClosedLoop(c, X, T, use_graph=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = loop.run()
        run_s.append(time.perf_counter() - t0)
    print(json.dumps(dict(mode=mode, root=os.path.relpath(ROOT, HERE), estimator=est, plants=B, steps=T, iters=c.max_iterations,
                          run_s=float(np.median(run_s)), run_s_all=run_s, surviving=float((out["done_step"] < 0).mean()),
                          controls_sha1=hashlib.sha1(np.ascontiguousarray(out["controls"]).tobytes()).hexdigest()[:16])), flush=True)
elif mode == "demo":
    B, T = int(os.environ.get("PLANTS", 256)), int(os.environ.get("STEPS", 100))
    c = controller("phnn_cartpole_trained")
    rng = np.random.default_rng(1)
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    bias = np.linspace(-2.0, 2.0, B)
    sc = closed_loop.PlantScenario(force_bias=bias, meas_sigma=[0.002, 0.002, 0.0, 0.0], seed=0xE57)
    pos = dict(measured=(0, 1), Qn=[1e-8, 1e-8, 1e-4, 1e-4], Rn=[4e-6, 4e-6], P0=1e-4)
    cases = {
        "no estimator": None,
        "plain EKF": estimation.EKF(**pos),
        "DisturbanceEKF, compensate off": estimation.DisturbanceEKF(Qd=1e-6, Pd0=4.0, compensate=False, **pos),
        "DisturbanceEKF, compensate on": estimation.DisturbanceEKF(Qd=1e-6, Pd0=4.0, compensate=True, **pos),
    }
    for name, est in cases.items():
        out = closed_loop.run_mpc_batch_device(c, X, T, scenario=sc, metrics=True, **({} if est is None else {"estimator": est}))
        res = dict(mode=mode, case=name, plants=B, steps=T, mean_cost=float(np.mean(out["cost"])), median_cost=float(np.median(out["cost"])),
                   stable=int(out["stable"].sum()), surviving=int((out["done_step"] < 0).sum()))
        if "disturbances" in out:
            d = out["disturbances"][:, :, 0].astype(np.float64)
            ok = np.isfinite(d[-1])
            res.update(dhat_finite=int(ok.sum()), dhat_rms_error_end=float(np.sqrt(np.mean((d[-1][ok] - bias[ok]) ** 2))),
                       dhat_rms_error_step10=float(np.sqrt(np.nanmean((d[10] - bias) ** 2))),
                       dhat_bias_correlation_end=float(np.corrcoef(d[-1][ok], bias[ok])[0, 1]) if ok.sum() > 2 else None,
                       bias_rms=float(np.sqrt(np.mean(bias ** 2))), ekf_failed=int((out["ekf_status"] == 2).sum()))
        print(json.dumps(res), flush=True)
else:
    raise SystemExit(f"unknown MODE {mode}")
