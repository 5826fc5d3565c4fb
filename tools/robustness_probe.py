#!/usr/bin/env python3
"""Robustness probe of the device closed loop under plant scenarios: 4096 cart-poles x 100 control
steps whose cart mass, pole mass and pole length are spread +-20 % about the model's, with Gaussian force noise of
standard deviation 0.5, a freeze at termination and the metrics kept by the plant step -- no logs.  Per controller (Adam,
MPPI, CEM): the fraction of plants that survive, the mean closed-loop cost of the survivors, the fraction that meets the
config's stability criterion, and the wall time of the graphed loop.

  python tools/robustness_probe.py [--plants 4096] [--steps 100] [--spread 0.2] [--force-sigma 0.5]   one JSON line per controller
  python tools/robustness_probe.py --plain     the same loops through phnn_plant_step: no scenario, no metrics, logs kept

Each loop is run three times after a short warm-up run; the times are wall-clock seconds of DeviceClosedLoop.run()
(capture of the control step, steps - 1 replays, one synchronisation) and of building the loop (allocations, uploads).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONTROLLERS = {
    "Adam": dict(optimizer="Adam"),  # the config's 30 iterations
    "MPPI": dict(optimizer="MPPI", samples=64, lam=50.0, sigma=3.0, seed=1, optimizer_steps=4),
    "CEM": dict(optimizer="CrossEntropy", samples=64, elites=8, alpha=0.25, sigma=3.0, sigma_min=0.05, seed=1, optimizer_steps=4),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plants", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--spread", type=float, default=0.2, help="relative spread of masscart, masspole and length")
    ap.add_argument("--force-sigma", type=float, default=0.5)
    ap.add_argument("--plain", action="store_true", help="phnn_plant_step: no scenario, no metrics, with logs")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--weights", default="phnn_cartpole", help="fixture weights under tests/golden (phnn_cartpole_trained: the trained model)")
    a = ap.parse_args()
    import torch
    import yaml
    import oracle_lib as ol
    from phnn_mpc_amd import closed_loop
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    cfgp = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
    rng = np.random.default_rng(0)
    B, T = a.plants, a.steps
    X = rng.uniform(-1, 1, size=(B, 4)) * [0.2, 0.08, 0.1, 0.1]
    kw = {}
    if not a.plain:
        rel = {"masscart": a.spread, "masspole": a.spread, "length": a.spread}
        sc = closed_loop.PlantScenario(params=closed_loop.PlantScenario.spread(B, rel, rng), force_sigma=a.force_sigma,
                                       seed=0x9E3779B97F4A7C15, freeze_done=True)
    for name, over in CONTROLLERS.items():
        cfg = yaml.safe_load(open(cfgp))
        cfg["mpc"].update(over)
        if not a.plain:
            kw = dict(scenario=sc, metrics=cfg.get("stability", True), log=False)
        m = pHNN(cfgp)
        m.load_state_dict({k: torch.tensor(w) for k, w in ol.load_weights(a.weights).items()})
        c = create_mpc_from_config(m, cfg)
        warm = dict(kw)
        if not a.plain:
            warm["scenario"] = closed_loop.PlantScenario(params=sc.params[:64], force_sigma=a.force_sigma, seed=sc.seed, freeze_done=True)
        closed_loop.DeviceClosedLoop(c, X[:64], 3, **warm).run()  # warm-up: kernels loaded, workspaces sized
        build_s, run_s = [], []
        for _ in range(a.runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop = closed_loop.DeviceClosedLoop(c, X, T, use_graph=True, **kw)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = loop.run()
            run_s.append(time.perf_counter() - t1)
            build_s.append(t1 - t0)
        alive = out["done_step"] < 0
        res = {"controller": name, "weights": a.weights, "plants": B, "steps": T, "plain": a.plain, "iters": c.max_iterations,
               "run_s": float(np.median(run_s)), "run_s_all": run_s, "build_s": float(np.median(build_s)),
               "plant_steps_per_s": B * T / float(np.median(run_s)), "surviving": float(alive.mean())}
        if not a.plain:
            res.update(spread=a.spread, force_sigma=a.force_sigma, stable=float(out["stable"].mean()),
                       mean_cost_of_survivors=float(out["cost"][alive].mean()) if alive.any() else None,
                       mean_cost_of_terminated=float(out["cost"][~alive].mean()) if (~alive).any() else None)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
