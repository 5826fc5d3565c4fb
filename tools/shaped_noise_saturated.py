#!/usr/bin/env python3
"""The saturated start of DESIGN.md section 12 (u_init = 2 u_max, K = 64, 4 iterations, the shipped cart-pole controller)
with white, ar1(0.9) and colored(beta = 2) noise, MPPI and CEM: the cost the nominal / mean reaches and the best sample's
cost, on the device and in the float64 model (the CPU oracle engines of tests/shaped_noise_model.py).  One JSON line per
(method, noise, where).  DESIGN.md section 15 records the output.

  python tools/shaped_noise_saturated.py [--cpu-only]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-only", action="store_true", help="the float64 model only")
    a = ap.parse_args()
    import torch
    import yaml
    import oracle_lib as ol
    import shaped_noise_model as sn
    from test_cem_model import SAT as SAT_CEM
    from test_mppi_model import CFG, SAT as SAT_MPPI, SEED, X0
    from phnn_mpc_amd import noise
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.solver import cem_solve, mppi_solve
    w = ol.load_weights("phnn_cartpole")
    shapes = {"white": None, "ar1(0.9)": noise.Noise(noise.ar1(20, 0.9)), "colored(2)": noise.Noise(noise.colored(20, 2.0))}
    for where in ("float64 model",) + (() if a.cpu_only else ("device",)):
        m = pHNN(CFG)
        m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
        if where != "device":
            m.set_engine(sn.ShapedCemOracleEngine(w, "f64"))
        c = create_mpc_from_config(m, yaml.safe_load(open(CFG)))
        eng, cost = c.engine, c._cost()
        x0 = torch.tensor(X0[None]).to(eng.device)
        u_init = torch.full((1, 20, 1), 2.0 * float(cost.u_max), device=eng.device)
        c_sat = float(eng.rollout_cost(x0, torch.clamp(u_init, float(cost.u_min), float(cost.u_max)), cost, "euler", 0.02)[0])
        for meth, solve, sat in (("mppi", mppi_solve, SAT_MPPI), ("cem", cem_solve, SAT_CEM)):
            for name, shp in shapes.items():
                out = solve(eng, x0, u_init, cost, "euler", 0.02, seed=SEED, **sat, **({} if shp is None else {"noise": shp}))
                reached = float(eng.rollout_cost(x0, out["u_last"], cost, "euler", 0.02)[0])
                print(json.dumps({"where": where, "method": meth, "noise": name, "cost_saturated": c_sat, "cost_reached": reached,
                                  "best_sample_cost": float(out["best_cost"][0]),
                                  "nominal_costs": [float(v) for v in out["costs"][:, 0]]}), flush=True)


if __name__ == "__main__":
    main()
