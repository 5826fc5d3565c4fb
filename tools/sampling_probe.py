#!/usr/bin/env python3
"""Timing probe of the sampling solves, MPPI and CEM (DESIGN.md sections 12 and 13): per-iteration time split into k_sample /
K1 / k_mppi_update or k_cem_update, the sample and update kernels' algorithmic bytes against the achievable HBM rate, K1
inside an iteration against a plain K1 of the same batch, and the single-plant / closed-loop latencies.

  python tools/sampling_probe.py --method mppi|cem --shape 1024x64 [--H 50] [--elites 8] [--reps 20]   one JSON line per measurement
  python tools/sampling_probe.py --method cem --shape 1024x64 --loop   also: one plant graphed, 4096 plants x 100 closed-loop steps
  python tools/sampling_probe.py --method mppi --shape 4096x256 --noise ar1:0.9|colored:2|knots:8   shaped noise
  rocprofv3 --kernel-trace --stats -d profiles/mppi_1024x64 -- python tools/sampling_probe.py --method mppi --shape 1024x64 --reps 5

Times are device events around `reps` back-to-back launches of one phase (median of 5 such groups), after a warm-up.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_TBS = 6.3  # achievable HBM rate DESIGN.md section 11 uses


def timed(torch, fn, reps, groups=5):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(groups):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return float(np.median(out)), float(min(out)), float(max(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", required=True, choices=("mppi", "cem"))
    ap.add_argument("--shape", default="1024x64", help="BxK")
    ap.add_argument("--H", type=int, default=50)
    ap.add_argument("--elites", type=int, default=8, help="cem only")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--noise", default=None, help="shaped noise: ar1:RHO | colored:BETA | knots:COUNT (default: white)")
    ap.add_argument("--loop", action="store_true", help="also: one plant H=20 K=64 iters=4 graphed, 4096 plants x 100 steps")
    a = ap.parse_args()
    import torch
    import yaml
    import oracle_lib as ol
    from phnn_mpc_amd.engine import RolloutEngine
    B, K = (int(x) for x in a.shape.split("x"))
    H, E, M = a.H, a.elites, a.method
    eng = RolloutEngine(ol.load_weights("phnn_cartpole"), "cuda:0")
    cost = ol.cost_from_golden(ol.load_golden("phnn_cartpole"))
    rng = np.random.default_rng(0)
    x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * [1.0, 0.3, 0.5, 0.5]).astype(np.float32), device="cuda")
    u = torch.zeros(B, H, 1, device="cuda")
    ws = {}
    R, N, n = B * K, H * eng.m, eng.n
    nkw = {}  # the `noise` keyword of the sample and solve calls
    if a.noise:
        from phnn_mpc_amd import noise as nz
        kind, _, arg = a.noise.partition(":")
        L = {"ar1": lambda: nz.ar1(H, float(arg)), "colored": lambda: nz.colored(H, float(arg)),
             "knots": lambda: nz.knots(H, int(arg))}[kind]()
        nkw = {"noise": nz.Noise(L)}
    # per method: the three calls, the closed-loop config, and the algorithmic bytes of sample and update
    if M == "mppi":
        sample = lambda: eng.mppi_sample(x0, u, cost, K, 2.0, 1, 0, workspace=ws, **nkw)
        update = lambda: eng.mppi_update(u, v, s, 50.0, cost, best_cost=bc, best_u=bu)
        solve = lambda: eng.solve_mppi(x0, u, cost, "euler", 0.02, iters=4, samples=K, lam=50.0, sigma=2.0, seed=1,
                                       record_costs=False, workspace=ws, **nkw)
        config = dict(optimizer="MPPI", samples=64, lam=50.0, sigma=3.0, seed=1, optimizer_steps=4)
        by_s = 4 * (R * N + B * N + R * n + B * n)          # samples written, nominal read, x0 replicated
        by_u = 4 * (R * N + 2 * R + 2 * B * N + 2 * B)      # samples read, costs read twice (L2), nominal + best written
    else:
        sig = torch.full((B, H, 1), 2.0, device="cuda")
        u2, sig2 = u.clone(), sig.clone()  # the update works in place: alpha = 0.25 keeps both in range over the repetitions
        sample = lambda: eng.cem_sample(x0, u, sig, cost, K, 1, 0, workspace=ws, **nkw)
        update = lambda: eng.cem_update(u2, sig2, v, s, E, 0.25, 0.05, cost, best_cost=bc, best_u=bu)
        solve = lambda: eng.solve_cem(x0, u, cost, "euler", 0.02, iters=4, samples=K, elites=E, alpha=0.25, sigma=2.0,
                                      sigma_min=0.05, seed=1, record_costs=False, workspace=ws, **nkw)
        config = dict(optimizer="CrossEntropy", samples=64, elites=8, alpha=0.25, sigma=3.0, sigma_min=0.05, seed=1,
                      optimizer_steps=4)
        by_s = 4 * (R * N + 2 * B * N + R * n + B * n)          # samples written, mean + sigma read, x0 replicated
        by_u = 4 * (2 * B * E * N + 35 * R + 4 * B * N + 2 * B)  # elite rows read twice, costs read 35 x (L2), mean + sigma read + written
    v, x0r = sample()
    s = eng.rollout_cost(x0r, v, cost, "euler", 0.02)
    bc, bu = torch.full((B,), float("inf"), device="cuda"), torch.zeros_like(u)
    res = {"shape": a.shape, "H": H, **({"elites": E} if M == "cem" else {}), "rollouts": R, "variant": eng.variant,
           "noise": a.noise or "white", **({"P": nkw["noise"].P} if nkw else {})}
    t_s = timed(torch, sample, a.reps)
    t_u = timed(torch, update, a.reps)
    # K1 on the sample tensor (what an iteration launches) and on an ordinary (R, H, m) batch, alternating
    xr, ur = x0r.clone(), (torch.rand(R, H, 1, device="cuda") - 0.5) * 10
    k1 = {M: [], "plain": []}
    for _ in range(3):
        k1[M].append(timed(torch, lambda: eng.rollout_cost(x0r, v, cost, "euler", 0.02), a.reps, 3)[0])
        k1["plain"].append(timed(torch, lambda: eng.rollout_cost(xr, ur, cost, "euler", 0.02), a.reps, 3)[0])
    t_k = float(np.median(k1[M]))
    res.update(sample_ms=t_s[0], k1_ms=t_k, update_ms=t_u[0], k1_plain_ms=float(np.median(k1["plain"])),
               **{f"k1_{M}_runs_ms": k1[M]}, k1_plain_runs_ms=k1["plain"],
               new_kernels_share=(t_s[0] + t_u[0]) / (t_s[0] + t_k + t_u[0]),
               sample_bytes=by_s, update_bytes=by_u, sample_TBs=by_s / t_s[0] / 1e9, update_TBs=by_u / t_u[0] / 1e9,
               sample_of_hbm=by_s / t_s[0] / 1e9 / HBM_TBS, update_of_hbm=by_u / t_u[0] / 1e9 / HBM_TBS,
               k1_us_per_1k_rollouts=1e3 * t_k / (R / 1e3))
    t_it = timed(torch, solve, max(a.reps // 4, 1))
    res["solve_4_iters_ms"] = t_it[0]
    print(json.dumps(res), flush=True)
    if a.loop:
        import time
        from phnn_mpc_amd.closed_loop import run_mpc_batch_device
        from phnn_mpc_amd.models import pHNN
        from phnn_mpc_amd.mpc_controller import create_mpc_from_config
        cfgp = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
        cfg = yaml.safe_load(open(cfgp))
        cfg["mpc"].update(config)
        if nkw:
            kind, _, arg = a.noise.partition(":")
            cfg["mpc"]["noise"] = {"type": kind, {"ar1": "rho", "colored": "beta", "knots": "count"}[kind]: float(arg) if kind != "knots" else int(arg)}
        m = pHNN(cfgp)
        m.load_state_dict({k: torch.tensor(w) for k, w in ol.load_weights("phnn_cartpole").items()})
        c = create_mpc_from_config(m, cfg)
        c.use_graph = True
        one = np.array([[0.0, 0.1, 0.0, 0.0]], np.float32)
        c.compute_control_batch(one, epoch=0)
        lat = []
        for e in range(1, 51):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.compute_control_batch(one, epoch=e)
            lat.append(1e3 * (time.perf_counter() - t0))
        X = rng.uniform(-1, 1, size=(4096, 4)) * [0.2, 0.08, 0.1, 0.1]
        run_mpc_batch_device(c, X[:64], 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_mpc_batch_device(c, X, 100, use_graph=True)
        loop_s = time.perf_counter() - t0
        print(json.dumps({"one_plant_H20_K64_iters4_graphed_ms": float(np.median(lat)), "closed_loop_4096x100_s": loop_s}),
              flush=True)


if __name__ == "__main__":
    main()
