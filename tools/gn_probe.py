#!/usr/bin/env python3
"""The batched Gauss-Newton solve (phnn_solve_gn) on the cart-pole pHNN (default f16x2).  Run under
`rocprofv3 --kernel-trace --stats`, one setting per run, for the per-kernel times of the five launches of an iteration
(k_rollout_linearize, k_gn_direction, k_gn_candidates, K1, k_gn_select):
  MODE=solve   B problems (default 4096), L line steps (default 16: B * L = 65 536 candidate rollouts), H = 50, ITERS
               iterations per solve, REPS solves
  MODE=one     one plant, H = 20, the solve captured as a HIP graph and replayed REPS times
  MODE=loop    B plants x T closed-loop steps of DeviceClosedLoop (graph per control step), OPT=GaussNewton or Adam (the
               reference configuration: lr 0.015, 30 iterations); GaussNewton runs ITERS iterations of L line steps
B, L, H, ITERS, REPS, T, OPT from the environment.  Prints the host time per repetition (device synchronised)."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phnn_mpc_amd import _capi, solver
from phnn_mpc_amd.engine import RolloutEngine

mode = os.environ.get("MODE", "solve")
B = int(os.environ.get("B", 1 if mode == "one" else 4096))
L = int(os.environ.get("L", 8 if mode != "solve" else 16))
H = int(os.environ.get("H", 20 if mode != "solve" else 50))
iters, reps, T = int(os.environ.get("ITERS", 4)), int(os.environ.get("REPS", 10)), int(os.environ.get("T", 100))
with np.load(os.path.join(ROOT, "tests", "golden", "weights_phnn_cartpole.npz")) as z:
    w = {k: z[k] for k in z.files}
rng = np.random.default_rng(0)
x0n = (rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.2, 0.3, 0.3])).astype(np.float32)


def timed(what, fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print(f"{what}: {dt * 1e3:.3f} ms per repetition ({n} repetitions)")
    return dt


if mode == "loop":
    import yaml
    from phnn_mpc_amd.closed_loop import run_mpc_batch_device
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "cartpole_mpc.yaml")))
    opt = os.environ.get("OPT", "GaussNewton")
    cfg["mpc"].update(horizon=H, optimizer=opt)
    if opt == "GaussNewton":
        cfg["mpc"].update(optimizer_steps=iters, gn_line_steps=L)
    model = pHNN(os.path.join(ROOT, "configs", "cartpole_mpc.yaml"))
    model.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    ctl = create_mpc_from_config(model, cfg)
    X = x0n.astype(np.float64) * 0.4
    out = {}

    def run():
        out.update(run_mpc_batch_device(ctl, X, T, use_graph=True, log=False, metrics=True))

    dt = timed(f"{opt} closed loop, {B} plants x {T} steps, H = {H}", run, max(reps // 5, 2))
    print(f"  closed-loop cost: mean {out['cost'].mean():.4f}, stable {int(out['stable'].sum())} of {B}, "
          f"{B * T / dt / 1e6:.3f} M plant-steps/s")
else:
    eng = RolloutEngine(w)
    cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], [0.01], None, -15.0, 15.0)
    x0 = torch.tensor(x0n, device="cuda")
    u0 = torch.zeros(B, H, 1, device="cuda")
    kw = dict(iters=iters, line_steps=L, record_costs=False)
    if mode == "one":
        graphed = solver.GraphedGN(eng)
        timed(f"graphed solve, one plant, H = {H}, {iters} iterations x {L} line steps",
              lambda: graphed(eng, x0, u0, cost, "euler", 0.02, **kw), reps)
    else:
        ws = {}
        dt = timed(f"solve, B = {B}, L = {L} ({B * L} candidates), H = {H}, {iters} iterations",
                   lambda: eng.solve_gn(x0, u0, cost, "euler", 0.02, workspace=ws, **kw), reps)
        print(f"  {dt / iters * 1e3:.3f} ms per iteration, set-up included")
        r = eng.solve_gn(x0, u0, cost, "euler", 0.02, iters=iters, line_steps=L)
        print(f"  mean cost {float(r['costs'][0].mean()):.3f} -> {float(r['cost'].mean()):.3f}, "
              f"accepted {float(r['accepts'].float().mean()):.2f} of {iters}")
