#!/usr/bin/env python3
"""The bench workload (cart-pole pHNN, default f16x2, Euler, B=65536, H=50, K1 -> K2 stash) with and without a
per-problem time-varying reference (B, H+1, 4): K1 + K2 of each, alternating.  Run under
`rocprofv3 --kernel-trace --stats` for the per-kernel cost of the reference row load (k_rollout_fwd / k_rollout_grad
with and without the REF flag).  REF=0 runs only the plain kernels, REF=1 only the tracking ones, REF=both (default)
both."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phnn_mpc_amd import _capi
from phnn_mpc_amd.engine import RolloutEngine
with np.load(os.path.join(ROOT, "tests", "golden", "weights_phnn_cartpole.npz")) as z:
    w = {k: z[k] for k in z.files}
eng = RolloutEngine(w)
B, H, dt = int(os.environ.get("B", 65536)), int(os.environ.get("H", 50)), 0.02
cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], [0.01], None, -15.0, 15.0)
rng = np.random.default_rng(0)
x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([1.0, 0.3, 0.5, 0.5])).astype(np.float32), device="cuda")
U = torch.tensor(rng.uniform(-15, 15, size=(B, H, 1)).astype(np.float32), device="cuda")
t = np.arange(H + 1)[None, :, None]
x_ref = torch.tensor((rng.uniform(-0.5, 0.5, size=(B, 1, 4)) * np.cos(0.1 * t)).astype(np.float32), device="cuda")
mode = os.environ.get("REF", "both")
runs = {"0": [None], "1": [x_ref], "both": [None, x_ref]}[mode]
ws = {}
for r in runs:
    for _ in range(3):
        eng.rollout_cost_grad(x0, U, cost, "euler", dt, workspace=ws, x_ref=r)
torch.cuda.synchronize()
reps = int(os.environ.get("REPS", 20))
for r in runs:
    t0 = time.perf_counter()
    for _ in range(reps):
        eng.rollout_cost_grad(x0, U, cost, "euler", dt, workspace=ws, x_ref=r)
    torch.cuda.synchronize()
    el = (time.perf_counter() - t0) / reps
    print(f"{eng.variant} euler B={B} H={H} reference={'(B,H+1,4)' if r is not None else 'none'}: "
          f"{el * 1e3:.3f} ms per K1+K2, {B / el / 1e6:.2f} M rollouts+grads/s")
