#!/usr/bin/env python3
"""k_gn_direction_box against k_gn_direction at the timing shape of section 18: the cart-pole
pHNN, B = 4096 problems, H = 50, Euler.  Run under `rocprofv3 --kernel-trace --stats`, one setting per run:
  BOX=0           the plain direction
  BOX=1 CLAMP=0   the box direction with bounds nothing reaches (no clamped step)
  BOX=1 CLAMP=50  the box direction with the bound chosen (bisection on the kernel's own nclamp) so that about half of
                  the problem-steps hold their control on it
B, H, REPS from the environment.  Prints the share of clamped problem-steps and the host time per launch."""
import os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phnn_mpc_amd import _capi
from phnn_mpc_amd.engine import RolloutEngine

B, H, reps = int(os.environ.get("B", 4096)), int(os.environ.get("H", 50)), int(os.environ.get("REPS", 20))
box, clamp = os.environ.get("BOX", "1") == "1", int(os.environ.get("CLAMP", 0))
with np.load(os.path.join(ROOT, "tests", "golden", "weights_phnn_cartpole.npz")) as z:
    w = {k: z[k] for k in z.files}
eng = RolloutEngine(w, "cuda:0")
rng = np.random.default_rng(0)
x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.2, 0.3, 0.3])).astype(np.float32), device="cuda:0")
u = torch.zeros(B, H, 1, device="cuda:0")


def cost_of(limit):
    return _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], 0.01, None, -limit, limit)


def share(limit):
    c = cost_of(limit)
    A, Bm, traj = eng.rollout_linearize(x0, u, c, "euler", 0.02)
    return float(eng.gn_direction(A, Bm, traj, u, c, 1e-6, box=True)["nclamp"].sum()) / (B * H)


limit = 1e6
if box and clamp:
    lo, hi = 1e-3, 100.0
    for _ in range(30):  # the share falls as the bound widens
        mid = (lo * hi) ** 0.5
        lo, hi = (mid, hi) if share(mid) > clamp / 100.0 else (lo, mid)
    limit = hi
cost = cost_of(limit)
A, Bm, traj = eng.rollout_linearize(x0, u, cost, "euler", 0.02)
mu = torch.full((B,), 1e-6, dtype=torch.float64, device="cuda:0")
kw = {"box": True} if box else {}
out = eng.gn_direction(A, Bm, traj, u, cost, mu, **kw)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(reps):
    eng.gn_direction(A, Bm, traj, u, cost, mu, **kw)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / reps
held = float(out["nclamp"].sum()) / (B * H) if box else 0.0
print(f"box={int(box)} |u| <= {limit:.4g}: {100 * held:.1f} % of the problem-steps clamped, status != 0 on "
      f"{int((out['status'] != 0).sum())} problems, {dt * 1e6:.1f} us per launch (host, {reps} launches)")
