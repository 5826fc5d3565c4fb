#!/usr/bin/env python3
"""The step Jacobians (A_t, B_t) of the bench workload (cart-pole pHNN, default f16x2, B=65536, H=50) two ways, and the
two kernels that stand next to them.  Run under `rocprofv3 --kernel-trace --stats`, one setting per run, for the
per-kernel times:
  MODE=new       K1, then k_rollout_linearize on the stored trajectory (one launch)
  MODE=composed  the only way to the same numbers without it: K1 of the batch, then K1 of the B*H one-step rollouts and
                 n = 4 phnn_rollout_vjp launches over them with unit cotangents on x_1 (cost_bar = 0)
  MODE=point     k_model_jacobian at B points
  MODE=tvlqr     k_tvlqr at (B, H) on the (A, Bm) of MODE=new
INTEG=euler|rk4 (new / composed / tvlqr), B, H, REPS from the environment.  Prints the host time per repetition (device
synchronised) of each."""
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
mode, integ, reps = os.environ.get("MODE", "new"), os.environ.get("INTEG", "euler"), int(os.environ.get("REPS", 10))
cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], [0.01], None, -15.0, 15.0)
rng = np.random.default_rng(0)
x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([1.0, 0.3, 0.5, 0.5])).astype(np.float32), device="cuda")
U = torch.tensor(rng.uniform(-15, 15, size=(B, H, 1)).astype(np.float32), device="cuda")
_, traj = eng.rollout_cost(x0, U, cost, integ, dt, want_traj=True)


def new():
    return eng.rollout_linearize(x0, U, cost, integ, dt, traj=traj)


if mode == "composed":
    P = B * H
    x1, u1 = traj[:, :H].reshape(P, 4).contiguous(), U.reshape(P, 1, 1)
    tbs = []
    for i in range(4):
        tb = torch.zeros(P, 2, 4, device="cuda")
        tb[:, 1, i] = 1.0
        tbs.append(tb)
    zero = torch.zeros(P, device="cuda")
    tr1 = torch.empty(P, 2, 4, device="cuda")

    def run():
        eng.rollout_cost(x1, u1, cost, integ, dt, traj_out=tr1)
        return [eng.rollout_vjp(x1, u1, tr1, cost, integ, dt, traj_bar=tb, cost_bar=zero) for tb in tbs]
elif mode == "point":
    xp = x0
    up = U[:, 0].contiguous()

    def run():
        return eng.jacobian(xp, up)
elif mode == "tvlqr":
    A, Bm, _ = new()

    def run():
        return eng.tvlqr(A, Bm, cost)
else:
    run = new

for _ in range(2):
    out = run()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(reps):
    out = run()
torch.cuda.synchronize()
el = (time.perf_counter() - t0) / reps
what = {"new": f"k_rollout_linearize {integ}", "composed": f"K1 + 4 x phnn_rollout_vjp over {B * H} one-step rollouts, {integ}",
        "point": "k_model_jacobian", "tvlqr": f"k_tvlqr ({integ} linearisation)"}[mode]
print(f"{eng.variant} B={B} H={H} {what}: {el * 1e3:.3f} ms per repetition (host clock, allocations of the outputs included)")
if mode == "tvlqr":
    st = out["status"]
    print(f"  status != 0 for {int((st != 0).sum())} of {B} problems; K finite for {int(torch.isfinite(out['K']).all(dim=(1, 2, 3)).sum())}")
