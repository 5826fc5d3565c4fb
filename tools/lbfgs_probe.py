#!/usr/bin/env python3
"""k_lbfgs, the batched L-BFGS slot kernel (phnn_solve_lbfgs), at scale.

  python tools/lbfgs_probe.py run        one solve of B problems (B=, H=, HS= history size, SLOTS= iterations; no
                                         tolerance breaks, so every problem iterates in every slot).  Run it under
                                         `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`, one shape
                                         per run.
  python tools/lbfgs_probe.py report DIR B H HS
                                         reads DIR's kernel trace: mean k_lbfgs time over the slots whose history is
                                         full (slot >= HS + 1), algorithmic bytes per call, fraction of 6.3 TB/s, and
                                         the share of a slot k_lbfgs takes next to K1 + K2.
  python tools/lbfgs_probe.py latency    one plant, G13 controller: device solve (HIP graph) vs host compute_control;
                                         then 4096 plants x 100 closed-loop steps with the L-BFGS controller.
"""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM = 6.3e12


def lbfgs_bytes(B, H, m, hs):
    """Bytes one k_lbfgs call moves once the history holds hs pairs (every problem active)."""
    N = H * m
    Np = (N + 3) // 4 * 4
    per = (hs * (2 * Np * 4 + 4) + hs * 4   # loop 1: s, y, ro; al written
           + hs * (2 * Np * 4 + 4 + 4)      # loop 2: y, s, ro, al
           + 2 * Np * 4                     # new (s, y) pair + ro
           + N * 4 + 4                      # grad, cost
           + 2 * Np * 4 + 2 * Np * 4        # prev_g, d: read + write
           + 2 * N * 4                      # u: read + write
           + 2 * 48 + 8)                    # per-problem scalars, counters
    return B * per


def run():
    import torch
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import RolloutEngine
    with np.load(os.path.join(ROOT, "tests", "golden", "weights_phnn_cartpole.npz")) as z:
        w = {k: z[k] for k in z.files}
    eng = RolloutEngine(w)
    B, H = int(os.environ.get("B", 65536)), int(os.environ.get("H", 50))
    hs, slots = int(os.environ.get("HS", 100)), int(os.environ.get("SLOTS", 110))
    cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], [0.01], None, -15.0, 15.0)
    rng = np.random.default_rng(0)
    x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.1, 0.3, 0.3])).astype(np.float32), device="cuda")
    u0 = torch.zeros(B, H, 1, device="cuda")
    kw = dict(lr=0.05, outer_steps=1, max_iter=slots, max_eval=2 * slots, tolerance_grad=0.0, tolerance_change=0.0,
              history_size=hs, record_costs=True)
    ws = {}
    eng.solve_lbfgs(x0, u0, cost, "euler", 0.02, workspace=ws, **dict(kw, max_iter=2))  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.solve_lbfgs(x0, u0, cost, "euler", 0.02, workspace=ws, **kw)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    fin = eng.rollout_cost(x0, out["u_last"], cost)
    print(f"{eng.variant} B={B} H={H} history={hs} slots={slots}: {el * 1e3:.1f} ms per solve "
          f"({el / slots * 1e3:.3f} ms per slot of K1 + K2 + k_lbfgs); n_iter min {int(out['n_iter'].min())}, "
          f"mean cost {float(out['costs'][0].mean()):.3f} -> {float(fin.mean()):.3f}")


def report(d, B, H, hs):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9
    lb = [dur(r) for r in rows if "k_lbfgs" in r["Kernel_Name"]]
    fwd = [dur(r) for r in rows if "k_rollout_fwd" in r["Kernel_Name"]]
    grd = [dur(r) for r in rows if "k_rollout_grad" in r["Kernel_Name"]]
    full = lb[2 + hs + 1:] or lb[-5:]  # after the warm-up solve (2 slots) and the hs + 1 slots that fill the history
    t = float(np.mean(full))
    nbytes = lbfgs_bytes(B, H, 1, hs)
    k12 = float(np.mean(fwd[-len(full):]) + np.mean(grd[-len(full):]))
    print(f"k_lbfgs B={B} H={H} history={hs}: {t * 1e3:.3f} ms per call over {len(full)} calls with a full history "
          f"(min {min(full) * 1e3:.3f}, max {max(full) * 1e3:.3f}); {nbytes / 1e9:.3f} GB algorithmic -> "
          f"{nbytes / t / 1e12:.2f} TB/s = {nbytes / t / HBM * 100:.0f} % of 6.3 TB/s; "
          f"K1 + K2 {k12 * 1e3:.3f} ms: k_lbfgs is {t / (t + k12) * 100:.0f} % of a slot")


def latency():
    import torch
    from phnn_mpc_amd.closed_loop import run_mpc_batch_device
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import MPCController
    m = pHNN(os.path.join(ROOT, "configs", "cartpole_mpc.yaml"))
    with np.load(os.path.join(ROOT, "tests", "golden", "weights_phnn_cartpole.npz")) as z:
        m.load_state_dict({k: torch.tensor(z[k]) for k in z.files})
    g13 = dict(horizon=20, dt=0.02, Q=[10.0, 200.0, 1.0, 10.0], R=0.01, target_state=[0.0] * 4, u_min=-15.0, u_max=15.0,
               optimizer_type="LBFGS", lr=0.5, max_iterations=3)
    c = MPCController(phnn_model=m, **g13)
    x = np.array([0.1, 0.05, 0.0, 0.0], np.float32)
    for _ in range(3):
        c.compute_control(x)
    reps = 20
    t0 = time.perf_counter()
    for _ in range(reps):
        c.compute_control(x)
    host = (time.perf_counter() - t0) / reps
    c.use_graph = True
    for _ in range(3):
        c.compute_control_batch(x[None])
    t0 = time.perf_counter()
    for _ in range(reps):
        c.compute_control_batch(x[None])
    dev = (time.perf_counter() - t0) / reps
    print(f"one plant, G13 (H=20, lr=0.5, 3 x LBFGS(max_iter=20)): host compute_control {host * 1e3:.2f} ms, "
          f"device solve (HIP graph, 60 slots) {dev * 1e3:.2f} ms per solve")
    rng = np.random.default_rng(0)
    X0 = rng.uniform(-1, 1, size=(4096, 4)) * np.array([0.5, 0.1, 0.3, 0.3])
    run_mpc_batch_device(c, X0, 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = run_mpc_batch_device(c, X0, 100)
    el = time.perf_counter() - t0
    print(f"closed loop, 4096 plants x 100 steps, L-BFGS controller (device loop, graph): {el:.2f} s "
          f"({el / 100 * 1e3:.1f} ms per control step); plants terminated: {int((out['done_step'] >= 0).sum())}")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "run"
    if mode == "run":
        run()
    elif mode == "report":
        report(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    else:
        latency()
