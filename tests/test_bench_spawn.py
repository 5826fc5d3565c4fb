"""bench.py --gpus N must produce N ranks by itself: the parent starts torch.distributed.run
as a child before anything touches the GPU and relays rank 0's JSON line.  Rehearsed here on CPU: gloo backend, the CPU
oracle behind the engine protocol (tests/oracle_engine.py) instead of RolloutEngine -- the line is marked rehearsal.
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(extra, env_extra=None, timeout=600):
    env = dict(os.environ)
    env["PYTHONPATH"] = HERE + os.pathsep + ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--rehearsal-engine", "oracle_engine:bench_rehearsal_engine",
           "--batch", "48", "--horizon", "6", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--global-batch", "37"] + extra
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def test_gpus2_spawns_two_ranks_and_reports_them():
    r = _run(["--gpus", "2", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["rehearsal"] is True
    assert line["config"]["global_batch"] == 96 and line["config"]["batch_per_gpu"] == 48
    assert line["config"]["collective_backend"] == "gloo" and "gloo all-gather" in line["config"]["workload"]
    assert "RCCL" not in line["config"]["workload"]
    assert line["scaling"] == "weak" and line["value"] > 0
    assert line["metric"] == "pHNN-MPC rollouts+grads/sec, cartpole H=6 batch=48"
    assert line["strong_scaling"]["global_batch"] == 37  # ragged split over the two ranks


def test_gpus1_runs_in_process_with_unchanged_line_shape():
    r = _run(["--gpus", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and "strong_scaling" not in line and line["config"]["collective_backend"] is None
    for key in ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline"):
        assert key in line


def test_world_size_mismatch_is_an_error_not_a_warning():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def test_plain_run_leaves_the_full_measurements_out():
    """Without --full the line carries the headline figure only: no strong-scaling run after the timed steps."""
    r = _run(["--gpus", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["steps"] == 2 and line["ms_per_step"] > 0
    for key in ("strong_scaling", "cpu_baseline", "cpu_baseline_torch", "other_modes"):
        assert key not in line


def test_dump_outputs_hold_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: float32 .npy files of what the timed path returned, equal to the same rollouts computed
    directly on bench.py's seeded inputs."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    import oracle_engine
    import oracle_lib as ol
    from phnn_mpc_amd import _capi

    r = _run(["--gpus", "1", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["cost.npy", "grad_u.npy", "rollout_index.npy"]
    out = {k: np.load(tmp_path / f"{k}.npy") for k in ("cost", "grad_u", "rollout_index")}
    assert out["cost"].dtype == np.float32 and out["grad_u"].dtype == np.float32
    assert out["cost"].shape == (48,) and out["grad_u"].shape == (48, 6, 1)
    assert np.array_equal(out["rollout_index"], np.arange(48, dtype=np.float64))
    x0, U = bench.synthetic_inputs(4, 48, 6, 0, 5.0)
    cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], [0.01], None, -15.0, 15.0)
    c, g = oracle_engine.bench_rehearsal_engine(ol.load_weights("phnn_cartpole")).rollout_cost_grad(x0, U, cost, "euler", 0.02)
    assert np.array_equal(out["cost"], np.asarray(c)) and np.array_equal(out["grad_u"], np.asarray(g))


def test_dump_outputs_sample_the_same_rollouts_when_over_budget(tmp_path, monkeypatch):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES", 1000)
    B = 100
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"cost": torch.arange(B, dtype=torch.float32),
                                               "grad_u": torch.arange(B * 6, dtype=torch.float32).reshape(B, 6, 1)})
    idx = np.load(tmp_path / "a" / "rollout_index.npy")
    cost, gu = np.load(tmp_path / "a" / "cost.npy"), np.load(tmp_path / "a" / "grad_u.npy")
    assert idx.dtype == np.float64 and len(idx) == 1000 // (4 + 24 + 8) and np.all(np.diff(idx) > 0)
    assert np.array_equal(cost, idx.astype(np.float32)) and np.array_equal(gu[:, 0, 0], 6 * cost)
    assert np.array_equal(np.load(tmp_path / "b" / "rollout_index.npy"), idx)  # a fixed sample, run to run
