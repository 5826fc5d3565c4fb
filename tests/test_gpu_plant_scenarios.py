"""phnn_plant_step_ex (k_plant_step_ex): per-plant parameters, force disturbances, measurement noise, freeze at termination
and running metrics on the device plant, and the closed loops built on it.

Shapes: B = 1 / 19 / 257 (one plant, ragged, past one 256-thread block), 5 steps, action_stride 1 and 7, |state| <= 1 (asserted
on the host result), so the bounds of tests/test_gpu_plant_edges.py apply unchanged: 1e-13 absolute on the float64 state
against the numpy plant (the device's double-precision sin / cos), 2e-7 relative on state_f32, 1e-12 on closed-loop
states.  Everything else is compared bit for bit.

  1 identity     ex = metrics = NULL, a zero-initialised ex, params_dev filled with the shared constants: every output bit of
                 phnn_plant_step, a -0.0 command on an all-zero state included
  2 parameters   every plant its own four constants == the numpy plant run alone with them; each column alone moves the result
  3 disturbance  the numpy plant fed float64(uf) + float64(w_logged); w_logged bits == bias + sigma * z in numpy float32, z
                 the bits of the device's own white sampler (phnn_mppi_sample, K = 2, N = 8, epoch = step: row 2b + 1,
                 element 0); z against mppi_model.normals within the sampler's allowance
  4 measurement  state_f32 bits == float32(state) + meas_sigma_i * z_i (elements 4..7 of that row); state, logs and done_step
                 are those of the run without it; a component with sigma 0 is exactly float32(x_i)
  5 invariance   257 plants in one call == 100 + 157 with plant_offset; device step counter == host step index; another seed
                 changes the noise
  6 freeze       tight limits; a terminated plant keeps its state bits and its metrics stop, the others are the run without
                 freeze; without the flag nothing changes
  7 metrics      cost (1e-12 relative) and the run counters (exact) against numpy on the device's own logs; plants leave and
                 re-enter the band; a NaN state breaks the run; best_run == stability_report
  8 arguments    one bad field at a time: PHNN_ERR_INVALID_ARG, every buffer keeps its bits
  9 footprint    tests/footprint.py's guarded arena, every optional pointer given and each one NULL, B = 19 and 257
 10 closed loop  19 plants x 4 steps, H = 5, 3 iterations, Adam and MPPI: eager == graphed bit for bit, == run_mpc_batch with
                 replay= of the device's disturbance log; measurement noise: eager == graphed, the seed matters; log=False
                 returns the metrics of log=True
"""
import ctypes as C
import os

import numpy as np
import pytest
import yaml

import footprint as fp
import mppi_model as mm
import oracle_lib as ol
from test_gpu_mppi import allowance, engine
from test_gpu_plant_edges import DEFAULT, OTHER, against_host, bits32, bits64, plant_of, run_device, run_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
SEED = 0x5EED_0F_A_91A27
NAMES = ("gravity", "masscart", "masspole", "length")
T = 5


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def inputs(nb, steps, seed, f_lim=2.0):
    rng = np.random.default_rng(seed)
    init = rng.uniform(-1, 1, size=(nb, 4)) * [0.6, 0.2, 0.4, 0.4]
    return init, rng.uniform(-f_lim, f_lim, size=(steps, nb)).astype(np.float32)


def own_params(nb, seed, rel=0.3):
    """(nb,4): every plant its own gravity, masscart, masspole, length, within +-rel of the defaults."""
    base = np.array([DEFAULT[k] for k in NAMES])
    return base * (1.0 + rel * np.random.default_rng(seed).uniform(-1, 1, size=(nb, 4)))


def metric_spec(tol=(0.3, 0.1, 0.2, 0.3), target=(0.05, -0.02, 0.0, 0.01)):
    rng = np.random.default_rng(77)
    Q = np.diag([10.0, 100.0, 1.0, 10.0]) + 0.1 * rng.uniform(-1, 1, size=(4, 4))  # full and non-symmetric
    return dict(Q=Q, R=0.01, target=np.array(target, np.float64), tol=np.array(tol, np.float64))


def run_ex(torch, consts, init, forces, stride=1, bounds=None, step_dev=False, first_step=0, ex=None, metrics=None, null=False):
    """T steps of phnn_plant_step_ex, called through the C-ABI.  forces (T,B) float32; ex: None = a zero-initialised
    struct, or dict(params (B,4), bias (B,), force_sigma, meas_sigma (4,), seed, plant_offset, freeze, dlog bool);
    metrics: None or metric_spec() (+ run0 (B,)); null: ex = metrics = NULL.  -> run_device's dict + dlog (T,B), cost,
    run, best (B)."""
    from phnn_mpc_amd import _capi
    eng = engine("phnn_cartpole")
    nb, steps = init.shape[0], forces.shape[0]
    plant = plant_of(consts)
    dev = dict(device="cuda")
    state = torch.tensor(init, dtype=torch.float64, **dev)
    x32 = torch.full((nb, 4), -7.0, dtype=torch.float32, **dev)
    done = torch.full((nb,), -1, dtype=torch.int32, **dev)
    logs = torch.zeros(first_step + steps + 1, nb, 4, dtype=torch.float64, **dev)
    logc = torch.zeros(first_step + steps, nb, dtype=torch.float32, **dev)
    sd = torch.full((1,), first_step, dtype=torch.int32, **dev) if step_dev else None
    keep = {}
    e = _capi.PlantEx()
    ex = ex or {}
    if ex.get("params") is not None:
        keep["params"] = torch.tensor(ex["params"], dtype=torch.float64, **dev)
        e.params_dev = keep["params"].data_ptr()
    if ex.get("bias") is not None:
        keep["bias"] = torch.tensor(ex["bias"], dtype=torch.float32, **dev)
        e.force_bias_dev = keep["bias"].data_ptr()
    e.force_sigma = ex.get("force_sigma", 0.0)
    for i, v in enumerate(ex.get("meas_sigma", (0.0,) * 4)):
        e.meas_sigma[i] = v
    e.seed, e.plant_offset, e.freeze_done = ex.get("seed", 0), ex.get("plant_offset", 0), int(ex.get("freeze", False))
    dlog = None
    if ex.get("dlog"):
        dlog = torch.zeros(first_step + steps, nb, dtype=torch.float32, **dev)
        e.disturbance_log_dev = dlog.data_ptr()
    mt = None
    if metrics is not None:
        mt = _capi.PlantMetrics()
        for i in range(16):
            mt.Q[i] = float(metrics["Q"].reshape(-1)[i])
        mt.R = metrics["R"]
        for i in range(4):
            mt.target[i], mt.tol[i] = float(metrics["target"][i]), float(metrics["tol"][i])
        keep["cost"] = torch.zeros(nb, dtype=torch.float64, **dev)
        keep["run"] = torch.tensor(metrics.get("run0", np.zeros(nb)), dtype=torch.int32, **dev)
        keep["best"] = keep["run"].clone()
        mt.cost_acc_dev, mt.run_dev, mt.best_run_dev = keep["cost"].data_ptr(), keep["run"].data_ptr(), keep["best"].data_ptr()
    has_b = bounds is not None
    states, x32s = [], []
    for t in range(steps):
        a = torch.full((nb, stride), 1e30, dtype=torch.float32, **dev)
        a[:, 0] = torch.tensor(forces[t], **dev)
        rc = eng.lib.phnn_plant_step_ex(eng.h, C.byref(plant), None if null else C.byref(e), None if (null or mt is None) else C.byref(mt),
                                        eng._p(state), eng._p(a), stride, nb, int(has_b), bounds[0] if has_b else 0.0,
                                        bounds[1] if has_b else 0.0, eng._p(x32), eng._p(done), eng._p(sd),
                                        -5 if step_dev else first_step + t, eng._p(logs), eng._p(logc), eng._stream())
        fp.check_rc(eng, rc)
        if step_dev:
            eng.advance_step(sd)
        states.append(state.cpu().numpy().copy())
        x32s.append(x32.cpu().numpy().copy())
    out = dict(states=np.stack(states), x32=np.stack(x32s), logs=logs.cpu().numpy()[first_step:], logc=logc.cpu().numpy()[first_step:],
               done=done.cpu().numpy())
    if dlog is not None:
        out["dlog"] = dlog.cpu().numpy()[first_step:]
    if mt is not None:
        out.update(cost=keep["cost"].cpu().numpy(), run=keep["run"].cpu().numpy(), best=keep["best"].cpu().numpy())
    return out


def same_bits(a, b, keys=("states", "logs", "x32", "logc", "done")):
    for k in keys:
        f = bits64 if a[k].dtype == np.float64 else (bits32 if a[k].dtype == np.float32 else np.asarray)
        assert np.array_equal(f(a[k]), f(b[k])), k


_Z = {}


def sampler_row(torch, seed, step, offset, nb):
    """(nb, 8) float32: row 2b + 1 of the device's white sampler (u = 0, sigma = 1, no bounds, K = 2, N = 8) at epoch =
    step, iteration 0: element 0 is the force normal, elements 4..7 the measurement normals of plant offset + b."""
    from phnn_mpc_amd import _capi
    key = (seed, step, offset, nb)
    if key not in _Z:
        eng = engine("phnn_cartpole")
        cost = _capi.make_cost(4, 1, [1.0, 1.0, 1.0, 1.0], 0.01)
        assert not cost.has_u_bounds
        x0 = torch.zeros(nb, 4, dtype=torch.float32, device="cuda")
        u = torch.zeros(nb, 8, 1, dtype=torch.float32, device="cuda")
        v, _ = eng.mppi_sample(x0, u, cost, 2, 1.0, seed, 0, epoch=step, problem_offset=offset)
        _Z[key] = v.cpu().numpy().reshape(nb, 2, 8)[:, 1].copy()
    return _Z[key]


def sampler_rows(torch, seed, steps, offset, nb):
    return np.stack([sampler_row(torch, seed, t, offset, nb) for t in range(steps)])  # (T, nb, 8)


# ----------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("stride", [1, 7])
@pytest.mark.parametrize("nb", [1, 19, 257])
def test_nothing_extended_gives_the_bits_of_phnn_plant_step(torch, nb, stride):
    init, forces = inputs(nb, T, nb, f_lim=25.0)
    init[0] = 0.0
    forces[:, 0] = -0.0  # a -0.0 command on an all-zero state
    if nb > 2:
        forces[2, 2] = np.nan
    bounds = (-15.0, 15.0)
    for consts in (DEFAULT, OTHER):
        old = run_device(torch, consts, init, forces, stride, bounds=bounds)
        assert np.signbit(old["logc"][:, 0]).all()
        shared = np.tile([consts[k] for k in NAMES], (nb, 1))
        for kw in (dict(null=True), dict(), dict(ex=dict(params=shared)), dict(ex=dict(seed=SEED, plant_offset=5))):
            same_bits(run_ex(torch, consts, init, forces, stride, bounds=bounds, **kw), old)


# ----------------------------------------------------------------------------- 2. per-plant parameters
def host_alone(consts, params, init, forces):
    """The numpy plant, every plant run alone with its own four constants."""
    runs = [run_host(dict(consts, **dict(zip(NAMES, params[b]))), init[b:b + 1], forces[:, b:b + 1]) for b in range(len(init))]
    return {k: np.concatenate([r[k] for r in runs], axis=-1 if k == "done" else 1) for k in ("states", "done", "flags")}


@pytest.mark.parametrize("stride", [1, 7])
@pytest.mark.parametrize("nb", [1, 19, 257])
def test_per_plant_parameters_against_the_numpy_plant_run_alone(torch, nb, stride):
    init, forces = inputs(nb, T, 100 + nb)
    params = own_params(nb, nb)
    variants = [params]
    if nb == 19 and stride == 1:  # every column alone
        for k in range(4):
            one = np.tile([DEFAULT[n] for n in NAMES], (nb, 1))
            one[:, k] = params[:, k]
            variants.append(one)
    base = run_host(DEFAULT, init, forces)
    for p in variants:
        host = host_alone(DEFAULT, p, init, forces)
        assert np.abs(host["states"]).max() <= 1.0  # the range the 1e-13 bound is stated for
        dev = run_ex(torch, DEFAULT, init, forces, stride, ex=dict(params=p))
        against_host(dev, host, forces)
        assert not np.array_equal(host["states"], base["states"])  # the column matters on these inputs
    if nb == 19 and stride == 1:  # dt and the limits stay the shared ones
        tight = dict(OTHER, **{n: DEFAULT[n] for n in NAMES})
        host = host_alone(tight, params, init, forces)
        against_host(run_ex(torch, tight, init, forces, stride, ex=dict(params=params)), host, forces)
        assert (host["done"] >= 0).any() and (host["done"] < 0).any()


# ----------------------------------------------------------------------------- 3. disturbance
@pytest.mark.parametrize("case", ["bias+sigma", "bias", "sigma"])
@pytest.mark.parametrize("nb, stride", [(1, 1), (19, 7), (257, 1)])
def test_disturbance_is_logged_applied_and_the_samplers(torch, nb, stride, case):
    init, forces = inputs(nb, T, 200 + nb)
    bias = np.random.default_rng(nb).uniform(-1, 1, nb).astype(np.float32) if "bias" in case else None
    sigma = 0.5 if "sigma" in case else 0.0
    off = 1000
    dev = run_ex(torch, DEFAULT, init, forces, stride, ex=dict(bias=bias, force_sigma=sigma, seed=SEED, plant_offset=off, dlog=True))
    w = dev["dlog"]
    host = run_host(DEFAULT, init, forces.astype(np.float64) + w.astype(np.float64))
    assert np.abs(host["states"]).max() <= 1.0
    against_host(dev, host, forces)
    assert not np.array_equal(host["states"], run_host(DEFAULT, init, forces)["states"])
    z = sampler_rows(torch, SEED, T, off, nb)[:, :, 0]
    want = np.zeros((T, nb), np.float32) if bias is None else np.broadcast_to(bias, (T, nb)).copy()
    if sigma:
        want = want + np.float32(sigma) * z  # float32: the product rounded, then the sum
        gids = off + np.arange(nb)
        for t in range(T):
            z64, z32 = mm.normals(SEED, t, 0, gids, 2, 8, np.float64)[:, 1, 0], mm.normals(SEED, t, 0, gids, 2, 8, np.float32)[:, 1, 0]
            assert np.abs(z[t].astype(np.float64) - z64).max() <= allowance(z32, z64)
        assert len(np.unique(z)) == z.size  # fresh noise for every plant and step
    assert np.array_equal(bits32(w), bits32(want))


# ----------------------------------------------------------------------------- 4. measurement noise
@pytest.mark.parametrize("nb, stride", [(1, 1), (19, 7), (257, 1)])
def test_measurement_noise_reaches_state_f32_only(torch, nb, stride):
    init, forces = inputs(nb, T, 300 + nb)
    ms = np.array([0.01, 0.0, 0.03, 0.002], np.float32)
    quiet = run_ex(torch, OTHER, init, forces, stride, ex=dict(seed=SEED, plant_offset=3))
    noisy = run_ex(torch, OTHER, init, forces, stride, ex=dict(meas_sigma=ms, seed=SEED, plant_offset=3))
    same_bits(noisy, quiet, ("states", "logs", "logc", "done"))
    assert (quiet["done"] >= 0).any() or nb == 1  # OTHER's tight limits: termination is decided by the true state
    z = sampler_rows(torch, SEED, T, 3, nb)[:, :, 4:]
    x32 = noisy["states"].astype(np.float32)
    want = x32.copy()
    on = ms > 0
    want[:, :, on] = x32[:, :, on] + ms[on] * z[:, :, on]
    assert np.array_equal(bits32(noisy["x32"]), bits32(want))
    assert np.array_equal(bits32(noisy["x32"][:, :, 1]), bits32(x32[:, :, 1]))  # sigma 0: exactly float32(x_i)
    assert not np.any(noisy["x32"][:, :, on] == x32[:, :, on])


# ----------------------------------------------------------------------------- 5. invariance
def test_noise_follows_the_global_id_the_step_and_the_seed(torch):
    nb, cut = 257, 100
    init, forces = inputs(nb, T, 5)
    rng = np.random.default_rng(6)
    full = dict(params=own_params(nb, 7), bias=rng.uniform(-1, 1, nb).astype(np.float32), force_sigma=0.5,
                meas_sigma=(0.01, 0.02, 0.0, 0.01), seed=SEED, plant_offset=40, dlog=True)
    keys = ("states", "logs", "x32", "logc", "done", "dlog")
    whole = run_ex(torch, DEFAULT, init, forces, ex=full)
    parts = []
    for sl, off in ((slice(0, cut), 40), (slice(cut, nb), 40 + cut)):
        part = dict(full, params=full["params"][sl], bias=full["bias"][sl], plant_offset=off)
        parts.append(run_ex(torch, DEFAULT, init[sl], forces[:, sl], ex=part))
    joined = {k: np.concatenate([p[k] for p in parts], axis=0 if k == "done" else 1) for k in keys}
    same_bits(joined, whole, keys)
    same_bits(run_ex(torch, DEFAULT, init, forces, ex=full, step_dev=True, first_step=2),
              run_ex(torch, DEFAULT, init, forces, ex=full, first_step=2), keys)
    other = run_ex(torch, DEFAULT, init, forces, ex=dict(full, seed=SEED + 1))
    assert not np.any(other["dlog"] == whole["dlog"]) and not np.array_equal(other["x32"], whole["x32"])
    later = run_ex(torch, DEFAULT, init, forces, ex=full, first_step=2)
    assert np.array_equal(later["dlog"][:T - 2], whole["dlog"][2:])  # the noise of step s, whenever it is drawn


# ----------------------------------------------------------------------------- 6. freeze, 7. metrics
def metrics_np(logs, logc, spec, active, run0):
    """cost, run, best from logged states (T+1,B,4) and controls (T,B) in the kernel's operation order; active (T,B):
    the plant was stepped."""
    steps, nb = logc.shape
    cost, run = np.zeros(nb), np.array(run0, np.int64)
    best = run.copy()
    Q, R = spec["Q"], float(spec["R"])
    with np.errstate(invalid="ignore"):
        for t in range(steps):
            e = logs[t + 1] - spec["target"]
            c = np.zeros(nb)
            for i in range(4):
                for j in range(4):
                    c = c + (e[:, i] * Q[i, j]) * e[:, j]
            uf = logc[t].astype(np.float64)
            c = c + (uf * R) * uf
            ok = np.all(np.abs(e) <= spec["tol"], axis=1)
            a = active[t]
            cost = np.where(a, cost + c, cost)
            run = np.where(a, np.where(ok, run + 1, 0), run)
            best = np.maximum(best, run)
    return cost, run, best


def check_metrics(dev, spec, active, run0):
    cost, run, best = metrics_np(dev["logs"], dev["logc"], spec, active, run0)
    assert np.array_equal(np.isnan(dev["cost"]), np.isnan(cost))
    fin = ~np.isnan(cost)
    assert np.all(np.abs(dev["cost"][fin] - cost[fin]) <= 1e-12 * np.abs(cost[fin]))
    assert np.array_equal(dev["run"], run) and np.array_equal(dev["best"], best)
    return cost, run, best


@pytest.mark.parametrize("nb", [19, 257])
def test_freeze_keeps_terminated_plants_and_stops_their_metrics(torch, nb):
    consts = dict(DEFAULT, x_limit=0.45, theta_limit=0.15)
    init, forces = inputs(nb, T, 600 + nb)
    spec = metric_spec()
    noise = dict(force_sigma=0.3, seed=SEED, dlog=True)
    free = run_ex(torch, consts, init, forces, ex=dict(noise), metrics=spec)
    froz = run_ex(torch, consts, init, forces, ex=dict(noise, freeze=True), metrics=spec)
    done = free["done"]
    assert ((done >= 0) & (done < T - 1)).any() and (done < 0).any()  # some terminate early, some never
    assert np.array_equal(froz["done"], done)
    same_bits(froz, free, ("logc", "dlog"))  # the command and the computed disturbance are logged, applied or not
    steps = np.arange(T)[:, None]
    live = (done[None, :] < 0) | (steps <= done[None, :])  # (T,B): stepped under freeze
    for k in ("states", "x32"):
        f = bits64 if k == "states" else bits32
        assert np.array_equal(f(froz[k])[live], f(free[k])[live]), k
    last = np.where(done >= 0, done, T - 1)
    kept = froz["states"][last, np.arange(nb)]  # the state at termination
    for t in range(T):
        idle = ~live[t]
        assert np.array_equal(bits64(froz["states"][t][idle]), bits64(kept[idle]))
        assert np.array_equal(bits64(froz["logs"][t + 1][idle]), bits64(kept[idle]))  # the log row repeats it
        assert np.array_equal(bits32(froz["x32"][t][idle]), bits32(kept[idle].astype(np.float32)))
    assert (~live).any() and not np.array_equal(froz["states"][-1], free["states"][-1])
    check_metrics(froz, spec, live, np.zeros(nb))
    cost_free, _, _ = check_metrics(free, spec, np.ones((T, nb), bool), np.zeros(nb))
    early = (done >= 0) & (done < T - 1)
    assert np.all(froz["cost"][early] < cost_free[early]) and np.array_equal(froz["cost"][~early], free["cost"][~early])
    # without the flag the behaviour is today's
    same_bits(run_ex(torch, consts, init, forces), run_device(torch, consts, init, forces))


@pytest.mark.parametrize("nb", [1, 19, 257])
def test_metrics_against_numpy_on_the_logged_run(torch, nb):
    from phnn_mpc_amd.closed_loop import stability_report
    steps = 5
    rng = np.random.default_rng(700 + nb)
    init = rng.uniform(-1, 1, size=(nb, 4)) * [0.25, 0.08, 0.15, 0.2]
    forces = rng.uniform(-15, 15, size=(steps, nb)).astype(np.float32)  # x_dot moves by up to 0.27 a step: in and out of its band
    if nb > 1:
        init[0] = [0.0, 0.0, 0.19, 0.0]
        forces[:, 0] = [10.0, -10.0, 10.0, -10.0, 10.0]  # plant 0 leaves the x_dot band and re-enters it, twice
        init[1, 0] = np.nan  # a NaN state never counts
    if nb > 2:
        init[2] = [0.0, 0.0, 0.0, 0.0]
        forces[:, 2] = [0.0, 0.0, np.nan, 0.0, 0.0]  # in the band for two steps, then NaN for good
    spec = metric_spec()
    with np.errstate(invalid="ignore"):
        run0 = np.all(np.abs(init - spec["target"]) <= spec["tol"], axis=1).astype(np.int64)  # the initial state counts
    dev = run_ex(torch, DEFAULT, init, forces, metrics=dict(spec, run0=run0), null=False)
    cost, run, best = check_metrics(dev, spec, np.ones((steps, nb), bool), run0)
    logged = np.concatenate([init[None], dev["logs"][1:]])  # states 0..T: row 0 of the log is the caller's
    with np.errstate(invalid="ignore"):
        rep = stability_report(logged, spec["target"], spec["tol"], 0.05, 0.02)  # 3 steps
        ok = np.all(np.abs(logged - spec["target"]) <= spec["tol"], axis=2)  # (T+1,B)
    assert np.array_equal(dev["best"], np.rint(rep["longest_run_s"] / 0.02).astype(np.int64))
    assert np.array_equal(dev["best"] >= 3, rep["stable"])
    if nb > 1:
        assert ok[:, 0].tolist() == [True, False, True, False, True, False] and dev["best"][0] == 1 and dev["run"][0] == 0
        assert np.isnan(dev["cost"][1]) and dev["run"][1] == dev["best"][1] == 0 and dev["done"][1] == -1
        reenter = [(~ok[:i, b]).any() and ok[i:, b].any() and ok[:i, b].any() for b in range(nb) for i in range(1, steps + 1)]
        assert any(reenter)
    if nb > 2:
        assert run0[2] == 1 and dev["best"][2] == 3 and dev["run"][2] == 0 and np.isnan(dev["cost"][2])
        assert rep["stable"][2] and not rep["stable"][0]
    if nb > 19:
        assert rep["stable"].any() and not rep["stable"].all() and len(np.unique(dev["best"])) >= 4


# ----------------------------------------------------------------------------- 8. arguments
def test_bad_arguments_are_refused_and_nothing_is_written(torch):
    from phnn_mpc_amd import _capi
    eng = engine("phnn_cartpole")
    nb = 19
    rng = np.random.default_rng(8)
    dev = dict(device="cuda")
    t = dict(state=torch.tensor(rng.uniform(-0.3, 0.3, size=(nb, 4)), **dev), action=torch.tensor(rng.uniform(-2, 2, nb), dtype=torch.float32, **dev),
             x32=torch.full((nb, 4), -7.0, dtype=torch.float32, **dev), done=torch.full((nb,), -1, dtype=torch.int32, **dev),
             logs=torch.full((3, nb, 4), 5.0, dtype=torch.float64, **dev), logc=torch.full((2, nb), 5.0, dtype=torch.float32, **dev),
             dlog=torch.full((2, nb), 5.0, dtype=torch.float32, **dev), params=torch.tensor(own_params(nb, 1), **dev),
             bias=torch.ones(nb, dtype=torch.float32, **dev), cost=torch.full((nb,), 2.0, dtype=torch.float64, **dev),
             run=torch.full((nb,), 3, dtype=torch.int32, **dev), best=torch.full((nb,), 4, dtype=torch.int32, **dev))
    before = {k: v.clone() for k, v in t.items()}
    plant = _capi.Plant.default()

    def structs():
        e, m = _capi.PlantEx(), _capi.PlantMetrics()
        e.params_dev, e.force_bias_dev, e.disturbance_log_dev = t["params"].data_ptr(), t["bias"].data_ptr(), t["dlog"].data_ptr()
        e.force_sigma, e.seed, e.freeze_done = 0.5, SEED, 1
        spec = metric_spec()
        for i in range(16):
            m.Q[i] = float(spec["Q"].reshape(-1)[i])
        m.R = 0.01
        for i in range(4):
            e.meas_sigma[i], m.tol[i] = 0.01, 0.1
        m.cost_acc_dev, m.run_dev, m.best_run_dev = t["cost"].data_ptr(), t["run"].data_ptr(), t["best"].data_ptr()
        return e, m

    def call(e, m, done=True, step=1, logs=True, B=nb, bounds=(0, 0.0, 0.0), stride=1, state=True, plant_ok=True):
        return eng.lib.phnn_plant_step_ex(eng.h, C.byref(plant) if plant_ok else None, C.byref(e) if e is not None else None,
                                          C.byref(m) if m is not None else None, eng._p(t["state"]) if state else None,
                                          eng._p(t["action"]), stride, B, bounds[0], bounds[1], bounds[2], eng._p(t["x32"]),
                                          eng._p(t["done"]) if done else None, None, step, eng._p(t["logs"]) if logs else None,
                                          eng._p(t["logc"]) if logs else None, eng._stream())

    def setf(which, name, value, index=None):
        def f(e, m):
            s = e if which == "e" else m
            if index is None:
                setattr(s, name, value)
            else:
                getattr(s, name)[index] = value
        return f

    nan, inf = float("nan"), float("inf")
    bad = [("force_sigma < 0", setf("e", "force_sigma", -0.5), {}), ("force_sigma inf", setf("e", "force_sigma", inf), {}),
           ("force_sigma nan", setf("e", "force_sigma", nan), {}), ("meas_sigma < 0", setf("e", "meas_sigma", -1.0, 2), {}),
           ("meas_sigma nan", setf("e", "meas_sigma", nan, 0), {}), ("meas_sigma inf", setf("e", "meas_sigma", inf, 3), {}),
           ("plant_offset < 0", setf("e", "plant_offset", -1), {}), ("plant_offset + B > 2^48", setf("e", "plant_offset", 2 ** 48 - nb + 1), {}),
           ("freeze without done_step", None, dict(done=False)), ("disturbance log without a step", None, dict(step=-1, logs=False)),
           ("reserved", setf("e", "reserved", 1, 3), {}), ("metrics NULL cost", setf("m", "cost_acc_dev", None), {}),
           ("metrics NULL run", setf("m", "run_dev", None), {}), ("metrics NULL best", setf("m", "best_run_dev", None), {}),
           ("tol < 0", setf("m", "tol", -0.1, 1), {}), ("tol nan", setf("m", "tol", nan, 3), {}),
           # what phnn_plant_step refuses
           ("NULL plant", None, dict(plant_ok=False)), ("NULL state", None, dict(state=False)), ("B < 0", None, dict(B=-1)),
           ("stride < 0", None, dict(stride=-1)), ("u_min > u_max", None, dict(bounds=(1, 1.0, -1.0))),
           ("log without a step", None, dict(step=-1))]
    for what, change, kw in bad:
        e, m = structs()
        if change:
            change(e, m)
        assert call(e, m, **kw) == -1, what  # PHNN_ERR_INVALID_ARG
        assert eng.lib.phnn_last_error(eng.h), what
    e, m = structs()
    e.plant_offset = 2 ** 48 - nb  # the last valid offset is accepted, and B == 0 returns before any check
    torch.cuda.synchronize()
    for k, v in t.items():
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k
    assert call(e, m, B=0) == 0 and call(e, m) == 0
    torch.cuda.synchronize()
    assert not torch.equal(t["state"], before["state"]) and bool((t["dlog"][1] != 5.0).all()) and bool((t["dlog"][0] == 5.0).all())


# ----------------------------------------------------------------------------- 9. footprint
class PlantExOp(fp.Op):
    """phnn_plant_step_ex at step `step` of steps; `drop`: the optional pointers left NULL ('ex' / 'metrics': the struct)."""
    ALL = ("params", "bias", "dlog", "state_f32", "done_step", "log_states", "log_controls")

    def __init__(self, B, steps, step, rng, drop=()):
        super().__init__()
        self.name, self.B, self.T, self.step, self.drop = f"plant_ex B{B} step{step} drop={','.join(drop) or '-'}", B, steps, step, set(drop)
        self.H = 3
        st = rng.uniform(-0.4, 0.4, size=(B, 4))
        st[::5, 0] = 10.5  # terminates at this step
        done = np.full(B, -1, np.int32)
        done[::10] = 0  # terminated earlier: frozen
        f32, f64, i32 = np.float32, np.float64, np.int32
        self.add("state", f64, (B, 4), fp.INOUT, st)
        self.add("action", f32, (B, self.H), fp.IN, rng.uniform(-2.5, 2.5, size=(B, self.H)).astype(f32))
        if "ex" not in self.drop:
            if "params" not in self.drop:
                self.add("params", f64, (B, 4), fp.IN, own_params(B, B))
            if "bias" not in self.drop:
                self.add("bias", f32, (B,), fp.IN, rng.uniform(-1, 1, B).astype(f32))
            if "dlog" not in self.drop:
                self.add("dlog", f32, (steps, B), fp.INOUT, np.zeros((steps, B), f32))
        if "state_f32" not in self.drop:
            self.add("state_f32", f32, (B, 4), fp.OUT)
        if "done_step" not in self.drop:
            self.add("done_step", i32, (B,), fp.INOUT, done)
        if "log_states" not in self.drop:
            self.add("log_states", f64, (steps + 1, B, 4), fp.INOUT, np.zeros((steps + 1, B, 4)))
        if "log_controls" not in self.drop:
            self.add("log_controls", f32, (steps, B), fp.INOUT, np.zeros((steps, B), f32))
        if "metrics" not in self.drop:
            self.add("cost", f64, (B,), fp.INOUT, rng.uniform(0, 1, B))
            self.add("run", i32, (B,), fp.INOUT, rng.integers(0, 3, B).astype(i32))
            self.add("best", i32, (B,), fp.INOUT, np.full(B, 2, i32))

    def _structs(self, p):
        """p: name -> address (or missing)"""
        from phnn_mpc_amd import _capi
        e = m = None
        if "ex" not in self.drop:
            e = _capi.PlantEx()
            e.params_dev, e.force_bias_dev, e.disturbance_log_dev = p.get("params"), p.get("bias"), p.get("dlog")
            e.force_sigma, e.seed, e.plant_offset, e.freeze_done = 0.5, SEED, 7, int("done_step" not in self.drop)
            for i in range(4):
                e.meas_sigma[i] = 0.01
        if "metrics" not in self.drop:
            m = _capi.PlantMetrics()
            spec = metric_spec()
            for i in range(16):
                m.Q[i] = float(spec["Q"].reshape(-1)[i])
            m.R = 0.01
            for i in range(4):
                m.tol[i] = 0.3
            m.cost_acc_dev, m.run_dev, m.best_run_dev = p["cost"], p["run"], p["best"]
        return e, m

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        e, m = self._structs({k: v.value for k, v in p.items()})
        pl = _capi.Plant.default()
        fp.check_rc(eng, eng.lib.phnn_plant_step_ex(eng.h, C.byref(pl), C.byref(e) if e else None, C.byref(m) if m else None, p["state"],
                                                    p["action"], self.H, self.B, 1, -1.5, 2.0, p.get("state_f32"), p.get("done_step"),
                                                    None, self.step, p.get("log_states"), p.get("log_controls"), eng._stream()))

    def engine(self, eng):
        import torch
        from phnn_mpc_amd import _capi
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        if "state_f32" not in self.drop:
            t["state_f32"] = torch.empty(self.B, 4, dtype=torch.float32, device=eng.device)
        e, m = self._structs({k: v.data_ptr() for k, v in t.items()})
        eng.plant_step(_capi.Plant.default(), t["state"], t["action"], self.H, u_min=-1.5, u_max=2.0, state_f32=t.get("state_f32"),
                       done_step=t.get("done_step"), step=self.step, log_states=t.get("log_states"),
                       log_controls=t.get("log_controls"), ex=e, metrics=m)
        return {b.name: t[b.name] for b in self.outputs()}


@pytest.mark.parametrize("nb", [19, 257])
def test_footprint_of_the_extended_plant_step(torch, nb):
    from test_gpu_footprint import Report, footprint, rng_of
    eng = engine("phnn_cartpole")
    rep = Report(f"phnn_plant_step_ex B{nb}")
    for drop in [()] + [(k,) for k in PlantExOp.ALL] + [("ex",), ("metrics",)]:
        op = PlantExOp(nb, 3, 1, rng_of("plant_ex", nb), drop)
        ff = footprint(rep, torch, eng, op)
        if not drop:  # the step wrote row 1 (2 of the states) of each log and nothing else of them
            for k, row, width in (("dlog", 1, 4 * nb), ("log_controls", 1, 4 * nb), ("log_states", 2, 32 * nb)):
                got = ff[2].written(k, 0)
                assert got is not None and row * width <= got[0] and got[1] <= (row + 1) * width, (k, got)
    rep.finish()


# ----------------------------------------------------------------------------- 10. closed loop
def _load(cls, name, torch):
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights(name).items()})
    return m


def _controller(torch, which):
    from phnn_mpc_amd.models import pHNN
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(horizon=5, optimizer_steps=3)
    if which == "MPPI":
        cfg["mpc"].update(optimizer="MPPI", samples=16, lam=20.0, sigma=3.0, seed=0x1234_5678_9ABC_DEF0)
    c = create_mpc_from_config(_load(pHNN, "phnn_cartpole", torch), cfg)
    assert c.horizon == 5 and c.max_iterations == 3 and c.optimizer_type == which
    return c, cfg


@pytest.mark.parametrize("which", ["Adam", "MPPI"])
def test_closed_loop_scenarios(torch, which):
    from phnn_mpc_amd.closed_loop import BatchedCartPole, PlantScenario, run_mpc_batch, run_mpc_batch_device, stability_report
    c, cfg = _controller(torch, which)
    nb, steps = 19, 4
    rng = np.random.default_rng(10)
    X0 = rng.uniform(-1, 1, size=(nb, 4)) * [0.2, 0.08, 0.1, 0.1]
    params = PlantScenario.spread(nb, {"masscart": 0.2, "masspole": 0.2, "length": 0.2}, rng)
    stab = dict(tolerance=[0.25, 0.1, 0.3, 0.6], min_duration=0.05)
    sc = PlantScenario(params=params, force_sigma=0.5, seed=SEED)
    runs = {g: run_mpc_batch_device(c, X0, steps, use_graph=g, scenario=sc, metrics=stab) for g in (False, True)}
    eager, graphed = runs[False], runs[True]
    assert set(eager) == {"states", "controls", "done_step", "disturbance", "cost", "longest_run_s", "stable"}
    for k in eager:
        f = bits64 if eager[k].dtype == np.float64 else np.asarray
        assert np.array_equal(f(eager[k]), f(graphed[k])), k
    w = eager["disturbance"]
    assert w.shape == (steps, nb) and w.dtype == np.float32 and len(np.unique(w)) == w.size
    plain = run_mpc_batch_device(c, X0, steps)
    assert not np.array_equal(plain["states"], eager["states"]) and set(plain) == {"states", "controls", "done_step"}
    host = run_mpc_batch(BatchedCartPole(0.02, scenario=PlantScenario(params=params), replay=w), c, X0, steps)
    assert np.array_equal(bits32(eager["controls"]), bits32(host["controls"]))
    assert np.allclose(eager["states"], host["states"], rtol=0, atol=1e-12)
    assert np.array_equal(eager["done_step"], host["done_step"]) and np.array_equal(host["disturbance"], w)
    # the metrics are those of the logged run
    rep = stability_report(eager["states"], cfg["mpc"].get("x_target", [0, 0, 0, 0]), stab["tolerance"], stab["min_duration"], 0.02)
    assert np.array_equal(eager["stable"], rep["stable"]) and np.array_equal(eager["longest_run_s"], rep["longest_run_s"])
    Q = np.diag(np.asarray(cfg["mpc"]["Q_diag"], np.float32).astype(np.float64))
    spec = dict(Q=Q, R=float(np.float32(cfg["mpc"]["R_diag"][0])), target=np.zeros(4), tol=np.array(stab["tolerance"]))
    cost, _, _ = metrics_np(eager["states"], eager["controls"][:, :, 0].astype(np.float32), spec, np.ones((steps, nb), bool), np.zeros(nb))
    assert np.all(np.abs(eager["cost"] - cost) <= 1e-12 * cost) and np.all(cost > 0)
    # log=False: the same metrics, no logs
    bare = run_mpc_batch_device(c, X0, steps, scenario=sc, metrics=stab, log=False)
    assert bare["states"] is None and bare["controls"] is None and bare["disturbance"] is None
    for k in ("cost", "stable", "done_step", "longest_run_s"):
        assert np.array_equal(bare[k], eager[k]), k
    # measurement noise: eager == graphed, and the seed matters
    noisy = {}
    for seed in (SEED, SEED + 1):
        ms = PlantScenario(params=params, meas_sigma=[0.01, 0.005, 0.01, 0.01], seed=seed)
        a, b = (run_mpc_batch_device(c, X0, steps, use_graph=g, scenario=ms) for g in (False, True))
        for k in a:
            assert np.array_equal(bits64(a[k]) if a[k].dtype == np.float64 else a[k], bits64(b[k]) if b[k].dtype == np.float64 else b[k]), k
        assert not a["disturbance"].any()  # nothing is added to the force
        noisy[seed] = a
    assert not np.array_equal(noisy[SEED]["controls"][1:], noisy[SEED + 1]["controls"][1:])
    assert np.array_equal(noisy[SEED]["controls"][0], noisy[SEED + 1]["controls"][0])  # the initial state is handed over as it is
