"""k_plant_step (engine.plant_step) and the device closed loop at their edges, against the numpy plant
closed_loop.BatchedCartPole (pinned to the reference simulator's G11 run in tests/test_host_logic.py).

  constants    a phnn_plant with EVERY field away from the reference's values, and each field changed alone: 5 steps,
               B = 1 / 19 / 257 (one plant, ragged, past one 256-thread block), action_stride 1 and 7, |state| <= 1, so the
               bound of tests/test_gpu_configs.py applies: 1e-13 absolute on the float64 state (the device's
               double-precision sin / cos can differ from numpy's in the last bit), 2e-7 relative on state_f32.
  forces       beyond the bounds and +-inf: clamped, and log_controls holds the clamped value.  A NaN force under the
               bounds is NOT clamped (torch.clamp passes it on; fminf(fmaxf()) alone would apply u_min): NaN in the
               state, state_f32, log_states and log_controls exactly where the numpy plant has it, done_step stays -1; a
               NaN state never terminates; every output row of every other plant has the bits of the run without it.
  termination  strict: |x| == x_limit is not done, nextafter(x_limit) is, the same for theta (x_dot = theta_dot = 0: the
               position update is exact); done_step is written once -- a plant that re-enters the limits keeps its first
               step; a device step counter and a host step index give identical logs.
  closed loop  19 plants, plant 7 starts at a NaN state; MPCController (Adam, 3 iterations, H = 5, bounds on: the last
               iterate is NaN, and so is the force) and MPCControllerCanonical (best iterate: none is ever recorded, the
               force is 0); 4 control steps; run_mpc_batch_device, eager and graphed, == run_mpc_batch: controls bit for
               bit with NaN for NaN, done_step equal, the other plants' states within the closed-loop contract's 1e-12
               and bit-identical to the run without plant 7.
"""
import os

import numpy as np
import pytest
import yaml

import oracle_lib as ol
from test_gpu_mppi import engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
DEFAULT = dict(gravity=9.8, masscart=1.0, masspole=0.1, length=0.5, dt=0.02, x_limit=10.0, theta_limit=0.5)
OTHER = dict(gravity=9.81, masscart=1.3, masspole=0.25, length=0.7, dt=0.01, x_limit=0.7, theta_limit=0.2)
QNAN = np.uint32(0x7FC00000)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def plant_of(c):
    from phnn_mpc_amd import _capi
    return _capi.Plant(*(float(c[k]) for k in ("gravity", "masscart", "masspole", "length", "dt", "x_limit", "theta_limit")))


def bits32(a):
    """float32 array -> uint32 view, every NaN one pattern (a NaN's sign and payload are not part of the contract)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = QNAN
    return b


def bits64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = np.uint64(0x7FF8000000000000)
    return b


def run_device(torch, consts, init, forces, stride=1, bounds=None, step_dev=False, first_step=0):
    """forces (T,B) float32 -> dict(states (T,B,4), x32 (T,B,4), logs (T+1,B,4), logc (T,B), done (B)); the action tensor
    is (B, stride) with the force in column 0 and a sentinel in the others."""
    eng = engine("phnn_cartpole")
    nb, T = init.shape[0], forces.shape[0]
    plant = plant_of(consts)
    state = torch.tensor(init, dtype=torch.float64, device="cuda")
    x32 = torch.full((nb, 4), -7.0, dtype=torch.float32, device="cuda")
    done = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    logs = torch.zeros(first_step + T + 1, nb, 4, dtype=torch.float64, device="cuda")
    logc = torch.zeros(first_step + T, nb, dtype=torch.float32, device="cuda")
    sd = torch.full((1,), first_step, dtype=torch.int32, device="cuda") if step_dev else None
    kw = {} if bounds is None else dict(u_min=bounds[0], u_max=bounds[1])
    states, x32s = [], []
    for t in range(T):
        a = torch.full((nb, stride), 1e30, dtype=torch.float32, device="cuda")
        a[:, 0] = torch.tensor(forces[t], device="cuda")
        eng.plant_step(plant, state, a, stride, state_f32=x32, done_step=done, step=-5 if step_dev else first_step + t,
                       step_dev=sd, log_states=logs, log_controls=logc, **kw)
        if step_dev:
            eng.advance_step(sd)
        states.append(state.cpu().numpy().copy())
        x32s.append(x32.cpu().numpy().copy())
    return dict(states=np.stack(states), x32=np.stack(x32s), logs=logs.cpu().numpy()[first_step:], logc=logc.cpu().numpy()[first_step:],
                done=done.cpu().numpy())


def run_host(consts, init, forces, first_step=0):
    """The numpy plant on float64 forces (T,B) -> dict(states (T,B,4), done (B), flags (T,B))."""
    from phnn_mpc_amd.closed_loop import BatchedCartPole
    sim = BatchedCartPole(**consts)
    sim.reset(init)
    states, flags = [], []
    done = np.full(init.shape[0], -1)
    with np.errstate(invalid="ignore"):
        for t in range(forces.shape[0]):
            hs, hd = sim.step(np.asarray(forces[t], np.float64))
            done[(done < 0) & hd] = first_step + t
            states.append(hs)
            flags.append(hd)
    return dict(states=np.stack(states), done=done, flags=np.stack(flags))


def against_host(dev, host, forces_applied):
    """The stated bounds, NaN for NaN."""
    assert np.array_equal(np.isnan(dev["states"]), np.isnan(host["states"]))
    assert np.allclose(dev["states"], host["states"], rtol=0, atol=1e-13, equal_nan=True)
    with np.errstate(invalid="ignore"):
        h32 = host["states"].astype(np.float32).astype(np.float64)
    assert np.allclose(dev["x32"].astype(np.float64), h32, rtol=2e-7, atol=1e-30, equal_nan=True)
    assert np.array_equal(np.isnan(dev["x32"]), np.isnan(host["states"]))
    assert np.array_equal(bits64(dev["logs"][1:]), bits64(dev["states"]))  # the log holds the state the step left
    assert np.array_equal(bits32(dev["x32"]), bits32(dev["states"].astype(np.float32)))  # state_f32 = float32(state)
    assert np.array_equal(bits32(dev["logc"]), bits32(forces_applied))
    assert np.array_equal(dev["done"], host["done"])


def inputs(nb, T, seed, f_lim=5.0):
    rng = np.random.default_rng(seed)
    init = rng.uniform(-1, 1, size=(nb, 4)) * [0.8, 0.25, 0.5, 0.5]
    return init, rng.uniform(-f_lim, f_lim, size=(T, nb)).astype(np.float32)


# ----------------------------------------------------------------------------- constants
@pytest.mark.parametrize("stride", [1, 7])
@pytest.mark.parametrize("nb", [1, 19, 257])
def test_non_default_plant_against_the_numpy_plant(torch, nb, stride):
    init, forces = inputs(nb, 5, nb)
    variants = [OTHER]
    if nb == 19 and stride == 1:  # every field alone, so that none can hide behind another
        variants += [dict(DEFAULT, **{k: OTHER[k]}) for k in OTHER]
    base = run_host(DEFAULT, init, forces)
    for consts in variants:
        dev, host = run_device(torch, consts, init, forces, stride), run_host(consts, init, forces)
        assert np.abs(host["states"]).max() <= 1.0  # the range the 1e-13 bound is stated for
        against_host(dev, host, forces)
        moved = not np.array_equal(host["states"], base["states"]) or not np.array_equal(host["done"], base["done"])
        assert moved, consts  # the field matters on these inputs
        if nb >= 19 and (consts["x_limit"] < 10 or consts["theta_limit"] < 0.5):  # some plants terminate, some do not
            assert (host["done"] >= 0).any() and (host["done"] < 0).any()


# ----------------------------------------------------------------------------- forces
BOUNDS = (-15.0, 15.0)


def test_forces_past_the_bounds_are_clamped_and_a_nan_force_stays_nan(torch):
    nb, T = 19, 4
    init, forces = inputs(nb, T, 3, f_lim=25.0)  # about 40 % of the forces past +-15
    forces[:, 3], forces[:, 4], forces[0, 5], forces[1, 5] = np.inf, -np.inf, 15.0, -15.0
    init[9] = [np.nan, 0.1, 0.0, 0.0]  # a NaN state: never done
    clean = forces.copy()
    clean[:, [7, 12]] = 0.0
    dirty = clean.copy()
    dirty[1:, 7] = np.nan  # goes NaN in mid-run
    dirty[0, 12] = np.nan  # one NaN command: the state keeps it
    applied = {k: torch.clamp(torch.tensor(f), *BOUNDS).numpy() for k, f in (("clean", clean), ("dirty", dirty))}
    assert np.array_equal(np.isnan(applied["dirty"]), np.isnan(dirty)) and (np.abs(clean) > 15).any()
    assert np.array_equal(applied["clean"], np.clip(clean, *BOUNDS)) and np.abs(applied["clean"]).max() == 15.0
    out = {}
    for k, f in (("clean", clean), ("dirty", dirty)):
        out[k] = run_device(torch, DEFAULT, init, f, stride=3, bounds=BOUNDS)
        against_host(out[k], run_host(DEFAULT, init, applied[k]), applied[k])
    d, c = out["dirty"], out["clean"]
    keep = np.ones(nb, bool)
    keep[[7, 12]] = False
    for name in ("states", "logs"):
        assert np.array_equal(bits64(d[name][:, keep]), bits64(c[name][:, keep])), name
    for name in ("x32", "logc"):
        assert np.array_equal(bits32(d[name][:, keep]), bits32(c[name][:, keep])), name
    assert np.array_equal(d["done"][keep], c["done"][keep])
    assert np.isfinite(c["states"][:, np.arange(nb) != 9]).all() and np.isfinite(c["logc"]).all()
    # the NaN plants: velocities at once, positions one step later, the log says NaN, nothing terminates
    assert np.isnan(d["states"][1, 7, 2:]).all() and np.isfinite(d["states"][1, 7, :2]).all() and np.isnan(d["states"][2:, 7]).all()
    assert np.isfinite(d["states"][0, 7]).all() and np.isnan(d["states"][1:, 12]).all()
    assert np.array_equal(np.isnan(d["logc"]), np.isnan(dirty)) and np.isnan(d["logs"][3:, 7]).all()
    assert np.isnan(d["x32"][2:, 7]).all()
    assert d["done"][7] == d["done"][12] == d["done"][9] == -1 and np.isnan(d["states"][:, 9, 0]).all()


# ----------------------------------------------------------------------------- termination
@pytest.mark.parametrize("consts", [DEFAULT, OTHER], ids=["default", "other"])
def test_termination_is_strict(torch, consts):
    xl, tl = consts["x_limit"], consts["theta_limit"]
    up = lambda v: float(np.nextafter(v, np.inf))
    init = np.array([[xl, 0, 0, 0], [up(xl), 0, 0, 0], [-xl, 0, 0, 0], [-up(xl), 0, 0, 0],
                     [0, tl, 0, 0], [0, up(tl), 0, 0], [0, -tl, 0, 0], [0, -up(tl), 0, 0], [0, 0, 0, 0]], np.float64)
    forces = np.zeros((1, len(init)), np.float32)
    dev = run_device(torch, consts, init, forces, first_step=5)
    assert np.array_equal(dev["states"][0, :, :2], init[:, :2])  # x + dt * 0: the positions are exact
    assert dev["done"].tolist() == [-1, 5, -1, 5, -1, 5, -1, 5, -1]
    assert np.array_equal(dev["done"], run_host(consts, init, forces, first_step=5)["done"])


def test_done_step_is_written_once_and_both_step_sources_agree(torch):
    consts = dict(DEFAULT, x_limit=1.0)
    init = np.array([[0.99, 0, 1.0, 0], [0.95, 0, 1.0, 0], [0.0, 0, 0.1, 0]], np.float64)
    forces = np.zeros((5, 3), np.float32)
    forces[0, 0] = -100.0  # plant 0 leaves at step 0 and is pushed back inside at step 1
    host = run_host(consts, init, forces, first_step=2)
    assert host["flags"][:, 0].tolist() == [True, False, False, False, False]
    assert host["flags"][:, 1].tolist() == [False, False, True, True, True] and not host["flags"][:, 2].any()
    dev = run_device(torch, consts, init, forces, first_step=2)
    against_host(dev, host, forces)
    assert dev["done"].tolist() == [2, 4, -1]
    cnt = run_device(torch, consts, init, forces, first_step=2, step_dev=True)  # the step index read from the device
    for k in ("states", "logs"):
        assert np.array_equal(bits64(cnt[k]), bits64(dev[k])), k
    for k in ("x32", "logc"):
        assert np.array_equal(bits32(cnt[k]), bits32(dev[k])), k
    assert np.array_equal(cnt["done"], dev["done"])


# ----------------------------------------------------------------------------- closed loop
def _load(cls, name, torch):
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights(name).items()})
    return m


@pytest.mark.parametrize("which", ["MPCController", "MPCControllerCanonical"])
def test_closed_loop_with_a_nan_plant(torch, which):
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(horizon=5, optimizer_steps=3)
    if which == "MPCController":
        c = create_mpc_from_config(_load(pHNN, "phnn_cartpole", torch), cfg)
        assert c.horizon == 5 and c.max_iterations == 3 and c.optimizer_type == "Adam" and (c.u_min, c.u_max) == (-15.0, 15.0)
    else:
        c = create_mpc_controller(_load(pHNN_Canonical, "canonical_cartpole", torch), cfg)
        assert c.horizon == 5 and c.optimizer_steps == 3 and c.optimizer == "Adam" and (c.u_min, c.u_max) == (-15.0, 15.0)
    nb, bad, T = 19, 7, 4
    rng = np.random.default_rng(6)
    X0 = rng.uniform(-1, 1, size=(nb, 4)) * [0.2, 0.08, 0.1, 0.1]
    Xn = X0.copy()
    Xn[bad, 2] = np.nan
    keep = np.arange(nb) != bad
    with np.errstate(invalid="ignore"):
        host = run_mpc_batch(BatchedCartPole(0.02), c, Xn, T)
    # the diverged plant shows: the last Adam iterate is NaN and so is the force; the canonical controller never records a
    # best iterate and applies its initial best_u, 0
    if which == "MPCController":
        assert np.isnan(host["controls"][:, bad]).all()
    else:
        assert (host["controls"][:, bad] == 0).all()
    assert np.isfinite(host["controls"][:, keep]).all() and np.isnan(host["states"][1:, bad, 2]).all()
    for use_graph in (False, True):
        dev = run_mpc_batch_device(c, Xn, T, use_graph=use_graph)
        clean = run_mpc_batch_device(c, X0, T, use_graph=use_graph)
        assert dev["controls"].shape == host["controls"].shape and dev["states"].shape == host["states"].shape
        assert np.array_equal(bits32(dev["controls"]), bits32(host["controls"])), use_graph
        assert np.array_equal(dev["done_step"], host["done_step"]) and dev["done_step"][bad] == -1
        assert np.allclose(dev["states"][:, keep], host["states"][:, keep], rtol=0, atol=1e-12)
        assert np.array_equal(np.isnan(dev["states"]), np.isnan(host["states"]))
        assert np.array_equal(bits64(dev["states"][:, keep]), bits64(clean["states"][:, keep]))
        assert np.array_equal(bits32(dev["controls"][:, keep]), bits32(clean["controls"][:, keep]))
        assert np.array_equal(dev["done_step"][keep], clean["done_step"][keep])
