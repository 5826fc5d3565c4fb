"""Plant scenarios on the host (closed_loop.PlantScenario, the numpy plant BatchedCartPole, noise.plant_normals): CPU only.

  default      a default PlantScenario on the numpy plant gives the bits of the plain plant, and so does a scenario whose
               per-plant parameters are the shared constants
  generator    the package's float64 generator == tests/mppi_model.normals bit for bit at the contract's counters: the
               force normal is element 0 and the measurement normals are elements 4..7 of sample 1 of problem gid at
               (seed, epoch = step, iteration = 0)
  replay       replay= of a drawn run's disturbance reproduces it bit for bit; the noise of a plant does not depend on the
               batch it is drawn in (plant_offset); freeze keeps a terminated plant's state
  spread       stays inside its bounds, column by column
  surface      the header declares phnn_plant_step_ex, EXPORTED lists it, the two structs match the header
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mppi_model as mm
from phnn_mpc_amd import _capi, noise
from phnn_mpc_amd.closed_loop import PARAMS, PLANT_DEFAULTS, BatchedCartPole, PlantScenario

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xC0FFEE_1234_5678


def _run(sim, init, forces):
    sim.reset(init)
    states, meas, dist = [], [], []
    for f in forces:
        s, _ = sim.step(f)
        states.append(s)
        meas.append(sim.measurement())
        dist.append(None if sim.disturbance is None else sim.disturbance.copy())
    return np.stack(states), np.stack(meas), dist


def _inputs(nb, T, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, size=(nb, 4)) * [0.8, 0.25, 0.5, 0.5], rng.uniform(-5, 5, size=(T, nb)).astype(np.float32)


def test_default_scenario_is_the_plain_plant_bit_for_bit():
    init, forces = _inputs(19, 6, 0)
    forces[0, 3] = -0.0
    init[3] = 0.0
    plain, pm, pd = _run(BatchedCartPole(0.02), init, forces)
    assert all(d is None for d in pd)
    shared = {k: np.full(19, PLANT_DEFAULTS[k]) for k in PARAMS}
    for sc in (PlantScenario(), PlantScenario(params=shared), PlantScenario(params={"length": 0.5}),
               PlantScenario(params=np.tile([9.8, 1.0, 0.1, 0.5], (19, 1)))):
        s, m, d = _run(BatchedCartPole(0.02, scenario=sc), init, forces)
        assert np.array_equal(s.view(np.uint64), plain.view(np.uint64))
        assert np.array_equal(m.view(np.uint32), pm.view(np.uint32)) and all(x is None for x in d)
    assert np.array_equal(pm.view(np.uint32), plain.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("step", [0, 3, -1, 2 ** 31 - 1])
def test_generator_equals_the_sampler_model_at_the_contract_counters(step):
    gids = np.array([0, 1, 18, 256, (1 << 32) + 5, (1 << 48) - 1])
    z = mm.normals(SEED, step, 0, gids, 2, 8)  # (gid, K = 2, N = 8), float64
    assert np.array_equal(noise.plant_normals(SEED, step, gids, 0).view(np.uint64), z[:, 1, :4].view(np.uint64))
    assert np.array_equal(noise.plant_normals(SEED, step, gids, 1).view(np.uint64), z[:, 1, 4:].view(np.uint64))
    other = noise.plant_normals(SEED + 1, step, gids, 0)
    assert not np.any(other == z[:, 1, :4])


def test_replay_reproduces_a_drawn_run_and_noise_follows_the_global_id():
    nb, T = 19, 6
    init, forces = _inputs(nb, T, 1)
    rng = np.random.default_rng(2)
    kw = dict(params=PlantScenario.spread(nb, 0.2, rng), force_bias=rng.uniform(-1, 1, nb), force_sigma=0.5,
              meas_sigma=[0.01, 0.0, 0.02, 0.0], seed=SEED)
    s, m, d = _run(BatchedCartPole(0.02, scenario=PlantScenario(**kw)), init, forces)
    d = np.stack(d)
    assert d.dtype == np.float32 and d.shape == (T, nb)
    z0 = np.stack([noise.plant_normals(SEED, t, np.arange(nb), 0)[:, 0] for t in range(T)]).astype(np.float32)
    assert np.array_equal(d, kw["force_bias"].astype(np.float32) + np.float32(0.5) * z0)
    assert np.array_equal(m[:, :, [1, 3]], s.astype(np.float32)[:, :, [1, 3]])  # sigma 0: exactly float32(x)
    assert not np.any(m[:, :, [0, 2]] == s.astype(np.float32)[:, :, [0, 2]])
    quiet = PlantScenario(params=kw["params"], meas_sigma=kw["meas_sigma"], seed=SEED)  # no bias, no force noise of its own
    s2, m2, d2 = _run(BatchedCartPole(0.02, scenario=quiet, replay=d), init, forces)
    assert np.array_equal(s2.view(np.uint64), s.view(np.uint64)) and np.array_equal(m2.view(np.uint32), m.view(np.uint32))
    assert np.array_equal(np.stack(d2), d)
    # plants 7.. alone, with plant_offset 7: the same run
    sub = PlantScenario(**dict(kw, params=kw["params"][7:], force_bias=kw["force_bias"][7:], plant_offset=7))
    s3, m3, d3 = _run(BatchedCartPole(0.02, scenario=sub), init[7:], forces[:, 7:])
    assert np.array_equal(s3.view(np.uint64), s[:, 7:].view(np.uint64)) and np.array_equal(m3.view(np.uint32), m[:, 7:].view(np.uint32))
    other, _, _ = _run(BatchedCartPole(0.02, scenario=PlantScenario(**dict(kw, seed=SEED + 1))), init, forces)
    assert not np.array_equal(other, s)


def test_freeze_keeps_a_terminated_plant():
    nb, T = 19, 6
    init, forces = _inputs(nb, T, 3)
    free, _, _ = _run(BatchedCartPole(0.02, x_limit=0.5, theta_limit=0.15), init, forces)
    s, _, _ = _run(BatchedCartPole(0.02, x_limit=0.5, theta_limit=0.15, scenario=PlantScenario(freeze_done=True)), init, forces)
    out = (np.abs(free[:, :, 0]) > 0.5) | (np.abs(free[:, :, 1]) > 0.15)
    first = np.where(out.any(axis=0), out.argmax(axis=0), T)
    assert (first < T - 1).any() and (first == T).any()
    for b in range(nb):
        f = first[b]
        assert np.array_equal(s[:f + 1, b], free[:f + 1, b])
        assert np.array_equal(s[f:, b], np.broadcast_to(s[min(f, T - 1), b], s[f:, b].shape))


def test_spread_stays_inside_its_bounds():
    rng = np.random.default_rng(4)
    base = np.array([PLANT_DEFAULTS[k] for k in PARAMS])
    p = PlantScenario.spread(4096, 0.2, rng)
    assert p.shape == (4096, 4) and p.dtype == np.float64
    assert np.all(p >= base * 0.8) and np.all(p <= base * 1.2)
    assert np.all(p.min(axis=0) < base * 0.81) and np.all(p.max(axis=0) > base * 1.19)  # and fills them
    q = PlantScenario.spread(257, {"masscart": 0.2, "masspole": 0.1, "length": 0.3}, rng)
    assert np.all(q[:, 0] == 9.8)  # no spread asked for
    for col, rel in ((1, 0.2), (2, 0.1), (3, 0.3)):
        assert np.all(q[:, col] >= base[col] * (1 - rel)) and np.all(q[:, col] <= base[col] * (1 + rel)) and np.ptp(q[:, col]) > 0
    with pytest.raises(ValueError):
        PlantScenario.spread(4, 1.0, rng)
    with pytest.raises(ValueError):
        PlantScenario.spread(4, {"mass": 0.1}, rng)
    with pytest.raises(ValueError):
        PlantScenario(force_sigma=-1.0)
    with pytest.raises(ValueError):
        PlantScenario(meas_sigma=[0.0, np.inf, 0.0, 0.0])


def test_header_declares_the_entry_point_and_the_structs_match():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    assert "phnn_plant_step_ex" in _capi.EXPORTED and re.search(r"\bint phnn_plant_step_ex\(", header)
    for name, cls in (("phnn_plant_ex", _capi.PlantEx), ("phnn_plant_metrics", _capi.PlantMetrics)):
        body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} %s;" % name, header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f for decl in body.split(";") for f in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
        assert fields == [f for f, _ in cls._fields_], (name, fields)
    e, m = _capi.PlantEx, _capi.PlantMetrics
    # 2 pointers, float, float[4] (+4 padding), uint64, int64, int32 (+4 padding), pointer, int32[4]
    assert C.sizeof(e) == 88
    assert (e.force_sigma.offset, e.meas_sigma.offset, e.seed.offset, e.plant_offset.offset, e.freeze_done.offset,
            e.disturbance_log_dev.offset, e.reserved.offset) == (16, 20, 40, 48, 56, 64, 72)
    assert C.sizeof(m) == 8 * 25 + 24 and (m.R.offset, m.target.offset, m.tol.offset, m.cost_acc_dev.offset) == (128, 136, 168, 200)
    z = _capi.PlantEx()
    assert not any(bytes(z))  # a default-constructed struct is the zero-initialised one
