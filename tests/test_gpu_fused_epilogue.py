"""The per-pair epilogues of the f16x2 hidden x hidden products (the element-wise passes of tile
pair P ride under the MFMAs of pair P + 1 in the whole-tile march kernels K1 and K2).

The fusion moves instructions, never operands or roundings, so two things pin it:

  1. the split-tile kernels, which keep the monolithic products and every summation order of the whole-tile ones, must
     agree with the whole-tile kernels BITWISE on cost, trajectory and grad_u -- at a lone rollout, at one full 16-rollout
     tile plus a ragged one, and at more tiles than a workgroup has waves; one step (only the epilogue behind the stream
     of the last pair matters as much as the others) and three; Euler and RK4; stash mode;
  2. the canonical cart-pole model (its forward march is fused, its adjoint is not: no registers to spare) and the
     cart-pole pHNN whose hidden widths are not 128 (zero-padded to the 128-wide kernels: whole tiles and tile pairs of
     zeros pass through the epilogues) must sit within the stated float32 tolerances of tests/test_gpu_parity.py against
     the float64 oracle.  (The 64-wide f16x2 kernels keep the monolithic order: no fused instantiation to test.)

Which launches are fused: the epilogues are compiled into the Euler march with the MPC tape only -- K1 as launched by
rollout_cost_grad with a stash (it writes the workspace's cost and trajectory and the tape) and the K2 that reads that
tape.  So cost, trajectory and grad_u are all taken from ONE rollout_cost_grad call with a workspace dict, and the test
asserts that the stash exists.  The RK4 cases and the forward-only rollout_cost call (K1 without a tape) run kernels
that keep the monolithic order: they are controls, and the forward-only trajectory of the same engine must equal the
fused K1's bit for bit as well.

A build with PHNN_NO_FUSED_EPILOGUE runs the same kernels in the monolithic order and passes unchanged.
"""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

DT = 0.02


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _march(eng, x0, U, cost, integ, dt):
    """cost, trajectory, grad_u of one K1 (MPC tape) + K2 (from that tape) pair: the launches the epilogues are in."""
    ws = {}
    c, gu = eng.rollout_cost_grad(x0, U, cost, integ, dt, workspace=ws)
    assert eng.use_stash and ws["stash"] is not None, "K1 must keep the tape: without it both kernels are other instantiations"
    assert c is ws["cost"]
    return c.clone(), ws["traj"].clone(), gu.clone()


def _is_whole_tile_f16x2(eng, B):
    """The fused path is what the whole-tile f16x2 kernels compile to: pin the variant and the kernel family.  A handle
    that may never use the split-tile kernels (split_tiles = 1) puts one wave on a tile at every batch size: as many
    workgroups as tiles / waves, and at a large batch eight tiles per workgroup where the split-tile kernels have one."""
    small, large = eng.kernel_info(B), eng.kernel_info(1 << 16)
    tiles = (B + 15) // 16
    waves = small["rollouts_per_workgroup"] // 16
    return ("f16x2" in eng.variant and eng.matmul_mode == "f16x2" and eng.options.split_tiles == 1
            and large["rollouts_per_workgroup"] > 16 and small["workgroups"] == (tiles + waves - 1) // waves)


@pytest.fixture(scope="module")
def engines(torch):
    from phnn_mpc_amd.engine import RolloutEngine
    w = ol.load_weights("phnn_cartpole")
    whole, split = RolloutEngine(w, split="never"), RolloutEngine(w, split="always")
    whole.use_stash = split.use_stash = True
    assert "hid=128" in whole.variant and "fixedG" in whole.variant, whole.variant
    return whole, split, ol.cost_from_golden(ol.load_golden("phnn_cartpole"))


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("B", [1, 17, 130])
def test_whole_tile_bitwise_equal_split_tile(torch, engines, B, H, integ):
    whole, split, cost = engines
    assert _is_whole_tile_f16x2(whole, B), (whole.variant, whole.kernel_info(B))
    assert split.kernel_info(B)["rollouts_per_workgroup"] == 16
    rng = np.random.default_rng(1000 * B + 10 * H + (integ == "rk4"))
    x0 = (rng.uniform(-1, 1, size=(B, 4)) * [1.0, 0.3, 0.5, 0.5]).astype(np.float32)
    U = rng.uniform(-17, 17, size=(B, H, 1)).astype(np.float32)
    res = [_march(eng, x0, U, cost, integ, DT) for eng in (whole, split)]
    for a, b, what in zip(res[0], res[1], ("cost", "traj", "grad_u")):
        assert torch.isfinite(a).all(), what
        assert torch.equal(a, b), (B, H, integ, what, float((a - b).abs().max()))
    # control: the forward-only K1 of the same engine (no tape: monolithic order) computes the same cost and trajectory
    c2, traj2 = whole.rollout_cost(x0, U, cost, integ, DT, want_traj=True)
    assert torch.equal(c2, res[0][0]) and torch.equal(traj2, res[0][1]), (B, H, integ, "forward-only control")


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("name", ["canonical_cartpole", "phnn_cartpole_odd"])
def test_fused_models_vs_oracle(torch, name, integ):
    from phnn_mpc_amd.engine import RolloutEngine
    w, g = ol.load_weights(name), ol.load_golden(name)
    eng = RolloutEngine(w, split="never", matmul="f16x2", force_matmul=True)
    eng.use_stash = True
    B, H = 17, 3
    assert _is_whole_tile_f16x2(eng, B), (eng.variant, eng.kernel_info(B))
    assert "hid=128" in eng.variant, eng.variant  # the widths that run the per-pair epilogues
    n = eng.n
    rng = np.random.default_rng(77)
    x0 = (rng.uniform(-1, 1, size=(B, n)) * np.array([1.0, 0.3, 0.5, 0.5][:n])).astype(np.float32)
    amp = 1.3 * float(g["u_max"])
    U = rng.uniform(-amp, amp, size=(B, H, 1)).astype(np.float32)
    cost = ol.cost_from_golden(g)
    dt = float(g["dt"])
    ref = ol.OracleModel(w, "f64").rollout(x0, U, cost, integ, dt)
    c, traj, gu = (npy(t) for t in _march(eng, x0, U, cost, integ, dt))
    traj_atol = 1e-5  # tests/test_gpu_parity.py: TRAJ_ATOL of both models
    gmax = np.abs(ref["grad_u"]).max(axis=(1, 2), keepdims=True)
    print(name, integ, "cost rel", np.abs(c / ref["cost"] - 1).max(), "traj abs", np.abs(traj - ref["traj"]).max(),
          "grad/max", (np.abs(gu - ref["grad_u"]) / np.maximum(gmax, 1e-300)).max())
    assert np.allclose(c, ref["cost"], rtol=1e-5, atol=0), np.abs(c / ref["cost"] - 1).max()
    assert np.allclose(traj, ref["traj"], rtol=1e-5, atol=traj_atol), np.abs(traj - ref["traj"]).max()
    assert np.all(np.abs(gu - ref["grad_u"]) <= 1e-4 * gmax), (np.abs(gu - ref["grad_u"]) / gmax).max()
