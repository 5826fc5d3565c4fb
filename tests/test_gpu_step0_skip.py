"""K2 leaves out the dynamics VJP of step 0 when nobody reads lambda_0 (grad_march): fixed-G pHNN,
Euler, grad_x0 and the trajectory cotangent not given.  Step 0 then forms grad_u[:, 0] from G^T (dt lambda_1 + dx_bar_0),
the R term and the bound mask alone -- the FMAs of the full VJP's control cotangent, so the result is the same bits.
(One wave-uniform branch on t == 0 inside the time-step loop.)

Pinned here, every K2 through the C entry points on guarded buffers (tests/footprint.py: 64 KiB of guard around every
input, output and workspace, the stash of exactly the reported size):
  S1  grad_u with grad_x0 = NULL is bit for bit grad_u with grad_x0 given (the march that runs step 0 in full);
  S2  no guard byte and no input byte changes in either call: nothing is written at or beyond the ends of grad_u;
  S3  grad_x0, where given, and grad_u match the float64 oracle at the gradient tolerance of tests/test_gpu_parity.py
      (1e-4 of the largest entry of the rollout; variant_census.grad_tol).
Cases: H in {1, 2, 3} (H = 1: the loop's only step is the one left out), B in {16, 17, 33} (one whole tile, a ragged
second, a ragged third), stash and recompute, whole-tile and split-tile kernels; a control of step 0 beyond the bound
(gradient exactly 0), one exactly on it (passes); a NaN control at step 0 without bounds (stays NaN); the learned-G pHNN
and ODEFunc, whose control cotangent comes out of the state path and whose kernels run step 0 as before.  A dX cotangent
(dx_bar) reaches K2 only through phnn_rollout_wgrad, whose record-writing march always runs step 0 (the records of step 0
are read): the case is pinned there, grad_x0 given against NULL.
"""
import numpy as np
import pytest

import footprint as fp
import oracle_lib as ol
import variant_census as vc

pytestmark = pytest.mark.gpu

FIXED = "phnn<n=4,hid=128,fixedG,f16x2>"
OTHERS = ["phnn<n=2,hid=64,Gnet>", "odefunc<n=3,hid=128,f16x2>"]
BATCHES, HORIZONS = (16, 17, 33), (1, 2, 3)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


_cache = {}


def setup(sid, split="auto"):
    """Engine, float64 oracle and spec of one census variant."""
    if (sid, split) not in _cache:
        from phnn_mpc_amd.engine import RolloutEngine
        s = vc.CENSUS[sid]
        sd = vc.build_state_dict(sid, s)
        eng = RolloutEngine(sd, "cuda:0", split=split, **vc.engine_kwargs(s))
        assert eng.variant == sid
        if "m64" not in _cache.setdefault(sid, {}):
            _cache[sid]["m64"] = ol.OracleModel(sd, "f64", activation=s["act"])
        _cache[(sid, split)] = (eng, _cache[sid]["m64"], s)
    return _cache[(sid, split)]


def batch(sid, s, B, H, unbounded=False):
    """Seeded states, controls and cost of one shape (shared by every kernel that runs it).  Step 0: rollout 0 beyond
    U_MAX, rollout 1 exactly on it, rollout 2 below U_MIN; unbounded: a cost without bounds and a NaN at step 0 of the
    last rollout."""
    key = (sid, "batch", B, H, unbounded)
    if key not in _cache:
        rng = np.random.default_rng(vc.seed_of(sid, s) + 1000 * B + H)
        cost = vc.cost_of(s, rng)
        x0, U = (0.5 * vc.states(rng, s["n"], B)).astype(np.float32), vc.controls(rng, B, H, s["m"])
        U[0, 0, :], U[1, 0, :], U[2, 0, :] = vc.U_MAX + 1.0, vc.U_MAX, vc.U_MIN - 0.5
        if unbounded:
            cost.has_u_bounds = 0
            U[B - 1, 0, 0] = np.nan
        _cache[key] = (x0, U, cost)
    return _cache[key]


def oracle(sid, m64, s, B, H):
    key = (sid, "ref", B, H)
    if key not in _cache:
        x0, U, cost = batch(sid, s, B, H)
        _cache[key] = m64.rollout(x0, U, cost, "euler", vc.dt_of(s), nthreads=8)
    return _cache[key]


def f32(torch, t, shape):
    return t.view(torch.float32).view(*shape).cpu().numpy()


def both_marches(torch, eng, cost, x0, U, dt, stash):
    """K1 + K2 on guarded buffers with grad_x0 given and with NULL -> (guard hits, grad_u with, grad_u without, grad_x0)."""
    B, H, m = U.shape
    runs = []
    for optional in (True, False):
        op = fp.RollOp(eng, cost, x0, U, 0, dt, kind="grad", stash=stash, optional=optional)
        hits, outs, _ = fp.run(torch, eng, op, 0xFF)
        runs.append((hits, outs))
    (h1, o1), (h0, o0) = runs
    assert fp.same_bytes(torch, o1["cost"], o0["cost"]) and fp.same_bytes(torch, o1["traj"], o0["traj"])
    return h1 + h0, o1["grad_u"], o0["grad_u"], f32(torch, o1["grad_x0"], (B, x0.shape[1]))


def check_shapes(torch, sid, split):
    eng, m64, s = setup(sid, split)
    dt, bad = vc.dt_of(s), []
    for B in BATCHES:
        for H in HORIZONS:
            x0, U, cost = batch(sid, s, B, H)
            ref = oracle(sid, m64, s, B, H)
            for stash in (True, False):
                hits, gu1, gu0, gx = both_marches(torch, eng, cost, x0, U, dt, stash)
                gu = f32(torch, gu0, U.shape)
                e_u, e_x = vc.err_rows(gu, ref["grad_u"]) / vc.grad_tol(s), vc.err_rows(gx, ref["grad_x0"]) / vc.grad_tol(s)
                same = fp.same_bytes(torch, gu1, gu0)
                mask = bool((gu[0, 0] == 0).all() and (gu[2, 0] == 0).all() and (gu[1, 0] != 0).all())
                print(f"{sid} split={split} B={B} H={H} stash={stash}: S1 {same}, guard hits {hits}, mask {mask}, "
                      f"error / tolerance grad_u {e_u:.3f} grad_x0 {e_x:.3f}")
                if not (same and not hits and mask and e_u <= 1.0 and e_x <= 1.0 and np.isfinite(gu).all()):
                    bad.append((B, H, stash, same, hits, mask, e_u, e_x))
    assert not bad, bad


@pytest.mark.parametrize("split", ["never", "always"])
def test_fixed_G_grad_u_is_the_full_march_bit_for_bit(torch, split):
    """S1-S3 for the model whose K2 leaves step 0 out, whole-tile and split-tile kernels."""
    check_shapes(torch, FIXED, split)


@pytest.mark.parametrize("sid", OTHERS)
def test_learned_G_and_odefunc_are_unchanged(torch, sid):
    """S1-S3 for the models whose control cotangent goes through the state path: both calls run step 0 in full."""
    check_shapes(torch, sid, "auto")


@pytest.mark.parametrize("split", ["never", "always"])
def test_nan_control_at_step_0_stays_nan(torch, split):
    """Without bounds a NaN control of step 0 reaches grad_u[:, 0] of its rollout as NaN in both marches (same bits), and
    no other rollout; the other rollouts match the float64 oracle."""
    eng, m64, s = setup(FIXED, split)
    for H in (1, 3):
        B = 17
        x0, U, cost = batch(FIXED, s, B, H, unbounded=True)
        keep = np.arange(B) != B - 1
        ref = m64.rollout(x0[keep], U[keep], cost, "euler", vc.dt_of(s), nthreads=8)
        for stash in (True, False):
            hits, gu1, gu0, gx = both_marches(torch, eng, cost, x0, U, vc.dt_of(s), stash)
            gu = f32(torch, gu0, U.shape)
            assert not hits and fp.same_bytes(torch, gu1, gu0), (H, stash, hits)
            assert np.isnan(gu[B - 1, 0]).all() and np.isfinite(gu[keep]).all() and np.isfinite(gx[keep]).all()
            assert vc.err_rows(gu[keep], ref["grad_u"]) <= vc.grad_tol(s) and vc.err_rows(gx[keep], ref["grad_x0"]) <= vc.grad_tol(s)


def test_dx_bar_cotangent_with_and_without_grad_x0(torch):
    """The dX cotangent enters through phnn_rollout_wgrad (record-writing march: step 0 always runs).  grad_u with
    grad_x0 = NULL is grad_u with it given, bit for bit, and both differ from the run without dx_bar at step 0."""
    eng, _, s = setup(FIXED, "never")
    n, m = s["n"], s["m"]
    for B, H in ((17, 1), (33, 3)):
        x0, U, _ = batch(FIXED, s, B, H)
        rng = np.random.default_rng(B * 100 + H)
        dxb = rng.normal(size=(B, H, n)).astype(np.float32)
        traj = eng.rollout_trajectory(x0, U, "euler", vc.dt_of(s))
        x0d, Ud, dbd = (torch.tensor(a, device="cuda") for a in (x0, U, dxb))
        ws = eng._wgrad_workspace(B, H, 0)
        out = {}
        for tag, db, want_x0 in (("with", dbd, True), ("without", dbd, False), ("no_dx_bar", None, True)):
            gt = torch.empty(eng.blob.size, dtype=torch.float32, device="cuda")
            gu = torch.full((B, H, m), float("nan"), dtype=torch.float32, device="cuda")
            gx = torch.empty(B, n, dtype=torch.float32, device="cuda") if want_x0 else None
            fp.check_rc(eng, eng.lib.phnn_rollout_wgrad(eng.h, eng._p(x0d), eng._p(Ud), B, H, 0, float(vc.dt_of(s)), eng._p(traj),
                                                        None, eng._p(db), eng._p(ws), eng._p(gt), 0, eng._p(gu), eng._p(gx),
                                                        eng._stream()))
            torch.cuda.synchronize()
            out[tag] = gu.cpu().numpy()
        assert np.isfinite(out["with"]).all()
        assert out["with"].tobytes() == out["without"].tobytes()
        assert (out["with"][:, 0] != out["no_dx_bar"][:, 0]).any()
