"""phnn_model_jacobian and phnn_rollout_linearize on the GPU, one spec per code path (tests/linearize_cases.py):

  1 point Jacobian   row i == phnn_model_vjp(x, u, e_i) as floats, B in {1, 5, 16, 17, 37}; parity against the float64
                     oracle Jacobian at the census tolerance of the point operations
  2 step Jacobians   row i of A[b,t], Bm[b,t] == grad_x0, grad_u of engine.rollout_vjp on the B*H one-step rollouts (their
                     own K1 trajectory, traj_bar = (0, e_i), cost_bar = 0), Euler and RK4, with and without bounds, a few
                     controls outside the range and one NaN; a reference rollout run alone gives the same bits; parity
                     against the float64 oracle at the census gradient tolerance, per rollout-step
  3 isolation        a NaN / inf / 1e30 state or a NaN control at one (b, t) changes no other rollout-step's bits
  4 tile loop        B*H around one grid stride against the same points run in two halves

"As floats": -0 == +0, NaN at the same positions.  The bodies of 1 and 2 live in tests/linearize_checks.py, which states the rule
of the composed reference at a NaN control; tests/test_gpu_linearize_census.py runs them on every census spec."""
import numpy as np
import pytest

import heterogeneous as het
import linearize_cases as lc
import linearize_checks as lk
import linearize_model as lm
import oracle_lib as ol
import variant_census as vc
import wgrad_checks as wc
from linearize_checks import npf
from test_gpu_footprint import engine
from tvlqr_model import same_floats

pytestmark = pytest.mark.gpu
INTEGS = ["euler", "rk4"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


# ----------------------------------------------------------------------------- 1. point Jacobian
@pytest.mark.parametrize("sid", lc.SPECS)
def test_point_jacobian(torch, sid):
    s, eng = vc.CENSUS[sid], engine(sid)
    d = vc.inputs(sid, s)
    for B in lc.POINT_BATCHES:
        A, Bm, bad = lk.point_rows(eng, d["x"][:B], d["u"][:B], sid)
        assert not bad, bad
    m64 = ol.OracleModel(vc.build_state_dict(sid, s), "f64", activation=s["act"])
    (eA, eB), tol = lk.point_errors(m64, d["x"], d["u"], A, Bm), vc.POINT_TOL * s["tol"]
    print(f"\n{sid}: point Jacobian A {eA / tol:.3f}, Bm {eB / tol:.3f} of the tolerance {tol:.1e}")
    assert eA <= tol and eB <= tol


def test_point_jacobian_of_a_model_class(torch):
    """_EngineBacked.jacobian: the model classes reach the same kernel."""
    import os
    import torch as t
    from phnn_mpc_amd.models import pHNN
    w = ol.load_weights("phnn_cartpole")
    model = pHNN(os.path.join(vc.ROOT, "configs", "cartpole_mpc.yaml"))
    model.load_state_dict({k: t.tensor(v) for k, v in w.items()})
    model.use_device("cuda:0")
    rng = np.random.default_rng(3)
    x, u = vc.states(rng, 4, 19), rng.uniform(-1, 1, size=(19, 1)).astype(np.float32)
    A, Bm = model.jacobian(t.tensor(x), t.tensor(u))
    A2, B2 = model.engine.jacobian(x, u)
    assert t.equal(A, A2) and t.equal(Bm, B2)
    rA, rB = lm.oracle_jacobian(ol.OracleModel(w, "f64"), x, u)
    assert vc.err_max(npf(A), rA) <= vc.POINT_TOL and vc.err_max(npf(Bm), rB) <= vc.POINT_TOL


# ----------------------------------------------------------------------------- 2. step Jacobians
@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("sid", lc.SPECS)
def test_rollout_linearize(torch, sid, integ):
    s, eng = vc.CENSUS[sid], engine(sid)
    m64 = ol.OracleModel(vc.build_state_dict(sid, s), "f64", activation=s["act"])
    worst = 0.0
    for B, H in lc.SHAPES:
        for bounded in (False, True):
            c = lc.case(sid, s, B, H, bounded)
            what = f"{sid} {integ} B{B} H{H} bounded={bounded}"
            r = lk.step_jacobians(torch, eng, m64, s, c, integ, bounded, what)
            assert not r["bad"], r["bad"]
            # a reference rollout run alone gives the bits it gives in the batch
            pts = sorted({0, (B * H) // 2, B * H - 1})
            sA, sB = lk.composed(eng, r["traj"], c["u"], c["cost"], integ, c["dt"], points=pts)
            assert same_floats(sA, r["rA"][pts]) and same_floats(sB, r["rB"][pts]), what
            worst = max(worst, r["err"] / vc.grad_tol(s))
            assert r["err"] <= vc.grad_tol(s), (what, r["err"], vc.grad_tol(s))
    print(f"\n{sid} {integ}: worst step-Jacobian error {worst:.3f} of the tolerance {vc.grad_tol(s):.1e}")


def test_no_cost_means_no_clamp(torch):
    sid = lc.HEADLINE
    s, eng = vc.CENSUS[sid], engine(sid)
    c = lc.case(sid, s, 5, 3, bounded=False)
    A, Bm, traj = eng.rollout_linearize(c["x0"], c["u"], c["cost"], "rk4", c["dt"])
    A2, B2, _ = eng.rollout_linearize(c["x0"], c["u"], None, "rk4", c["dt"], traj=traj)
    assert torch.equal(A, A2) and torch.equal(Bm, B2)


# ----------------------------------------------------------------------------- 3. isolation
_VALUE = {"nan_state": np.nan, "inf_state": np.inf, "state_1e30": 1e30}


@pytest.mark.parametrize("kind", wc.ISOLATION_KINDS)
@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("sid", [lc.HEADLINE, "odefunc<n=4,hid=128>", "phnn<n=2,hid=64,Gnet>"])
def test_rollout_steps_are_independent(torch, sid, integ, kind):
    """One poisoned (b, t) per poisoned rollout (first and last lane of a tile, a tile boundary, the ragged tile): every
    other rollout-step -- the other steps of the same rollout included -- keeps its bits."""
    s, eng = vc.CENSUS[sid], engine(sid)
    n, m, B, H = s["n"], s["m"], 37, 6
    c = lc.case(sid, s, B, H, bounded=False)
    A, Bm, traj = eng.rollout_linearize(c["x0"], c["u"], c["cost"], integ, c["dt"])
    tr, u = npf(traj).copy(), c["u"].copy()
    hit = np.zeros((B, H), bool)
    for b in het.POISONED:
        t = b % H
        hit[b, t] = True
        if kind == "nan_control":
            u[b, t, b % m] = np.nan
        else:
            tr[b, t, b % n] = _VALUE[kind]
    A2, B2, _ = eng.rollout_linearize(c["x0"], u, c["cost"], integ, c["dt"], traj=tr)
    A, Bm, A2, B2 = npf(A), npf(Bm), npf(A2), npf(B2)
    assert het.same_bits(A[~hit], A2[~hit]) and het.same_bits(Bm[~hit], B2[~hit])
    if kind == "nan_state":
        assert np.isnan(A2[hit]).any(axis=(1, 2)).all()  # and the poisoned steps show it


@pytest.mark.parametrize("kind", wc.ISOLATION_KINDS)
def test_points_are_independent(torch, kind):
    sid = lc.HEADLINE
    s, eng = vc.CENSUS[sid], engine(sid)
    d = vc.inputs(sid, s)
    x, u = het.poison_point(kind, d["x"], d["u"])
    keep = het.others(len(x))
    A, Bm = eng.jacobian(d["x"], d["u"])
    A2, B2 = eng.jacobian(x, u)
    assert het.same_bits(npf(A)[keep], npf(A2)[keep]) and het.same_bits(npf(Bm)[keep], npf(B2)[keep])


# ----------------------------------------------------------------------------- 4. tile loop
@pytest.mark.parametrize("integ", INTEGS)
def test_tile_loop_around_one_grid_stride(torch, integ):
    """H = 1, B around one stride of the tile loop, against the same points run in two halves (bitwise, on the device).
    The point kernels launch at most 4 n_cu workgroups of 8 waves: one stride is 4 n_cu * 8 * 16 points; n_cu * 8 * 16
    (one workgroup per CU, the last size at which no wave loops) is covered too."""
    sid = lc.HEADLINE
    s, eng = vc.CENSUS[sid], engine(sid)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(11)
    for stride in (n_cu * 8 * 16, 4 * n_cu * 8 * 16):
        big = stride + 1
        traj = torch.zeros(big, 2, 4, dtype=torch.float32, device="cuda:0")
        traj[:, 0] = torch.as_tensor(vc.states(rng, 4, big), device="cuda:0")
        u = torch.as_tensor(vc.controls(rng, big, 1, 1), device="cuda:0")
        cost = vc.cost_of(s, rng)
        for B in (stride - 1, stride, stride + 1):
            A, Bm, _ = eng.rollout_linearize(traj[:B, 0], u[:B], cost, integ, 0.02, traj=traj[:B])
            h = B // 2 + 3  # not a multiple of 16: the halves have ragged tiles of their own
            A1, B1, _ = eng.rollout_linearize(traj[:h, 0], u[:h], cost, integ, 0.02, traj=traj[:h])
            A2, B2, _ = eng.rollout_linearize(traj[h:B, 0], u[h:B], cost, integ, 0.02, traj=traj[h:B])
            i32 = torch.int32
            assert torch.equal(A.view(i32), torch.cat([A1, A2]).view(i32)), (integ, B)
            assert torch.equal(Bm.view(i32), torch.cat([B1, B2]).view(i32)), (integ, B)
            assert bool(torch.isfinite(A).all())
        if stride == 4 * n_cu * 8 * 16:
            x, uu = traj[:big, 0].contiguous(), u[:big, 0].contiguous()
            for B in (stride - 1, stride, stride + 1):
                A, Bm = eng.jacobian(x[:B], uu[:B])
                h = B // 2 + 3
                A1, B1 = eng.jacobian(x[:h], uu[:h])
                A2, B2 = eng.jacobian(x[h:B], uu[h:B])
                assert torch.equal(A.view(i32), torch.cat([A1, A2]).view(i32)) and torch.equal(Bm.view(i32), torch.cat([B1, B2]).view(i32))
