"""CPU tests (no GPU) of the float64 references the GPU linearisation tests trust (tests/linearize_model.py): the oracle
Jacobian built from unit-cotangent VJPs really is the Jacobian (central differences), the one-step rollout adjoint gives
the step Jacobians (Euler I + dt A, RK4 the composed stage Jacobians, clamped controls an exactly zero column), and the
float32 oracle stays inside the tolerances the GPU tests apply on the same inputs -- so those tolerances are not
absorbing the inputs' conditioning."""
import numpy as np
import pytest

import linearize_cases as lc
import linearize_model as lm
import oracle_lib as ol
import variant_census as vc

# one spec per family, with a state-dependent G / full mass matrix / the wide input layer: a transposition cannot hide
FAMILIES = ["phnn<n=4,m=3,hid=128,Gnet,f16x2>", "canonical<hid=128,f16x2,mass=full>", "odefunc<n=4,hid=128>"]


def models(sid, precisions=("f64",)):
    s = vc.CENSUS[sid]
    sd = vc.build_state_dict(sid, s)
    return s, [ol.OracleModel(sd, p, activation=s["act"]) for p in precisions]


@pytest.mark.parametrize("sid", FAMILIES)
def test_oracle_jacobian_is_the_jacobian(sid):
    """Unit-cotangent VJPs against central differences of forward in float64, h = 1e-5 (truncation + rounding about
    1e-9): within 1e-6 of the largest entry."""
    s, (m64,) = models(sid)
    d = vc.inputs(sid, s)
    A, Bm = lm.oracle_jacobian(m64, d["x"], d["u"])
    fA, fB = lm.fd_jacobian(m64, d["x"], d["u"])
    assert A.shape == (vc.POINT_B, s["n"], s["n"]) and Bm.shape == (vc.POINT_B, s["n"], s["m"])
    eA, eB = vc.err_max(A, fA), vc.err_max(Bm, fB)
    print(f"\n{sid}: A {eA:.2e}, Bm {eB:.2e} of the largest entry")
    assert eA <= 1e-6 and eB <= 1e-6
    # and it is not symmetric by accident: the transposed reference is far away
    assert vc.err_max(A, np.swapaxes(fA, 1, 2)) > 1e-3


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("sid", FAMILIES)
def test_one_step_rollout_adjoint_gives_the_step_jacobians(sid, integ):
    s, (m64,) = models(sid)
    case = lc.case(sid, s, 5, 3, bounded=False)
    traj = m64.rollout(case["x0"], case["u"], case["cost"], integ, case["dt"], grad=False)["traj"]
    A, Bm = lm.oracle_linearize(m64, traj, case["u"], case["cost"], integ, case["dt"])
    cA, cB = lm.composed_step(m64, traj[:, :3].reshape(15, -1), case["u"].reshape(15, -1), integ, case["dt"])
    eA, eB = vc.err_max(A.reshape(cA.shape), cA), vc.err_max(Bm.reshape(cB.shape), cB)
    print(f"\n{sid} {integ}: A {eA:.2e}, Bm {eB:.2e}")
    assert eA <= 1e-12 and eB <= 1e-12  # float64 against float64, another order of the same sums
    if integ == "euler":  # and in words: I + dt A, dt B
        pA, pB = lm.oracle_jacobian(m64, traj[:, :3].reshape(15, -1), case["u"].reshape(15, -1))
        assert vc.err_max(A.reshape(pA.shape), np.eye(s["n"]) + case["dt"] * pA) <= 1e-12
        assert vc.err_max(Bm.reshape(pB.shape), case["dt"] * pB) <= 1e-12


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_clamped_controls_give_an_exactly_zero_column(integ):
    sid = FAMILIES[0]
    s, (m64,) = models(sid)
    case = lc.case(sid, s, 37, 6, bounded=True)
    u = case["u"]
    out = lc.outside(u)
    assert out.any() and np.isnan(u).sum() == 1 and not out.all()
    traj = m64.rollout(case["x0"], u, case["cost"], integ, case["dt"], grad=False)["traj"]
    assert np.isfinite(traj[:, :6]).all()  # the NaN control sits in the last step: every state read is finite
    A, Bm = lm.oracle_linearize(m64, traj, u, case["cost"], integ, case["dt"])
    cols = np.broadcast_to(out[:, :, None, :], Bm.shape)
    assert np.all(Bm[cols] == 0.0) and np.all(Bm[~cols] != 0.0)
    # inside the bounds the clamp is the identity: the unclamped linearisation gives the same entries
    A2, B2 = lm.oracle_linearize(m64, traj, np.nan_to_num(u), None, integ, case["dt"])
    inside = ~out.any(axis=2)
    assert np.array_equal(Bm[inside], B2[inside]) and np.array_equal(A[inside], A2[inside])


@pytest.mark.parametrize("sid", lc.SPECS)
def test_float32_oracle_is_inside_the_gpu_tolerances(sid):
    """The yardstick: on the GPU tests' own inputs the float32 restatement of the same algebra meets the tolerances
    those tests apply to the kernels (point: POINT_TOL x tol with err_max; rollout rows: grad_tol per rollout-step)."""
    s, (m32, m64) = models(sid, ("f32", "f64"))
    d = vc.inputs(sid, s)
    pt = vc.POINT_TOL * s["tol"]
    A, Bm = lm.oracle_jacobian(m32, d["x"], d["u"])
    rA, rB = lm.oracle_jacobian(m64, d["x"], d["u"])
    worst = {"point": max(vc.err_max(A, rA), vc.err_max(Bm, rB)) / pt}
    for B, H in lc.SHAPES:
        for integ in ("euler", "rk4"):
            for bounded in (False, True):
                case = lc.case(sid, s, B, H, bounded)
                traj = m64.rollout(case["x0"], case["u"], case["cost"], integ, case["dt"], grad=False)["traj"]
                traj = traj.astype(np.float32)
                keep = lc.finite_points(case["u"])
                A, Bm = lm.oracle_linearize(m32, traj, case["u"], case["cost"], integ, case["dt"])
                rA, rB = lm.oracle_linearize(m64, traj, case["u"], case["cost"], integ, case["dt"])
                e = max(vc.err_rows(lm.rows_of(A)[keep], lm.rows_of(rA)[keep]),
                        vc.err_rows(lm.rows_of(Bm)[keep], lm.rows_of(rB)[keep]))
                worst["rollout"] = max(worst.get("rollout", 0.0), e / vc.grad_tol(s))
    print(f"\n{sid}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " (float32 oracle error / tolerance)")
    assert worst["point"] <= 1.0 and worst["rollout"] <= 1.0


MARGIN = 0.2  # test_variant_census.MARGIN: the float32 oracle's error as a fraction of the stated tolerance


def census_margins(sid, s):
    """{check: float32-oracle error / tolerance} on exactly the inputs of tests/test_gpu_linearize_census.py."""
    d = vc.inputs(sid, s)
    out = {}
    for scale in lc.CENSUS_SCALES:
        sd = vc.build_state_dict(sid, s, hidden_scale=scale)
        m32, m64 = (ol.OracleModel(sd, p, activation=s["act"]) for p in ("f32", "f64"))
        A, Bm = lm.oracle_jacobian(m32, d["x"], d["u"])
        rA, rB = lm.oracle_jacobian(m64, d["x"], d["u"])
        out[f"point x{scale:g}"] = max(vc.err_max(A, rA), vc.err_max(Bm, rB)) / lc.point_tol(s)
        if scale != 1.0:
            continue
        for B, H in lc.CENSUS_SHAPES:
            for integ in ("euler", "rk4"):
                for bounded in (False, True):
                    case = lc.case(sid, s, B, H, bounded)
                    traj = m64.rollout(case["x0"], case["u"], case["cost"], integ, case["dt"], grad=False)["traj"]
                    traj = traj.astype(np.float32)
                    assert np.isfinite(traj[:, :H]).all(), (sid, B, H, integ, bounded)  # every row the linearisation reads
                    keep = lc.finite_points(case["u"])
                    assert int((~keep).sum()) == (1 if bounded and B * H > 1 else 0)
                    A, Bm = lm.oracle_linearize(m32, traj, case["u"], case["cost"], integ, case["dt"])
                    rA, rB = lm.oracle_linearize(m64, traj, case["u"], case["cost"], integ, case["dt"])
                    e = max(vc.err_rows(lm.rows_of(A)[keep], lm.rows_of(rA)[keep]),
                            vc.err_rows(lm.rows_of(Bm)[keep], lm.rows_of(rB)[keep]))
                    out["rollout"] = max(out.get("rollout", 0.0), e / vc.grad_tol(s))
    return out


@pytest.mark.parametrize("sid", list(vc.ALL_SPECS))
def test_float32_oracle_leaves_room_under_the_census_tolerances(sid):
    """The same yardstick for the linearisation census, every spec: a fifth of each tolerance, so that a correct float32
    kernel has room."""
    out = census_margins(sid, vc.ALL_SPECS[sid][1])
    print(f"\n{sid}: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()) + " (float32 oracle error / tolerance)")
    assert all(v <= MARGIN for v in out.values()), (sid, out)
