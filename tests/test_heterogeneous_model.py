"""The heterogeneous-batch inputs (tests/heterogeneous.py) on the CPU: what tests/test_gpu_heterogeneous.py asks of the
kernels is first shown to be a property of float32 arithmetic, on the float32 C oracle (built with -ffp-contract=off).

A  Power-of-two homogeneity.  Scaling a cotangent, or Q, R and barrier_weight, by 2^k commutes with every float32 add,
   multiply and fma while nothing under- or overflows, and the nonlinear functions see only the state.  On the very
   inputs of the GPU test the float32 oracle satisfies, bit for bit and for every spec of the census,
     A1  rollout_vjp and vjp with per-rollout scales 2^k_b, k_b = 5 ((7 b mod 17) - 8): result = 2^k_b x the result at
         scale 1; rollouts 3 and 20 (scale exactly 0) give zeros;
     A2  rollout cost / grad_u / grad_x0 with Q, R, barrier_weight x 2^k: = 2^k x the k = 0 result, same trajectory.
   Exponent range finally used: the full range asked for, k_b in -40 .. 40 (A1) and k in {-40, -13, 0, 13, 40} (A2);
   no exponent had to be narrowed: every scaled result is a normal float32 (test_scaled_results_stay_normal).

C  Ladder admission.  A (spec, rung, group) is admitted when the float32 oracle's own error against the float64 oracle
   is at most ADMIT = 0.5 of the stated tolerance (variant_census: POINT_TOL, COST_RTOL, the trajectory tolerance,
   grad_tol; unscaled).  Rungs: census states x 10^j, j = -12, -8, -4, -2, 0, 1, 2, 3, 4; one component at 6.0e4 and at
   7.0e4; canonical model: the angle at 30, 300, 2900.  Groups: point (f, H, VJP), euler and rk4 (H = 6 rollout: cost,
   trajectory, grad_u, grad_x0).  Dropped, with the measured float32-oracle error / tolerance (heterogeneous.DROPPED
   holds the same table; this file asserts both directions):

     phnn<n=4,hid=128,fixedG,f16x2>    x1e4 point 19
     phnn<n=4,hid=128,Gnet,f16x2>      x1e4 point 1.55
     canonical<hid=128,f16x2>          x1e3 euler 0.746; x1e4 point 16.6, euler 1.43, rk4 3.53; theta30 euler 0.73;
                                       theta300 euler 1.05, rk4 1.57; theta2900 rk4 0.51
     odefunc<n=2,hid=128,f16x2>        x1e3 point 0.915, euler 1.77, rk4 1.89; x1e4 point 0.73, euler 2.74, rk4 2.72
     phnn<n=4,m=3,hid=128,Gnet,f16x2>  x1e4 point 3.09; big60000 point 58.3; big70000 point 525
     phnn<n=4,hid=128,fixedG>          x1e3 point 0.668; x1e4 point 11.8
     phnn<n=4,hid=128,fixedG,bf16x3>   x1e3 point 0.796; x1e4 point 1.18
     phnn<n=4,hid=128,fixedG,silu>     x1e3 euler 34.3, rk4 4.79; x1e4 point 6.79, euler inf, rk4 inf;
                                       big60000 euler inf, rk4 inf; big70000 euler inf, rk4 inf
     phnn<n=4,hid=128,fixedG,relu>     x1e3 euler 0.783, rk4 3.74; x1e4 euler inf, rk4 inf; big60000 euler inf, rk4 inf;
                                       big70000 euler inf, rk4 inf
     canonical<hid=128>                x1e4 point 6.37, euler 1.66, rk4 2.73; theta300 euler 0.735, rk4 1.62;
                                       theta2900 euler 0.703
     canonical<hid=128,bf16x3>         x1e4 point 4.36, euler 0.919, rk4 10.5; theta300 euler 4.42, rk4 10.6;
                                       theta2900 euler 0.623

   (inf: the float32 oracle itself overflows on some rollout -- SiLU and ReLU are unbounded, the march leaves float32.
   The point errors at 1e3 / 1e4 are the VJP's: the saturated tanh' terms cancel against the large state.)

GELU: with one first-layer pre-activation of H_net at z = +-1e19 and +-2e19 the float32 oracle's VJP is finite and
within ADMIT of POINT_TOL of the float64 oracle (phi''(z) = pdf(z) (2 - z^2) with the polynomial factor kept finite).
"""
import numpy as np
import pytest

import heterogeneous as het
import oracle_lib as ol
import variant_census as vc


def _m32(sid, s):
    return ol.OracleModel(vc.build_state_dict(sid, s), "f32", activation=s["act"])


def _homogeneous(got, base, sc):
    nz = sc != 0
    return het.same_bits(got[nz], het.scaled_rows(base, sc)[nz]) and bool((got[~nz] == 0).all())


def _normal(a):
    """every nonzero entry a normal, finite float32"""
    a = np.abs(np.asarray(a, np.float32))
    return bool(np.isfinite(a).all() and (a[a > 0] >= np.finfo(np.float32).tiny).all())


def test_row_scales_mix_magnitudes_inside_every_tile():
    k, sc = het.row_exponents(het.B), het.row_scales(het.B)
    assert k.min() == -40 and k.max() == 40
    for t0 in (0, 16):
        assert k[t0:t0 + 16].max() - k[t0:t0 + 16].min() >= 70
    assert np.ptp(k[32:]) >= 40
    assert all(sc[b] == 0 for b in het.ZERO_ROWS) and (np.delete(sc, het.ZERO_ROWS) > 0).all()
    assert np.array_equal(np.delete(sc, het.ZERO_ROWS), np.delete(np.exp2(k.astype(np.float64)), het.ZERO_ROWS))


@pytest.mark.parametrize("sid", list(vc.ALL_SPECS))
def test_float32_oracle_is_homogeneous(sid):
    """A1 and A2 on the float32 oracle, bit for bit, on the inputs of the GPU test."""
    s = vc.ALL_SPECS[sid][1]
    m32, d, sc = _m32(sid, s), het.batch(sid, s), het.row_scales(het.B)
    one = np.ones(het.B, np.float32)
    for integ in het.INTEGRATORS:
        gu0, gx0 = m32.rollout_vjp(d["x0"], d["U"], d["cost"], integ, d["dt"], traj_bar=d["T"], cost_bar=one)
        gu, gx = m32.rollout_vjp(d["x0"], d["U"], d["cost"], integ, d["dt"], traj_bar=het.scaled_rows(d["T"], sc),
                                 cost_bar=sc)
        assert np.abs(gu0).max() > 0 and np.abs(gx0).max() > 0
        assert _homogeneous(gu, gu0, sc) and _homogeneous(gx, gx0, sc), (sid, integ, "A1")
        assert _normal(gu) and _normal(gx), (sid, integ, "A1 leaves the normal range")
        r0 = m32.rollout(d["x0"], d["U"], d["cost_barrier"], integ, d["dt"])
        rp = m32.rollout(d["x0"], d["U"], d["cost"], integ, d["dt"])
        assert (r0["cost"] > rp["cost"]).any(), "the barrier is active somewhere"
        for k in het.COST_EXPONENTS:
            r = m32.rollout(d["x0"], d["U"], het.scale_cost(d["cost_barrier"], k), integ, d["dt"])
            f = np.float32(np.ldexp(1.0, k))
            for q in ("cost", "grad_u", "grad_x0"):
                assert het.same_bits(r[q], r0[q] * f), (sid, integ, k, q)
                assert _normal(r[q]), (sid, integ, k, q, "leaves the normal range")
            assert het.same_bits(r["traj"], r0["traj"]), (sid, integ, k)
    xb0, ub0 = m32.vjp(d["x0"], d["u"], d["lam"])
    xb, ub = m32.vjp(d["x0"], d["u"], het.scaled_rows(d["lam"], sc))
    assert _homogeneous(xb, xb0, sc) and _homogeneous(ub, ub0, sc), (sid, "vjp")
    assert _normal(xb) and _normal(ub)


def test_scaled_results_stay_normal():
    """The check above would not notice a result flushed to zero on both sides; _normal does: here it is shown to."""
    assert _normal(np.float32([1.0, 0.0, -3e38, 1.2e-38]))
    assert not _normal(np.float32([1e-39])) and not _normal(np.float32([np.inf]))


def test_poison_builders():
    sid = het.FAMILIES[0]
    s = vc.ALL_SPECS[sid][1]
    d = het.batch(sid, s)
    keep = het.others(het.B)
    assert keep.sum() == het.B - len(het.POISONED)
    for kind in het.POISONS:
        x0, U, cost = het.poison_rollout(kind, d["x0"], d["U"], d["cost"])
        assert het.same_bits(x0[keep], d["x0"][keep]) and het.same_bits(U[keep], d["U"][keep]), kind
        for b in het.POISONED:
            assert not (het.same_bits(x0[b], d["x0"][b]) and het.same_bits(U[b], d["U"][b])), (kind, b)
        assert cost.has_u_bounds == (0 if kind == "nan_control" else 1)
        x, u = het.poison_point(kind, d["x0"], d["u"])
        assert het.same_bits(x[keep], d["x0"][keep]) and het.same_bits(u[keep], d["u"][keep]), kind
    assert d["cost"].has_u_bounds == 1  # the builders copy


@pytest.mark.parametrize("kind", het.POISONS)
def test_float64_oracle_on_the_poisoned_rollouts(kind):
    """What the GPU test expects of the poisoned rollouts themselves: a NaN or infinite state or an unclamped NaN control
    (or one under the clamp, which passes a NaN on) makes the float64 oracle's cost non-finite; clamped infinite controls and the finite extreme states leave it finite."""
    sid = het.FAMILIES[0]
    s = vc.ALL_SPECS[sid][1]
    d = het.batch(sid, s)
    m64 = ol.OracleModel(vc.build_state_dict(sid, s), "f64", activation=s["act"])
    x0, U, cost = het.poison_rollout(kind, d["x0"], d["U"], d["cost"])
    c = m64.rollout(x0, U, cost, "euler", d["dt"], grad=False, traj=False)["cost"]
    rows = list(het.POISONED)
    assert np.isfinite(c[het.others(het.B)]).all()
    if kind in ("nan_state", "inf_state", "nan_control", "nan_control_clamped"):
        assert not np.isfinite(c[rows]).any()
    else:
        assert np.isfinite(c[rows]).all()


@pytest.mark.parametrize("sid", het.ISOLATION_SPECS)
def test_float64_oracle_passes_a_nan_control_through_the_clamp(sid):
    """nan_control_clamped on the oracle alone, at every shape the GPU test runs: the cost is non-finite on exactly
    POISONED, the trajectory is the clean one up to x_1 and non-finite from x_2 on, and both gradients are non-finite
    somewhere besides the entry of the NaN itself -- so what the GPU test asks of the kernels there is not vacuous."""
    s = vc.ALL_SPECS[sid][1]
    m64 = ol.OracleModel(vc.build_state_dict(sid, s), "f64", activation=s["act"])
    for nb in (het.B,) + (het.SPLIT_BATCHES[1:] if s["split"] else ()):
        d = het.batch(sid, s, nb)
        x0, U, cost = het.poison_rollout("nan_control_clamped", d["x0"], d["U"], d["cost"])
        assert cost.has_u_bounds == 1 and het.same_bits(x0, d["x0"])
        keep = het.others(nb)
        rows = np.flatnonzero(~keep)
        assert np.isnan(U).sum() == len(rows) and np.isnan(U[rows, 1]).any(axis=1).all()
        for integ in het.INTEGRATORS:
            r = m64.rollout(x0, U, cost, integ, d["dt"], nthreads=8)
            c = m64.rollout(d["x0"], d["U"], cost, integ, d["dt"], nthreads=8)
            assert not np.isfinite(r["cost"][rows]).any() and np.isfinite(r["cost"][keep]).all(), (sid, nb, integ)
            assert np.array_equal(r["traj"][rows][:, :2], c["traj"][rows][:, :2]), (sid, nb, integ)
            assert (~np.isfinite(r["traj"][rows][:, 2:])).any(axis=2).all(), (sid, nb, integ)
            assert (~np.isfinite(r["grad_u"][rows]) & ~np.isnan(U[rows])).any(axis=(1, 2)).all(), (sid, nb, integ)
            assert (~np.isfinite(r["grad_x0"][rows])).any(axis=1).all(), (sid, nb, integ)
            for q in ("cost", "traj", "grad_u", "grad_x0"):
                assert np.array_equal(r[q][keep], c[q][keep]), (sid, nb, integ, q)


@pytest.mark.parametrize("sid", het.LADDER_SPECS)
def test_ladder_admission(sid):
    """Every (rung, group) the GPU ladder runs leaves the float32 oracle within ADMIT of the tolerance; every dropped
    one does not (the table is not wider than it has to be)."""
    s = vc.ALL_SPECS[sid][1]
    sd = vc.build_state_dict(sid, s)
    m32, m64 = (ol.OracleModel(sd, p, activation=s["act"]) for p in ("f32", "f64"))
    d = het.batch(sid, s)
    bad = {}
    for rung in het.ladder(s):
        x = het.ladder_states(s, d["x0"], rung)
        assert np.isfinite(x).all()
        for g in het.GROUPS:
            r = het.oracle_margin(s, m32, m64, d, x, g)
            if ((sid, rung, g) in het.DROPPED) != (not r <= het.ADMIT):
                bad[(rung, g)] = r
    assert not bad, (sid, bad)
    assert all(k in het.admitted(sid, s) for k in (("x1e0", "point"), ("x1e0", "euler"), ("x1e0", "rk4")))


def test_dropped_table_names_real_rungs():
    for (sid, rung, g), r in het.DROPPED.items():
        assert sid in het.LADDER_SPECS and rung in het.ladder(vc.ALL_SPECS[sid][1]) and g in het.GROUPS
        assert r > het.ADMIT
    # the rungs this ladder exists for stay in: the float16 edge of the two cart-pole f16x2 models, all groups
    for sid in ("phnn<n=4,hid=128,fixedG,f16x2>", "canonical<hid=128,f16x2>"):
        for rung in ("big60000", "big70000"):
            for g in het.GROUPS:
                assert (sid, rung, g) not in het.DROPPED


def test_ladder_states():
    sid = "canonical<hid=128,f16x2>"
    s = vc.ALL_SPECS[sid][1]
    x = het.batch(sid, s)["x0"]
    assert np.abs(het.ladder_states(s, x, "theta2900")[:, 1]).tolist() == [2900.0] * het.B
    big = het.ladder_states(s, x, "big70000")
    assert (np.abs(big[:, 0]) == 7.0e4).all() and het.same_bits(big[:, 1:], x[:, 1:])
    s4 = vc.ALL_SPECS[het.FAMILIES[0]][1]
    big = het.ladder_states(s4, x, "big60000")
    assert all(abs(big[b, b % 4]) == 6.0e4 for b in range(het.B)) and (np.abs(big) == 6.0e4).sum() == het.B
    with np.errstate(over="ignore"):
        assert np.float16(6.0e4) == 6.0e4 and np.isinf(np.float32(7.0e4).astype(np.float16))
    assert np.allclose(het.ladder_states(s, x, "x1e-8"), x * 1e-8, rtol=1e-6, atol=0)


@pytest.mark.parametrize("z", het.GELU_Z)
def test_gelu_far_out_in_the_float32_oracle(z):
    sid = het.GELU_SPEC
    s = vc.ALL_SPECS[sid][1]
    d = het.batch(sid, s)
    sd = het.gelu_state_dict(sid, s, z)
    m32, m64 = (ol.OracleModel(sd, p, activation="gelu") for p in ("f32", "f64"))
    (xb, ub), (rxb, rub) = m32.vjp(d["x0"], d["u"], d["lam"]), m64.vjp(d["x0"], d["u"], d["lam"])
    assert np.isfinite(rxb).all() and np.isfinite(xb).all() and np.isfinite(ub).all()
    assert vc.err_max(xb, rxb) <= het.ADMIT * vc.POINT_TOL and vc.err_max(ub, rub) <= het.ADMIT * vc.POINT_TOL


@pytest.mark.parametrize("sid", het.FAMILIES)
def test_float32_oracle_leaves_room_at_the_scaled_cotangents(sid):
    """A3's yardstick: at the per-rollout scales the float32 oracle is within ADMIT of grad_tol of the float64 oracle."""
    s = vc.ALL_SPECS[sid][1]
    sd = vc.build_state_dict(sid, s)
    m32, m64 = (ol.OracleModel(sd, p, activation=s["act"]) for p in ("f32", "f64"))
    for nb in (het.B,) + (het.SPLIT_BATCHES if s["split"] else ()):
        d, sc = het.batch(sid, s, nb), het.row_scales(nb)
        for integ in het.INTEGRATORS:
            a, r = (m.rollout_vjp(d["x0"], d["U"], d["cost"], integ, d["dt"], traj_bar=het.scaled_rows(d["T"], sc),
                                  cost_bar=sc) for m in (m32, m64))
            assert vc.err_rows(a[0], r[0]) <= het.ADMIT * vc.grad_tol(s), (sid, nb, integ)
            assert vc.err_rows(a[1], r[1]) <= het.ADMIT * vc.grad_tol(s), (sid, nb, integ)
