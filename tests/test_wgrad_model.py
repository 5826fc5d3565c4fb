"""The weight-gradient checks (tests/wgrad_checks.py) on the CPU: what tests/test_gpu_wgrad_structure.py asks of the
kernels is first shown to be a property of float32 arithmetic, on the float32 C oracle (built with -ffp-contract=off),
and the yardstick itself is kept honest.

W2  Uniform 2^k homogeneity, bit for bit: every cotangent (traj_bar, dx_bar, lam, Hbar) times 2^k, k = -40, -13, 13, 40,
    gives grad_theta, grad_u, grad_x0 = 2^k x the k = 0 results; nothing leaves the normal float32 range; cotangents
    of exactly 0 give 0.
W4  Zero-cotangent independence: with the cotangents of the points or rollouts {0, 9, 15, 16, 36} exactly 0, replacing
    their states and controls by other finite values does not change one bit of grad_theta.
S   The float64 superposition is exact: the float64 sum of the per-point gradient blobs, accumulated in batch order,
    equals the batched float64 gradient bit for bit; the sum of per-rollout (and per-tile) blobs, which associates
    the H x stages terms of an entry differently, equals it to 1e-12 under the metric.  So sum_c contrib_c IS the
    reference.
M   The float32 oracle's entrywise metric per spec, printed, below 2e-4 (a guard on the yardstick and on the inputs,
    not on a kernel); every tensor that is not a buffer or an autograd constant has a nonzero scale, and the buffers
    are exactly zero.

Worst tensor of the float32 oracle under the metric, per spec (37 points | (37, 6) Euler | (37, 6) RK4; for the families
also one point | Euler with the 2^k_b scales mixed in every tile):

    phnn<n=4,hid=128,fixedG>                   1.0e-06  1.1e-06  1.3e-06  1.6e-05  1.1e-05
    phnn<n=4,hid=64,fixedG>                    6.8e-07  7.4e-07  7.7e-07
    phnn<n=2,hid=64,Gnet>                      5.8e-07  6.8e-07  6.5e-07  1.4e-05  1.1e-05
    phnn<n=2,hid=64,fixedG>                    5.2e-07  6.2e-07  7.3e-07
    canonical<hid=128>                         4.7e-07  6.4e-07  6.9e-07
    canonical<hid=64>                          1.0e-06  8.3e-07  1.1e-06  6.8e-06  1.0e-05
    phnn<n=4,hid=128,fixedG,f16x2>             7.5e-07  1.0e-06  1.0e-06
    canonical<hid=128,f16x2>                   5.4e-07  4.4e-07  8.4e-07  8.6e-06  2.6e-06
    phnn<n=4,hid=128,Gnet,f16x2>               7.2e-07  6.9e-07  8.8e-07  1.5e-05  2.2e-06
    phnn<n=2,hid=128,Gnet,f16x2>               1.0e-06  1.6e-06  1.0e-06
    phnn<n=2,hid=128,fixedG,f16x2>             3.9e-07  5.6e-07  8.4e-07
    phnn<n=4,m=2,hid=128,fixedG,f16x2>         9.5e-07  9.5e-07  9.9e-07
    phnn<n=4,m=2,hid=128,Gnet,f16x2>           1.5e-06  1.4e-06  1.2e-06
    canonical<m=2,hid=128,f16x2>               1.5e-06  9.2e-07  1.5e-06
    phnn<n=4,m=3,hid=128,fixedG,f16x2>         6.2e-07  7.0e-07  9.9e-07
    phnn<n=4,m=3,hid=128,Gnet,f16x2>           5.7e-07  6.1e-07  1.1e-06  1.2e-05  3.0e-06
    canonical<m=3,hid=128,f16x2>               5.1e-07  6.2e-07  1.2e-06
    phnn<n=4,m=4,hid=128,fixedG,f16x2>         5.5e-07  6.0e-07  9.2e-07
    phnn<n=4,m=4,hid=128,Gnet,f16x2>           1.2e-06  1.5e-06  9.6e-07
    canonical<m=4,hid=128,f16x2>               5.6e-07  4.9e-07  5.5e-07
    canonical<hid=128,f16x2,mass=constant>     2.3e-06  1.1e-06  6.7e-07
    canonical<hid=128,f16x2,mass=diagonal>     1.3e-06  9.3e-07  1.0e-06
    canonical<hid=128,f16x2,mass=full>         9.3e-07  1.0e-06  1.2e-06  1.2e-05  3.8e-06
    phnn<n=4,fixedG>/H96,80,R48                5.6e-07  4.8e-07  7.6e-07  5.3e-06  6.9e-06
    phnn<n=2,Gnet>/H48,40,R56,G36              2.5e-07  3.2e-07  7.8e-07
    phnn<n=4,m=3,Gnet>/H100,128,R64,G90        1.9e-06  7.7e-07  1.3e-06
    canonical/H40,56                           4.3e-07  7.0e-07  8.6e-07
    canonical/H96,72                           7.7e-07  6.1e-07  7.7e-07
"""
import numpy as np
import pytest

import heterogeneous as het
import oracle_lib as ol
import variant_census as vc
import wgrad_checks as wc

INTEGRATORS = het.INTEGRATORS
ZERO_KEYS = ("G_fixed", "G", "M_net.log_a", "M_net.b", "M_net.log_c")  # buffers / constants of the cart-pole models


def _models(sid):
    s = wc.spec(sid)
    sd = vc.build_state_dict(sid, s)
    return s, sd, ol.OracleModel(sd, "f32", activation=s["act"]), ol.OracleModel(sd, "f64", activation=s["act"])


def _normal(a):
    a = np.abs(np.asarray(a, np.float32))
    return bool(np.isfinite(a).all() and (a[a > 0] >= np.finfo(np.float32).tiny).all())


def _scaled(a, k):
    return (np.asarray(a, np.float32) * np.float32(np.ldexp(1.0, k))).astype(np.float32)


def test_specs_and_families():
    assert len(wc.WG_SPECS) >= 20 and all(wc.spec(sid)["wgrad"] for sid in wc.WG_SPECS)
    assert set(wc.WG_FAMILIES) <= set(wc.WG_SPECS) and set(wc.GRID_SPECS) <= set(wc.WG_FAMILIES)
    assert wc.spec(wc.PADDED_PHNN)["widths"] == {"H": [96, 80], "R": [48]}
    assert any(sid in vc.PADDED for sid in wc.WG_SPECS)
    assert {het.mode_of(vc.ALL_SPECS[sid][0]) for sid in wc.WG_FAMILIES} == {"f32", "f16x2"}
    n_cu = 256
    tiles = wc.grid_tiles(n_cu)
    per = [-(-t // min(t, n_cu)) for t in tiles]
    assert set(per) >= {1, 2, 3} and any(t % min(t, n_cu) for t in tiles)
    assert all(wc.grid_points(t) % 16 == 5 and -(-wc.grid_points(t) // 16) == t for t in tiles)


@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_float32_oracle_is_uniformly_homogeneous(sid):
    """W2 on the float32 oracle."""
    s, sd, m32, _ = _models(sid)
    d = wc.batch(sid, s)
    g0 = wc.oracle_point(m32, d)
    assert _normal(g0) and np.abs(g0).max() > 0
    r0 = {i: wc.oracle_rollout(m32, d, i) for i in INTEGRATORS}
    for k in wc.EXPONENTS:
        dk = wc.with_scales(d, np.float32(np.ldexp(1.0, k)))
        g = wc.oracle_point(m32, dk)
        assert het.same_bits(g, _scaled(g0, k)), (sid, k, "point")
        assert _normal(g), (sid, k, "point grad_theta leaves the normal range")
        for integ in INTEGRATORS:
            r = wc.oracle_rollout(m32, dk, integ)
            for q in ("grad_theta", "grad_u", "grad_x0"):
                assert het.same_bits(r[q], _scaled(r0[integ][q], k)), (sid, k, integ, q)
                assert _normal(r[q]), (sid, k, integ, q, "leaves the normal range")
            assert het.same_bits(r["traj"], r0[integ]["traj"]) and het.same_bits(r["dX"], r0[integ]["dX"])
    dz = wc.with_scales(d, np.float32(0.0))
    assert not wc.oracle_point(m32, dz).any()
    for integ in INTEGRATORS:
        r = wc.oracle_rollout(m32, dz, integ)
        assert not r["grad_theta"].any() and not r["grad_u"].any() and not r["grad_x0"].any()


@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_float32_oracle_ignores_zero_cotangent_rows(sid):
    """W4 on the float32 oracle."""
    s, sd, m32, _ = _models(sid)
    d = wc.with_zero_cotangents(wc.batch(sid, s))
    e = wc.replaced_rows(sid, s, d)
    keep = het.others(d["nb"])
    assert het.same_bits(d["x0"][keep], e["x0"][keep]) and not np.array_equal(d["x0"][~keep], e["x0"][~keep])
    assert np.isfinite(e["x0"]).all() and np.abs(e["x0"]).max() < 100.0 and np.isfinite(e["U"]).all()
    assert het.same_bits(wc.oracle_point(m32, d), wc.oracle_point(m32, e)), (sid, "point")
    for integ in INTEGRATORS:
        a, b = wc.oracle_rollout(m32, d, integ), wc.oracle_rollout(m32, e, integ)
        assert het.same_bits(a["grad_theta"], b["grad_theta"]), (sid, integ)
        for q in ("grad_u", "grad_x0"):
            assert het.same_bits(a[q][keep], b[q][keep]), (sid, integ, q)


def _f64_close(sd, batched, tot, sc):
    return all(r <= 1e-12 for r, _ in wc.entry_metric(wc.layout_of(sd), batched, tot, sc).values())


@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_float64_superposition_is_exact(sid):
    """S: the reference of the entrywise metric, sum_c contrib_c, is the batched float64 gradient itself: bit for bit
    for points (one term per point and entry, added in batch order)."""
    s, sd, _, m64 = _models(sid)
    d = wc.batch(sid, s)
    tot, sc = wc.superpose(lambda r: wc.oracle_point(m64, r), d, wc.groups_single(d["nb"]))
    assert np.array_equal(tot, wc.oracle_point(m64, d)), (sid, "point")
    assert (sc >= np.abs(tot)).all()
    tot, sc = wc.superpose(lambda r: wc.oracle_point(m64, r), d, wc.groups_tiles(d["nb"]))
    assert _f64_close(sd, wc.oracle_point(m64, d), tot, sc), (sid, "point, per tile")
    # a rollout adds H x stages terms to every entry, so the per-rollout sums associate differently from the batched
    # run: equal to float64 rounding (1e-12 under the metric, five orders below any float32 figure), not bit for bit
    for integ in INTEGRATORS:
        tot, sc = wc.superpose(lambda r: wc.oracle_rollout(m64, r, integ)["grad_theta"], d, wc.groups_single(d["nb"]))
        assert _f64_close(sd, wc.oracle_rollout(m64, d, integ)["grad_theta"], tot, sc), (sid, integ)
    # mixed scales (W3): the same with the cotangents of rollout b times 2^k_b
    dm = wc.with_scales(d, het.row_scales(d["nb"]))
    tot, sc = wc.superpose(lambda r: wc.oracle_rollout(m64, r, "euler")["grad_theta"], dm, wc.groups_single(d["nb"]))
    assert _f64_close(sd, wc.oracle_rollout(m64, dm, "euler")["grad_theta"], tot, sc), (sid, "mixed scales")
    tot, _ = wc.superpose(lambda r: wc.oracle_point(m64, r), dm, wc.groups_single(d["nb"]))
    assert np.array_equal(tot, wc.oracle_point(m64, dm)), (sid, "point, mixed scales")


def _oracle_metrics(sid, s, sd, m32, m64, d, cases):
    lay = wc.layout_of(sd)
    out = {}
    for name, fn in cases.items():
        tot, sc = wc.superpose(lambda r: fn(m64, r), d, wc.groups_single(d["nb"]))
        met = wc.entry_metric(lay, fn(m32, d), tot, sc)
        assert all(np.isfinite(b) and b >= wc.FACTOR * wc.ORACLE_FLOOR for b in wc.bounds(lay, met, tot, sc).values())
        out[name] = (met, wc.zero_tensors(lay, sc))
    return out


@pytest.mark.parametrize("sid", wc.WG_SPECS)
def test_float32_oracle_metric(sid):
    """M: the yardstick on the float32 oracle, per spec (printed), and the honesty of the inputs."""
    s, sd, m32, m64 = _models(sid)
    d = wc.batch(sid, s)
    cases = {"point": lambda m, r: wc.oracle_point(m, r),
             "euler": lambda m, r: wc.oracle_rollout(m, r, "euler")["grad_theta"],
             "rk4": lambda m, r: wc.oracle_rollout(m, r, "rk4")["grad_theta"]}
    res = _oracle_metrics(sid, s, sd, m32, m64, d, cases)
    if sid in wc.WG_FAMILIES:  # a single point: the contributions do not average out
        d1 = wc.batch(sid, s, 1, 1)
        res["point N=1"] = _oracle_metrics(sid, s, sd, m32, m64, d1, {"p": cases["point"]})["p"]
        dm = wc.with_scales(d, het.row_scales(d["nb"]))
        res["euler mixed scales"] = _oracle_metrics(sid, s, sd, m32, m64, dm, {"e": cases["euler"]})["e"]
    for name, (met, zeros) in res.items():
        worst = max(met, key=lambda k: met[k][0])
        print(f"ORACLE32 {sid} {name}: worst {met[worst][0]:.2e} ({worst}[{met[worst][1]}]); "
              + ", ".join(f"{k} {v[0]:.1e}" for k, v in met.items() if v[0] > 0))
        # H(x)'s output bias enters f = (J - R) grad H + G u only through Hbar: no gradient in a rollout
        allowed = ZERO_KEYS + (() if name.startswith("point") else ("H_net.net.4.bias",))
        assert set(zeros) <= set(allowed), (sid, name, "a parameter tensor has no scale", zeros)
        for k in zeros:
            assert met[k][0] == 0.0, (sid, name, k, "must be exactly zero")
        assert all(v[0] < wc.YARDSTICK_MAX for v in met.values()), (sid, name, met)


def test_metric_sees_what_the_old_criterion_misses():
    """An entry at 1e-3 of the tensor's maximum that is 10 % wrong passes |ours - ref| <= 1e-4 max|ref| and fails the
    entrywise metric by a wide margin; a non-finite entry and a nonzero buffer entry give inf."""
    lay = [("a", 0, (4,)), ("buf", 4, (2,))]
    contrib = np.array([[1.0, 0.5, 5e-4, 0.25, 0.0, 0.0], [1.0, -0.5, 5e-4, 0.25, 0.0, 0.0]])
    tot, sc = contrib.sum(axis=0), np.abs(contrib).sum(axis=0)
    ours = tot.copy()
    ours[2] *= 1.1
    assert np.abs(ours - tot).max() <= 1e-4 * np.abs(tot).max()
    met = wc.entry_metric(lay, ours, tot, sc)
    assert met["a"][1] == 2 and met["a"][0] > 3 * wc.FACTOR * wc.YARDSTICK_MAX and met["buf"] == (0.0, 0)
    ours = tot.copy()
    ours[1] = 3e-7  # the entry whose contributions cancel is judged by what was summed into it
    assert wc.entry_metric(lay, ours, tot, sc)["a"][0] < 3e-7
    ours[5] = 1e-30
    assert wc.entry_metric(lay, ours, tot, sc)["buf"] == (float("inf"), 1)
    ours[0] = np.nan
    assert wc.entry_metric(lay, ours, tot, sc)["a"][0] == float("inf")
    assert wc.bounds(lay, {"a": (1e-9, 0), "buf": (1e-5, 0)}, tot, sc) == {"a": 8 * 2.0 ** -22, "buf": 8e-5}
