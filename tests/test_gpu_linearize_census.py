"""The linearisation kernels of every census spec (tests/variant_census.py ALL_SPECS: the 50 variants and the 7 zero-padded
models) on the GPU.  k_model_jacobian<M>, k_rollout_linearize<M, EULER> and k_rollout_linearize<M, RK4> are instantiated
once per variant; tests/test_gpu_linearize.py runs nine of them at the wrapper's shapes, this file runs them all, with the
same checks (tests/linearize_checks.py) on the smallest inputs at which a variant can differ:

  point   variant_census.inputs' x, u (37 points: two full tiles and a ragged one of 5), at the census weights and with
          every MLP weight matrix x3: row i of A, Bm == phnn_model_vjp(x, u, e_i) as floats; A, Bm against the float64
          oracle Jacobian at the census tolerance of the point VJP (linearize_cases.point_tol)
  rollout (B, H) in {(1, 1), (5, 7)}, Euler and RK4, with and without bounds (controls outside them, one NaN control):
          == the composed form through phnn_rollout_vjp as floats, exactly zero Bm columns at clamped controls, and the
          float64 oracle's step Jacobians on the stored trajectory at variant_census.grad_tol per rollout-step

tests/test_linearize_model.py holds the float32 oracle to a fifth of these tolerances on the same inputs.  Every check of a
spec is measured and reported in one line before the test asserts."""
import pytest

import linearize_cases as lc
import linearize_checks as lk
import oracle_lib as ol
import variant_census as vc
from test_gpu_variant_census import Report, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def bitwise(rep, what, bad):
    rep.rows.append((what, float(bool(bad)), 0.0))
    rep.bad += bad


def _rollouts(rep, torch, eng, m64, sid, s):
    for integ in ("euler", "rk4"):
        for B, H in lc.CENSUS_SHAPES:
            for bounded in (False, True):
                tag = f"{integ} B{B} H{H} bounded={bounded}"
                r = lk.step_jacobians(torch, eng, m64, s, lc.case(sid, s, B, H, bounded), integ, bounded, f"{sid} {tag}")
                bitwise(rep, f"rollout_rows {tag}", r["bad"])
                rep.le(f"rollout {tag}", r["err"], vc.grad_tol(s))


@pytest.mark.parametrize("sid", list(vc.ALL_SPECS))
def test_linearisation_of_the_variant(torch, sid):
    variant, s = vc.ALL_SPECS[sid]
    rep = Report(sid)
    d = vc.inputs(sid, s)
    for scale in lc.CENSUS_SCALES:
        sd = vc.build_state_dict(sid, s, hidden_scale=scale)
        eng = _engine(sd, s)
        assert eng.variant == variant, (sid, eng.variant)
        m64 = ol.OracleModel(sd, "f64", activation=s["act"])
        tag = f"point_x{scale:g}"
        A, Bm, bad = lk.point_rows(eng, d["x"], d["u"], f"{sid} x{scale:g}")
        bitwise(rep, f"{tag}_rows", bad)
        eA, eB = lk.point_errors(m64, d["x"], d["u"], A, Bm)
        rep.le(f"{tag} A", eA, lc.point_tol(s))
        rep.le(f"{tag} Bm", eB, lc.point_tol(s))
        if scale == 1.0:
            _rollouts(rep, torch, eng, m64, sid, s)
        del eng
    torch.cuda.synchronize()
    rep.finish(digits=3)
