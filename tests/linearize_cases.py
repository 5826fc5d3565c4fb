"""The specs, shapes and seeded inputs shared by the CPU and GPU linearisation tests (TEST INFRASTRUCTURE): one spec per
code path, weights and input distributions from variant_census."""
import numpy as np

import variant_census as vc

HEADLINE = "phnn<n=4,hid=128,fixedG,f16x2>"
SPECS = [
    HEADLINE,
    "phnn<n=4,hid=128,fixedG,bf16x3>",
    "phnn<n=2,hid=64,Gnet>",
    "phnn<n=4,m=3,hid=128,Gnet,f16x2>",
    "canonical<hid=128,f16x2>",
    "canonical<hid=128,f16x2,mass=full>",
    "odefunc<n=4,hid=128>",          # the wide input layer
    "odefunc<n=2,hid=128,f16x2>",
    "phnn<n=4,hid=128,fixedG,silu>",
]
POINT_BATCHES = [1, 5, 16, 17, 37]
SHAPES = [(1, 1), (5, 3), (37, 6)]

# the linearisation census (every spec of variant_census.ALL_SPECS, tests/test_gpu_linearize_census.py): point Jacobians on
# the census inputs (variant_census.inputs, POINT_B = 37 points: two full tiles and a ragged one of 5) at the census
# weights and with every MLP weight matrix x3; step Jacobians on case() at a single lane and at 35 points whose H
# divides neither 16 nor the tile, so that tiles straddle rollouts
CENSUS_SCALES = (1.0, 3.0)
CENSUS_SHAPES = [(1, 1), (5, 7)]


def point_tol(s):
    """The census tolerance of the point VJP (test_gpu_variant_census._check_points), which a Jacobian row is."""
    return vc.POINT_TOL * s["tol"] if s["act"] != "relu" else vc.grad_tol(s)


def case(sid, s, B, H, bounded):
    """x0 (B,n), u (B,H,m), the census cost with or without the control bounds, dt.  Bounded: about a fifth of the
    controls lie outside [U_MIN, U_MAX] (variant_census.controls) and, where there is more than one point, one control
    of the last step is NaN (the last step, so that every state the linearisation reads stays finite).  Unbounded: the
    same controls, none of them NaN."""
    rng = np.random.default_rng(vc.seed_of(sid, s) + 1000 + 10 * B + H)
    x0 = vc.states(rng, s["n"], B)
    u = vc.controls(rng, B, H, s["m"])
    cost = vc.cost_of(s, rng)
    if bounded:
        if B * H > 1:
            u[B // 2, H - 1, s["m"] - 1] = np.nan
    else:
        cost.has_u_bounds = 0
    return dict(x0=x0, u=u, cost=cost, dt=vc.dt_of(s))


def outside(u):
    """The adjoint's mask: not (U_MIN <= u <= U_MAX); a NaN counts as outside."""
    return ~((u >= vc.U_MIN) & (u <= vc.U_MAX))


def finite_points(u):
    """(B*H,) mask of the rollout-steps whose controls are all finite (a tolerance against the oracle means nothing on
    a NaN row; those rows are compared as floats instead)."""
    return np.isfinite(u).all(axis=2).reshape(-1)
