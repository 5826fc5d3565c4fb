"""Input builders for the heterogeneous-batch tests (TEST INFRASTRUCTURE): batches whose rollouts differ in magnitude or
are partly non-finite, shared by tests/test_heterogeneous_model.py (CPU: the float32 oracle) and
tests/test_gpu_heterogeneous.py (GPU: the kernels).  Specs, weights, census inputs and tolerances come from
tests/variant_census.py.

Three groups:

  A  power-of-two homogeneity: per-rollout scales 2^k_b on the cotangents of rollout_vjp / vjp (row_exponents,
     row_scales: k_b = 5 ((7 b mod 17) - 8), -40 .. 40, mixed inside every 16-rollout tile, rollouts 3 and 20 scaled
     by exactly 0) and whole-cost scales 2^k on Q, R and barrier_weight (COST_EXPONENTS, scale_cost).
  B  isolation: a clean batch and a copy in which the rollouts POISONED carry a non-finite or extreme state or control
     (POISONS, poison_rollout, poison_point); a NaN control with and without the control bounds.
  C  the state-magnitude ladder (ladder, ladder_states, DROPPED): the census states times 10^j, one component at 6.0e4 / 7.0e4,
     and for the canonical model the angle at 30, 300 and 2900.
"""
import copy

import numpy as np

import variant_census as vc

B, H = 37, 6            # two full 16-rollout tiles and a ragged one of 5
SPLIT_BATCHES = (1, 17)  # further batch sizes for the split-tile kernels
INTEGRATORS = ("euler", "rk4")

# one spec per family (A3, B, C)
FAMILIES = ["phnn<n=4,hid=128,fixedG,f16x2>", "phnn<n=4,hid=128,Gnet,f16x2>", "canonical<hid=128,f16x2>",
            "odefunc<n=2,hid=128,f16x2>", "phnn<n=4,m=3,hid=128,Gnet,f16x2>"]
# B: + the f32 and bf16x3 modes of the cart-pole pHNN, one SiLU and one ReLU model
ISOLATION_SPECS = FAMILIES + ["phnn<n=4,hid=128,fixedG>", "phnn<n=4,hid=128,fixedG,bf16x3>",
                              "phnn<n=4,hid=128,fixedG,silu>", "phnn<n=4,hid=128,fixedG,relu>"]
# C: the same families, the pHNN and canonical cart-pole specs in all three matmul modes
LADDER_SPECS = ISOLATION_SPECS + ["canonical<hid=128>", "canonical<hid=128,bf16x3>"]
GELU_SPEC = "phnn<n=4,hid=128,fixedG,gelu>"


def mode_of(sid):
    """The matmul mode a census variant name states."""
    return "f16x2" if "f16x2" in sid else ("bf16x3" if "bf16x3" in sid else "f32")


# ----------------------------------------------------------------------------- A: power-of-two scales
ZERO_ROWS = (3, 20)
COST_EXPONENTS = (-40, -13, 0, 13, 40)


def row_exponents(nb):
    return 5 * ((7 * np.arange(nb)) % 17 - 8)


def row_scales(nb):
    """float32 (nb,): 2^k_b, rollouts ZERO_ROWS exactly 0."""
    sc = np.ldexp(np.float32(1.0), row_exponents(nb)).astype(np.float32)
    for b in ZERO_ROWS:
        if b < nb:
            sc[b] = 0.0
    return sc


def scaled_rows(base, sc):
    """base (nb, ...) float32 times sc (nb,) per row, in float32: exact while nothing under- or overflows."""
    base = np.asarray(base, np.float32)
    return (base * sc.reshape((-1,) + (1,) * (base.ndim - 1))).astype(np.float32)


def same_bits(a, b):
    """a, b float32 arrays: equal as uint32 (NaNs and the sign of zero included)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def scale_cost(cost, k):
    """A copy of the phnn_cost with Q, R and barrier_weight times 2^k (exact in float32)."""
    c = copy.deepcopy(cost)
    f = float(np.ldexp(1.0, k))
    for i in range(len(c.Q)):
        c.Q[i] = cost.Q[i] * f
    for i in range(len(c.R)):
        c.R[i] = cost.R[i] * f
    c.barrier_weight = cost.barrier_weight * f
    return c


def batch(sid, s, nb=B, horizon=H):
    """Seeded census-rule inputs at the shapes of these tests: x0 (nb,n), U (nb,H,m), point u (nb,m), trajectory
    cotangent T (nb,H+1,n), point cotangent lam (nb,n), the plain cost and the cost with the state barrier."""
    rng = np.random.default_rng(vc.seed_of(sid + "/heterogeneous", s) + nb)
    n, m = s["n"], s["m"]
    d = {"dt": vc.dt_of(s), "cost": vc.cost_of(s, rng), "cost_barrier": vc.cost_of(s, rng, barrier=True)}
    d["x0"], d["U"] = vc.states(rng, n, nb), vc.controls(rng, nb, horizon, m)
    d["u"] = rng.uniform(vc.U_MIN, vc.U_MAX, size=(nb, m)).astype(np.float32)
    d["T"] = rng.normal(size=(nb, horizon + 1, n)).astype(np.float32)
    d["lam"] = rng.normal(size=(nb, n)).astype(np.float32)
    return d


# ----------------------------------------------------------------------------- B: poisoned rollouts
POISONED = (0, 9, 15, 16, 36)  # first and last lane of a tile, a tile boundary, the last rollout of the ragged tile
POISONS = ("nan_state", "inf_state", "state_1e30", "state_7e4", "nan_control", "nan_control_clamped", "inf_control_clamped")
_STATE_VALUE = {"nan_state": np.nan, "inf_state": np.inf, "state_1e30": 1e30, "state_7e4": 7e4}


def unbounded(cost):
    c = copy.deepcopy(cost)
    c.has_u_bounds = 0
    return c


def poison_rollout(kind, x0, U, cost, rows=POISONED):
    """-> (x0', U', cost'): copies with the rollouts `rows` poisoned; cost' is also the cost of the clean run
    (nan_control runs without control bounds, nan_control_clamped keeps them: the clamp passes a NaN on, as torch.clamp
    does, so both give a NaN cost).  The poisoned state component rotates with the rollout (component b mod n);
    controls are poisoned at step 1 (NaN, component b mod m) or at steps 0 and 2 (+inf, -inf)."""
    x0, U = np.array(x0, np.float32), np.array(U, np.float32)
    n = x0.shape[1]
    rows = [b for b in rows if b < len(x0)]
    if kind in _STATE_VALUE:
        for b in rows:
            x0[b, b % n] = _STATE_VALUE[kind]
        return x0, U, cost
    if kind in ("nan_control", "nan_control_clamped"):
        for b in rows:
            U[b, 1, b % U.shape[2]] = np.nan
        return x0, U, unbounded(cost) if kind == "nan_control" else cost
    assert kind == "inf_control_clamped"
    for b in rows:
        U[b, 0, :] = np.inf
        U[b, 2, :] = -np.inf
    return x0, U, cost


def poison_point(kind, x, u, rows=POISONED):
    """The same for the point operations f(x,u) and its VJP (no clamp there: an infinite control stays infinite)."""
    x, u = np.array(x, np.float32), np.array(u, np.float32)
    n = x.shape[1]
    rows = [b for b in rows if b < len(x)]
    for b in rows:
        if kind in _STATE_VALUE:
            x[b, b % n] = _STATE_VALUE[kind]
        elif kind in ("nan_control", "nan_control_clamped"):
            u[b, b % u.shape[1]] = np.nan
        else:
            u[b, :] = np.inf if b % 2 == 0 else -np.inf
    return x, u


def others(nb, rows=POISONED):
    keep = np.ones(nb, bool)
    keep[[b for b in rows if b < nb]] = False
    return keep


# ----------------------------------------------------------------------------- C: the state-magnitude ladder
SCALE_RUNGS = (-12, -8, -4, -2, 0, 1, 2, 3, 4)
BIG_RUNGS = (6.0e4, 7.0e4)     # one component inside / outside the float16 range (65504; 65520 rounds to inf)
THETA_RUNGS = (30.0, 300.0, 2900.0)  # canonical model: the angle, up to sincos_dev's stated |theta| < 3000


def ladder(s):
    """Rung names of a spec, in rising magnitude."""
    r = [f"x1e{j}" for j in SCALE_RUNGS]
    if s["kind"] == "canonical":
        r += [f"theta{t:g}" for t in THETA_RUNGS]
    return r + [f"big{v:g}" for v in BIG_RUNGS]


def ladder_states(s, x, rung):
    """The census states x (nb,n) moved to a rung.  x1e<j>: times 10^j.  big<v>: one component of every row set to
    +-v; the component rotates with the row (b mod n), except for the canonical model, where it is the position
    (component 0): the angle has a stated range of its own, which the theta rungs cover.  theta<t>: the canonical
    model's angle (component 1) set to +-t."""
    x = np.array(x, np.float32)
    nb, n = x.shape
    sign = np.where(np.arange(nb) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if rung.startswith("x1e"):
        return (x.astype(np.float64) * 10.0 ** int(rung[3:])).astype(np.float32)
    if rung.startswith("theta"):
        x[:, 1] = sign * np.float32(float(rung[5:]))
        return x
    v = np.float32(float(rung[3:]))
    comp = np.zeros(nb, int) if s["kind"] == "canonical" else np.arange(nb) % n
    x[np.arange(nb), comp] = sign * v
    return x


def finite_rows(*arrays):
    """(nb,) mask: every entry of the row finite in every array."""
    ok = None
    for a in arrays:
        a = np.asarray(a)
        f = np.isfinite(a.reshape(len(a), -1)).all(axis=1)
        ok = f if ok is None else ok & f
    return ok


GROUPS = ("point", "euler", "rk4")  # what runs on a rung: f, H and the VJP at the states; an H-step rollout from them
_KEYS = {"point": ("f", "Hval", "xb", "ub"), "roll": ("cost", "traj", "grad_u", "grad_x0")}


def group_errors(s, group, out, ref):
    """{check: error / stated tolerance} of one group's outputs `out` against the float64 oracle's `ref` (dicts with
    f, Hval, xb, ub, or with cost, traj, grad_u, grad_x0), taken over the rows of `out` that are finite; the reference
    scale of the point checks, max|.| over the batch, comes from all rows.  -> (errors, finite row mask); with no
    finite row the errors are empty."""
    keys = _KEYS["point" if group == "point" else "roll"]
    fin = finite_rows(*[out[k] for k in keys])
    if not fin.any():
        return {}, fin
    pt = vc.POINT_TOL * s["tol"]
    vt = pt if s["act"] != "relu" else vc.grad_tol(s)
    gt = vc.grad_tol(s)

    def emax(a, r):
        a, r = np.asarray(a, np.float64), np.asarray(r, np.float64)
        return float(np.abs(a[fin] - r[fin]).max() / max(float(np.abs(r).max()), 1e-30))

    if group == "point":
        eH = float(np.abs(np.asarray(out["Hval"], np.float64)[fin] - ref["Hval"][fin]).max()
                   / max(1.0, np.abs(ref["Hval"]).max()))
        return {"f": emax(out["f"], ref["f"]) / pt, "H": eH / pt, "vjp_x": emax(out["xb"], ref["xb"]) / vt,
                "vjp_u": emax(out["ub"], ref["ub"]) / vt}, fin
    return {"cost": vc.err_cost(np.asarray(out["cost"])[fin], ref["cost"][fin]) / (vc.COST_RTOL * s["tol"]),
            "traj": vc.err_traj(np.asarray(out["traj"])[fin], ref["traj"][fin]) / s["tol"],
            "grad_u": vc.err_rows(np.asarray(out["grad_u"])[fin], ref["grad_u"][fin]) / gt,
            "grad_x0": vc.err_rows(np.asarray(out["grad_x0"])[fin], ref["grad_x0"][fin]) / gt}, fin


def oracle_group_outputs(model, d, x, group):
    """One group of the ladder on an OracleModel, at states x."""
    if group == "point":
        f, Hval = model.forward(x, d["u"])
        xb, ub = model.vjp(x, d["u"], d["lam"])
        return dict(f=f, Hval=Hval, xb=xb, ub=ub)
    r = model.rollout(x, d["U"], d["cost"], group, d["dt"], nthreads=8)
    return dict(cost=r["cost"], traj=r["traj"], grad_u=r["grad_u"], grad_x0=r["grad_x0"])


def oracle_margin(s, m32, m64, d, x, group):
    """Worst error / tolerance of the float32 oracle against the float64 oracle on one group (inf where the float32
    oracle is not finite on every row): the admission figure of a rung."""
    e, fin = group_errors(s, group, oracle_group_outputs(m32, d, x, group), oracle_group_outputs(m64, d, x, group))
    return max(e.values()) if fin.all() else float("inf")


# (spec, rung, group) the ladder leaves out: the float32 oracle's own error against the float64 oracle there is above
# ADMIT of the stated tolerance (value: that error / tolerance, inf where the float32 oracle itself is not finite), so
# no float32 implementation can be held to the tolerance.  tests/test_heterogeneous_model.py asserts that every other
# (spec, rung, group) is within ADMIT and that every entry here is indeed above it.
ADMIT = 0.5
DROPPED = {
    ("phnn<n=4,hid=128,fixedG,f16x2>", "x1e4", "point"): 19,
    ("phnn<n=4,hid=128,Gnet,f16x2>", "x1e4", "point"): 1.55,
    ("canonical<hid=128,f16x2>", "x1e3", "euler"): 0.746,
    ("canonical<hid=128,f16x2>", "x1e4", "point"): 16.6,
    ("canonical<hid=128,f16x2>", "x1e4", "euler"): 1.43,
    ("canonical<hid=128,f16x2>", "x1e4", "rk4"): 3.53,
    ("canonical<hid=128,f16x2>", "theta30", "euler"): 0.73,
    ("canonical<hid=128,f16x2>", "theta300", "euler"): 1.05,
    ("canonical<hid=128,f16x2>", "theta300", "rk4"): 1.57,
    ("canonical<hid=128,f16x2>", "theta2900", "rk4"): 0.51,
    ("odefunc<n=2,hid=128,f16x2>", "x1e3", "point"): 0.915,
    ("odefunc<n=2,hid=128,f16x2>", "x1e3", "euler"): 1.77,
    ("odefunc<n=2,hid=128,f16x2>", "x1e3", "rk4"): 1.89,
    ("odefunc<n=2,hid=128,f16x2>", "x1e4", "point"): 0.73,
    ("odefunc<n=2,hid=128,f16x2>", "x1e4", "euler"): 2.74,
    ("odefunc<n=2,hid=128,f16x2>", "x1e4", "rk4"): 2.72,
    ("phnn<n=4,m=3,hid=128,Gnet,f16x2>", "x1e4", "point"): 3.09,
    ("phnn<n=4,m=3,hid=128,Gnet,f16x2>", "big60000", "point"): 58.3,
    ("phnn<n=4,m=3,hid=128,Gnet,f16x2>", "big70000", "point"): 525,
    ("phnn<n=4,hid=128,fixedG>", "x1e3", "point"): 0.668,
    ("phnn<n=4,hid=128,fixedG>", "x1e4", "point"): 11.8,
    ("phnn<n=4,hid=128,fixedG,bf16x3>", "x1e3", "point"): 0.796,
    ("phnn<n=4,hid=128,fixedG,bf16x3>", "x1e4", "point"): 1.18,
    ("phnn<n=4,hid=128,fixedG,silu>", "x1e3", "euler"): 34.3,
    ("phnn<n=4,hid=128,fixedG,silu>", "x1e3", "rk4"): 4.79,
    ("phnn<n=4,hid=128,fixedG,silu>", "x1e4", "point"): 6.79,
    ("phnn<n=4,hid=128,fixedG,silu>", "x1e4", "euler"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,silu>", "x1e4", "rk4"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,silu>", "big60000", "euler"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,silu>", "big60000", "rk4"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,silu>", "big70000", "euler"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,silu>", "big70000", "rk4"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,relu>", "x1e3", "euler"): 0.783,
    ("phnn<n=4,hid=128,fixedG,relu>", "x1e3", "rk4"): 3.74,
    ("phnn<n=4,hid=128,fixedG,relu>", "x1e4", "euler"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,relu>", "x1e4", "rk4"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,relu>", "big60000", "euler"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,relu>", "big60000", "rk4"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,relu>", "big70000", "euler"): float("inf"),
    ("phnn<n=4,hid=128,fixedG,relu>", "big70000", "rk4"): float("inf"),
    ("canonical<hid=128>", "x1e4", "point"): 6.37,
    ("canonical<hid=128>", "x1e4", "euler"): 1.66,
    ("canonical<hid=128>", "x1e4", "rk4"): 2.73,
    ("canonical<hid=128>", "theta300", "euler"): 0.735,
    ("canonical<hid=128>", "theta300", "rk4"): 1.62,
    ("canonical<hid=128>", "theta2900", "euler"): 0.703,
    ("canonical<hid=128,bf16x3>", "x1e4", "point"): 4.36,
    ("canonical<hid=128,bf16x3>", "x1e4", "euler"): 0.919,
    ("canonical<hid=128,bf16x3>", "x1e4", "rk4"): 10.5,
    ("canonical<hid=128,bf16x3>", "theta300", "euler"): 4.42,
    ("canonical<hid=128,bf16x3>", "theta300", "rk4"): 10.6,
    ("canonical<hid=128,bf16x3>", "theta2900", "euler"): 0.623,
}


def admitted(sid, s):
    """[(rung, group)] the ladder runs for a spec."""
    return [(r, g) for r in ladder(s) for g in GROUPS if (sid, r, g) not in DROPPED]


# ----------------------------------------------------------------------------- GELU second derivative far out
GELU_Z = (1e19, -1e19, 2e19, -2e19)  # z^2 overflows float32 from 1.85e19 on; phi''(z) = pdf(z) (2 - z^2) -> 0
GELU_UNIT = 5


def gelu_state_dict(sid, s, z):
    """The spec's weights with the bias of one first-layer unit of H_net set to z: that unit's pre-activation is z
    to float32 precision for every O(1) state."""
    sd = vc.build_state_dict(sid, s)
    b = sd["H_net.net.0.bias"].copy()
    b[GELU_UNIT] = np.float32(z)
    sd["H_net.net.0.bias"] = b
    return sd
