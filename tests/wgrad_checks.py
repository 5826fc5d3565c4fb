"""Inputs, the entrywise metric and its bound for the weight-gradient tests (TEST INFRASTRUCTURE), shared by
tests/test_wgrad_model.py (CPU: the float32 oracle) and tests/test_gpu_wgrad_structure.py (GPU: the record-emitting
adjoint k_rollout_grad<..., WG=true> / k_model_vjp<..., true>, k_wgrad_reduce and k_wgrad_finish).  Specs, weights and
the input rules come from tests/variant_census.py, scales and poisons from tests/heterogeneous.py.

The metric.  A parameter gradient is a sum of contributions (one per evaluation point, per rollout, or per 16-point
tile).  With contrib_c the float64 oracle's gradient blob of contribution c alone, for entry e of tensor t

    scale_e = sum_c |contrib_c[e]|
    r_t     = max_e |ours[e] - sum_c contrib_c[e]| / (scale_e + 2^-7 max_{e' in t} scale_e')

so an entry is judged against what was summed into IT, not against the tensor's largest entry (the older criterion,
|ours - ref| <= 1e-4 max|ref|, lets an entry at 1e-3 of the maximum be 10 % wrong).  The 2^-7 floor: saturated hidden
units make 1 - a^2 ill-conditioned in any float32 arithmetic; without it the float32 oracle itself sits at 7e-4 on
H_net.net.2.weight of the trained pendulum fixture, with it at 1.1e-5.  Tensors whose float64 gradient is identically
zero (G_fixed, the canonical G, the CartPoleMassMatrix constants) must be exactly zero.

The bound of a tensor: FACTOR * max(r_t of the float32 oracle on the same inputs, 2^-22), FACTOR = 8: the f16x2 image
keeps 22 of 24 product bits (x4), the kernels' tanh (2.5e-7 absolute) and their summation order add x2; the 2^-22 floor
covers tensors where the oracle's own order happens to be near-exact (H_net.net.4.bias: 3e-9).  Five tensor families of
the f16x2 kernels carry a measured factor of their own (FACTORS below).
"""
import numpy as np

import heterogeneous as het
import variant_census as vc
from phnn_mpc_amd import weights

B, H = het.B, het.H              # 37 rollouts or points (two full tiles and a ragged one of 5), 6 steps
SMALL_SHAPES = ((1, 1), (5, 3))  # further (B, H) of the families
EXPONENTS = (-40, -13, 13, 40)   # W2: uniform scales 2^k on every cotangent
FLOOR = 2.0 ** -7
FACTOR = 8.0
ORACLE_FLOOR = 2.0 ** -22
YARDSTICK_MAX = 2e-4             # the float32 oracle's own metric stays below this on every spec (CPU guard)

# every census spec with weight-gradient kernels, padded widths included
WG_SPECS = [sid for sid, (_, s) in vc.ALL_SPECS.items() if s["wgrad"]]
PADDED_PHNN = "phnn<n=4,fixedG>/H96,80,R48"
# one spec per code path of the reduce
WG_FAMILIES = ["phnn<n=4,hid=128,fixedG>",            # f32 image; hbar_R comes from the record (HBREC)
               "phnn<n=4,hid=128,Gnet,f16x2>",        # hbar_R and hbar_G recomputed through v2_frag
               "phnn<n=2,hid=64,Gnet>",               # T = 4 waves
               "canonical<hid=64>",                   # T = 4 waves
               "canonical<hid=128,f16x2>",
               "phnn<n=4,m=3,hid=128,Gnet,f16x2>",
               "canonical<hid=128,f16x2,mass=full>",  # records carry the mass cotangents
               PADDED_PHNN]                           # widths H [96, 80], R [48]: the unpad map of k_wgrad_finish
# W7: record counts around the grid of the reduce
GRID_SPECS = ["phnn<n=4,hid=128,fixedG>", "phnn<n=4,hid=128,Gnet,f16x2>", "canonical<hid=64>"]
ISOLATION_KINDS = ("nan_state", "inf_state", "state_1e30", "nan_control")


def grid_tiles(n_cu):
    """Tile (= record) counts that give the workgroups of k_wgrad_reduce (wgrad_rows = min(n_rec, n_cu), striding over
    the records, software-pipelined over two exchange buffers) one, two and three records per stride, an uneven split
    and both buffer parities."""
    return [1, 2, n_cu - 1, n_cu, n_cu + 1, 2 * n_cu, 2 * n_cu + 1, 3 * n_cu + 2]


def grid_points(tiles):
    """N of a point-mode call with `tiles` records and a ragged last tile of 5."""
    return 16 * tiles - 11


def spec(sid):
    return vc.ALL_SPECS[sid][1]


def owned(s, key):
    """Tensors the kernels own.  A MassMatrixNetwork's own parameters (M_net.*) get their gradient from an autograd
    pass of the module over the recorded mass cotangents, so the kernels leave those slots exactly zero."""
    return s["mass"] == "cartpole" or not key.startswith("M_net.")


# ----------------------------------------------------------------------------- seeded inputs
def batch(sid, s, nb=B, horizon=H):
    """Census-rule inputs at the shapes of these tests: x0 / x (nb,n), U (nb,H,m), u (nb,m), cotangents traj_bar
    (nb,H+1,n), dx_bar (nb,H,n), lam (nb,n), Hbar (nb,)."""
    rng = np.random.default_rng(vc.seed_of(sid + "/wgrad", s) + 1000 * nb + horizon)
    n, m = s["n"], s["m"]
    d = {"dt": vc.dt_of(s), "nb": nb, "H": horizon, "cost": vc.cost_of(s, rng)}
    d["x0"], d["U"] = vc.states(rng, n, nb), vc.controls(rng, nb, horizon, m)
    d["u"] = rng.uniform(vc.U_MIN, vc.U_MAX, size=(nb, m)).astype(np.float32)
    d["traj_bar"] = rng.normal(size=(nb, horizon + 1, n)).astype(np.float32)
    d["dx_bar"] = rng.normal(size=(nb, horizon, n)).astype(np.float32)
    d["lam"], d["Hbar"] = rng.normal(size=(nb, n)).astype(np.float32), rng.normal(size=nb).astype(np.float32)
    return d


COTANGENTS = ("traj_bar", "dx_bar", "lam", "Hbar")


def with_scales(d, sc):
    """A copy of the batch with the cotangents of row b times sc[b] (float32 (nb,), or one number for all rows)."""
    sc = np.broadcast_to(np.asarray(sc, np.float32), (d["nb"],))
    out = dict(d)
    for k in COTANGENTS:
        out[k] = het.scaled_rows(d[k], sc)
    return out


def with_zero_cotangents(d, rows=het.POISONED):
    sc = np.ones(d["nb"], np.float32)
    sc[[b for b in rows if b < d["nb"]]] = 0.0
    return with_scales(d, sc)


def replaced_rows(sid, s, d, rows=het.POISONED):
    """W4: the states and controls of `rows` replaced by other finite values (states x -0.5, fresh controls)."""
    rng = np.random.default_rng(vc.seed_of(sid + "/wgrad/replaced", s) + d["nb"])
    rows = [b for b in rows if b < d["nb"]]
    out = dict(d)
    out["x0"], out["U"], out["u"] = d["x0"].copy(), d["U"].copy(), d["u"].copy()
    out["x0"][rows] = d["x0"][rows] * np.float32(-0.5)
    out["U"][rows] = vc.controls(rng, len(rows), d["H"], s["m"])
    out["u"][rows] = rng.uniform(vc.U_MIN, vc.U_MAX, size=(len(rows), s["m"])).astype(np.float32)
    return out


def rows_of(d, rows):
    """The sub-batch `rows` of a batch."""
    out = dict(d)
    for k in ("x0", "U", "u") + COTANGENTS:
        if k in d:
            out[k] = np.ascontiguousarray(d[k][rows])
    out["nb"] = len(out["x0"])
    return out


def point_inputs(sid, s, N):
    """Point-mode inputs for the record-count cases (x, u, lam, Hbar), seeded per (spec, N)."""
    rng = np.random.default_rng(vc.seed_of(sid + "/wgrad/grid", s) + N)
    n, m = s["n"], s["m"]
    return {"nb": N, "x0": vc.states(rng, n, N), "u": rng.uniform(vc.U_MIN, vc.U_MAX, size=(N, m)).astype(np.float32),
            "lam": rng.normal(size=(N, n)).astype(np.float32), "Hbar": rng.normal(size=N).astype(np.float32)}


# ----------------------------------------------------------------------------- the oracle side
def oracle_point(model, d, use_hbar=True):
    """grad_theta blob of sum_p lam_p . f(x_p,u_p) [+ Hbar_p H(x_p)] on an OracleModel."""
    return model.wgrad(d["x0"], d["u"], d["lam"], d["Hbar"] if use_hbar else None)


def oracle_rollout(model, d, integ, traj_bar=True, dx_bar=True):
    """dict(grad_theta, grad_u, grad_x0, traj, dX) of the rollout's reverse pass on an OracleModel."""
    return model.rollout_wgrad(d["x0"], d["U"], integ, d["dt"], d["traj_bar"] if traj_bar else None,
                               d["dx_bar"] if dx_bar else None)


def groups_single(nb):
    return [np.array([b]) for b in range(nb)]


def groups_tiles(nb):
    return [np.arange(t, min(t + 16, nb)) for t in range(0, nb, 16)]


def superpose(fn, d, groups):
    """fn(sub-batch) -> float64 gradient blob.  -> (sum over the groups, sum of absolute values): the reference value
    and the scale of every entry, accumulated in float64 in the order of the groups."""
    total = scale = None
    for rows in groups:
        g = np.asarray(fn(rows_of(d, rows)), np.float64)
        if total is None:
            total, scale = g.copy(), np.abs(g)
        else:
            total += g
            scale += np.abs(g)
    return total, scale


def entry_metric(layout, ours, total, scale, keep=lambda key: True):
    """{tensor: (r_t, flat index of the worst entry)} of the blob `ours` against the superposition (total, scale).
    A tensor of scale zero must be exactly zero (r = 0, else inf); a non-finite entry gives inf."""
    ours = np.asarray(ours, np.float64).reshape(-1)
    assert ours.shape == total.shape == scale.shape
    out = {}
    for key, off, shape in layout:
        if not keep(key):
            continue
        cnt = int(np.prod(shape)) if len(shape) else 1
        o, t, sc = ours[off:off + cnt], total[off:off + cnt], scale[off:off + cnt]
        mx = float(sc.max()) if cnt else 0.0
        if mx == 0.0:
            bad = np.flatnonzero(o != 0)
            out[key] = (float("inf"), int(bad[0])) if len(bad) else (0.0, 0)
            continue
        with np.errstate(invalid="ignore"):
            r = np.abs(o - t) / (sc + FLOOR * mx)
        r = np.where(np.isfinite(o), r, np.inf)
        e = int(np.argmax(r))
        out[key] = (float(r[e]), e)
    return out


# (matmul mode, tensor family) -> factor where the measured excess over FACTOR is the precision of the product mode:
# 2 x the worst ratio measured on an MI355X over every case of tests/test_gpu_wgrad_structure.py (DESIGN 3.7 has the
# table and the reasons).  Only f16x2 needs any: every all-f32 variant is within 8 in every family (worst 7.4), and
# with the SAME weights and inputs the all-f32 kernels sit at <= 2.9 on H_net W1 where the f16x2 kernels sit at 12 .. 23:
# these sums take grad H, q1 = W2^T g2 and W2^T gdot2 from 22-bit products, whose error is relative to sum |w||g| while
# the entry itself may cancel.  The older criterion, 1e-4 of the tensor's largest entry (OLD_TOL, old_criterion), is
# asserted on the same blobs, so a raised factor never lets an entry be further off than it was allowed to be before.
FACTORS = {("f16x2", "H_net W1 bias"): 46.0,    # measured 22.8
           ("f16x2", "H_net W1 weight"): 17.0,  # 8.4
           ("f16x2", "R_net V2 weight"): 44.0,  # 21.7
           ("f16x2", "G_net V2 weight"): 41.0,  # 20.3
           ("f16x2", "R_diag_raw"): 20.0}       # 10.0
OLD_TOL = 1e-4


def factor_of(mode, key):
    return FACTORS.get((mode, family(key)), FACTOR)


def bounds(layout, oracle_metric, total, scale, mode=None):
    """{tensor: factor * max(r of the float32 oracle, 2^-22)} for the tensors of `oracle_metric`."""
    out = {}
    for key, off, shape in layout:
        if key in oracle_metric:
            r = oracle_metric[key][0]
            out[key] = factor_of(mode, key) * max(r, ORACLE_FLOOR) if np.isfinite(r) else float("nan")
    return out


def old_criterion(layout, ours, total, keep=lambda key: True):
    """{tensor: max|ours - ref| / max|ref|}, the older per-tensor figure (<= OLD_TOL), on the same blob and reference:
    it runs beside the entrywise bound, so no factor, raised or not, lets an entry be further off than it did."""
    ours = np.asarray(ours, np.float64).reshape(-1)
    out = {}
    for key, off, shape in layout:
        cnt = max(int(np.prod(shape)), 1)
        mx = float(np.abs(total[off:off + cnt]).max())
        if keep(key) and mx > 0:
            out[key] = float(np.abs(ours[off:off + cnt] - total[off:off + cnt]).max()) / mx
    return out


def layout_of(sd):
    return weights.blob_layout(sd)


def zero_tensors(layout, scale):
    """Tensors whose float64 gradient is identically zero."""
    return [k for k, off, shape in layout if not scale[off:off + max(int(np.prod(shape)), 1)].any()]


def family(key):
    """Tensor family a state_dict key reports under."""
    if key in ("J", "R_diag_raw"):
        return key
    net, _, rest = key.partition(".net.")
    if not rest:
        return key
    idx, what = rest.split(".")
    names = {"H_net": {"0": "W1", "2": "W2", "4": "W3"}, "R_net": {"0": "V1", "2": "V2"}, "G_net": {"0": "V1", "2": "V2"}}
    return f"{net} {names.get(net, {}).get(idx, idx)} {what}"
