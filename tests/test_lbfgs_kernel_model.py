"""The bit-exact float32 model of k_lbfgs (lbfgs_kernel_model.py), checked on the CPU.

  tree shape   dot() sums in the kernel's order: per-lane serial sums from 0.f over float4 lane + 16k, then the DPP
               butterfly as a pairwise tree over the 16 lanes; hand-built vectors where the serial sum, NumPy's pairwise
               sum and the kernel tree give three different floats; N = 65, 255 where the lane layout decides the bits,
               N = 64, 256 where the 0.f start does, N = 1, 3 where the padding does
  algorithm    kernel_schedule == lbfgs_schedule (which equals torch.optim.LBFGS bit for bit) for N in {1, 7, 20, 65,
               129, 256} x history {1, 2, 3, 100} with every break reason forced, and on the oracle engine's G13 MPC
               closure: counters exactly whenever no tolerance decided a break, iterates and costs to rounding
  batch        a problem alone == the same problem inside a mixed batch, bitwise

The GPU side (tests/test_gpu_lbfgs_kernel.py) asserts device == kernel_schedule bit for bit.
"""
import numpy as np
import pytest
import torch

import oracle_lib as ol
from phnn_mpc_amd import _capi
from lbfgs_kernel_model import LANES, abs_max, dot, kernel_e4, kernel_schedule, row_sum, to_lanes
from lbfgs_reference import lbfgs_schedule, tanh_quadratic

F32 = np.float32
TOLERANCE_BREAKS = {"opt_cond_start", "opt_cond", "small_step", "loss_change", "gtd"}
# L-BFGS amplifies rounding, and lbfgs_schedule rounds like torch (another dot order): iterates agree to U_TOL of their
# largest magnitude and costs to C_TOL of theirs, on the few iterations of every case below
U_TOL, C_TOL = 2e-5, 1e-5


def _dot_n(a, b):
    """model dot of two length-N float32 vectors (one problem)"""
    E4 = kernel_e4(len(a))
    return dot(to_lanes(np.asarray(a, F32)[None], E4), to_lanes(np.asarray(b, F32)[None], E4))[0]


def _bits(x):
    return np.asarray(x, F32).view(np.uint32)


def _serial(a):
    s = F32(a[0])
    for v in a[1:]:
        s = F32(s + F32(v))
    return s


def test_launch_picks_e4_like_lbfgs_launch():
    assert [kernel_e4(n) for n in (1, 64, 65, 128, 129, 192, 193, 256, 257)] == [1, 1, 2, 2, 3, 3, 4, 4, 0]


def test_tree_shape_differs_from_serial_and_numpy():
    # N = 64, one float4 per lane: lane l holds elements 4l .. 4l + 3.  Lane 0 sums to 2^24, lanes 1 .. 15 to 1.
    a = np.zeros(64, F32)
    a[0] = 2.0 ** 24
    a[4::4] = 1.0
    ones = np.ones(64, F32)
    serial = _serial(a)  # 2^24 + 1 rounds back to 2^24 (ties to even), fifteen times
    pairwise = np.sum(a, dtype=F32)  # eight interleaved accumulators: 2^24 + 7 ones -> 2^24, then + 8
    # tree: (2^24 + 1) -> 2^24, (1 + 1) = 2, ... -> [2^24, 2 x 7] -> [2^24 + 2, 4 x 3] -> [2^24 + 6, 8] -> 2^24 + 14
    tree = _dot_n(a, ones)
    assert float(serial) == 2.0 ** 24 and float(pairwise) == 2.0 ** 24 + 8
    assert float(tree) == 2.0 ** 24 + 14, float(tree) - 2.0 ** 24


def test_tree_levels_in_butterfly_order():
    # quad_perm [1,0,3,2] before [2,3,0,1]: lanes 2^24, 1, 0, 1 -> (2^24 + 1) + (0 + 1) = 2^24; the other order,
    # (2^24 + 0) + (1 + 1), would give 2^24 + 2
    v = np.zeros((1, LANES), F32)
    v[0, :4] = (2.0 ** 24, 1.0, 0.0, 1.0)
    assert float(row_sum(v)[0]) == 2.0 ** 24
    # row_half_mirror before row_mirror: quads 2^24, 1, 0, 1 -> (Q0 + Q1) + (Q2 + Q3) = 2^24, not (Q0 + Q2) + (Q1 + Q3)
    v = np.zeros((1, LANES), F32)
    v[0, 0], v[0, 4], v[0, 12] = 2.0 ** 24, 1.0, 1.0
    assert float(row_sum(v)[0]) == 2.0 ** 24
    # every lane 1 but lane 8 = 2^24: left half 8, right half (2^24 (+1 lost), 2, 2, 2) -> 2^24 + 6; total 2^24 + 14
    v = np.ones((1, LANES), F32)
    v[0, 8] = 2.0 ** 24
    assert float(row_sum(v)[0]) == 2.0 ** 24 + 14


@pytest.mark.parametrize("N", [64, 256])
def test_lane_sums_start_from_positive_zero(N):
    # every product is -0 and, at N = 64 and 256, every lane holds only real elements (no padding): a lane sum started
    # from its first product stays -0 (and so does the tree of them), the kernel's 0.f + -0 is +0
    a, b = -np.zeros(N, F32), np.ones(N, F32)
    assert _bits(_serial(a * b)) == 0x80000000
    assert _bits(_dot_n(a, b)) == 0


@pytest.mark.parametrize("N", [1, 3])
def test_padding_products_make_short_sums_positive_zero(N):
    # every real product is -0; the padded +0 products of the same lane and the 15 lanes holding only padding make the
    # kernel's result +0 whatever the lane sums start from
    a, b = -np.zeros(N, F32), np.ones(N, F32)
    assert _bits(_serial(a * b)) == 0x80000000
    assert _bits(_dot_n(a, b)) == 0


@pytest.mark.parametrize("N", [65, 255])
def test_padded_layout_puts_element_64_in_lane_0(N):
    # E4 >= 2: lane 0 holds elements 0 .. 3 and 64 .. 67, so elements 1 and 64 (the last one at N = 65, followed by
    # three zeros of padding) meet in lane 0 before 2^24 (lane 1) is added
    a = np.zeros(N, F32)
    a[1], a[64], a[4] = 1.0, 1.0, 2.0 ** 24
    ones = np.ones(N, F32)
    assert float(_serial(a)) == 2.0 ** 24  # 1 + 2^24 -> 2^24 (ties to even), + 1 -> 2^24
    assert float(_dot_n(a, ones)) == 2.0 ** 24 + 2  # lane 0 = 1 + 1 = 2, lane 1 = 2^24, 2 + 2^24 exact


@pytest.mark.parametrize("N", [1, 3, 65, 255])
def test_dot_matches_a_scalar_restatement(N):
    """Random vectors: the model's dot equals a plain scalar loop over lanes in the kernel's order."""
    rng = np.random.default_rng(N)
    a, b = rng.standard_normal(N).astype(F32), rng.standard_normal(N).astype(F32)
    E4 = kernel_e4(N)
    lane_sum = []
    for lane in range(LANES):
        s = F32(0.0)
        for k in range(E4):
            for c in range(4):
                e = 4 * (lane + LANES * k) + c
                s = F32(s + (F32(a[e] * b[e]) if e < N else F32(0.0)))
        lane_sum.append(s)
    while len(lane_sum) > 1:
        lane_sum = [F32(lane_sum[i] + lane_sum[i + 1]) for i in range(0, len(lane_sum), 2)]
    assert _bits(_dot_n(a, b)) == _bits(lane_sum[0])


def test_abs_max_propagates_nan_and_rounds_the_product():
    a = to_lanes(np.array([[1.0, -3.0, 2.0], [1.0, np.nan, 0.0]], F32), 1)
    m = abs_max(a, np.array([0.5, 1.0], F32))
    assert float(m[0]) == 1.5 and np.isnan(m[1])


def _init(init, B, N):
    g = torch.Generator().manual_seed(N)
    return torch.zeros(B, N) if init == "zeros" else torch.randn(B, N, generator=g)


# case -> (tanh_quadratic seed, initial iterate, options); the forced reason is asserted on both sides
CASES = {
    "default": (1, "zeros", dict(lr=1.0, outer_steps=2, max_iter=3)),
    "opt_cond_start": (2, "zeros", dict(lr=0.5, outer_steps=3, tolerance_grad=1e6)),
    "lack_of_progress": (3, "zeros", dict(lr=0.5, outer_steps=2, max_iter=5)),  # tolerance_change searched
    "max_eval": (4, "zeros", dict(lr=0.5, outer_steps=3, max_eval=4)),
    "gtd": (5, "randn", dict(lr=1.0, outer_steps=3, tolerance_change=1e4)),
    "max_iter": (6, "zeros", dict(lr=0.1, outer_steps=2, max_iter=4, tolerance_change=0.0, tolerance_grad=0.0)),
    "skip_update": (7, "zeros", dict(lr=1e-6, outer_steps=2, max_iter=4, tolerance_change=0.0)),
    "wrap": (8, "zeros", dict(lr=0.05, outer_steps=1, max_iter=12, tolerance_change=0.0, tolerance_grad=0.0)),
}


def _compare(a, b):
    """a: kernel_schedule, b: lbfgs_schedule."""
    scale = max(float(b["u_last"].abs().max()), 1e-30)
    du = float((a["u_last"] - b["u_last"]).abs().max())
    assert du <= U_TOL * scale, (du, scale)
    dc = float((a["costs"] - b["costs"]).abs().max())
    assert dc <= C_TOL * float(b["costs"].abs().max()), (dc, float(b["costs"].abs().max()))
    if not TOLERANCE_BREAKS & set(b["reasons"]):
        assert torch.equal(a["n_iter"], b["n_iter"]), (a["n_iter"], b["n_iter"])
        assert torch.equal(a["func_evals"], b["func_evals"]), (a["func_evals"], b["func_evals"])
        assert a["reasons"] == b["reasons"], (a["reasons"], b["reasons"])


@pytest.mark.parametrize("hs", [1, 2, 3, 100])
@pytest.mark.parametrize("N", [1, 7, 20, 65, 129, 256])
@pytest.mark.parametrize("case", list(CASES))
def test_same_algorithm_as_torch(case, N, hs):
    seed, init, kw = CASES[case]
    B = 4
    ev = tanh_quadratic(B, N, seed=seed)
    u0 = _init(init, B, N)
    kw = dict(kw, history_size=hs)
    if case == "lack_of_progress":  # the smallest tolerance_change that stops some step() on |d t| or the loss change
        for tc in (1e-3, 1e-2, 1e-1, 1.0):
            b = lbfgs_schedule(ev, u0, **kw, tolerance_change=tc)
            if b["reasons"]["small_step"] + b["reasons"]["loss_change"] > 0:
                break
        kw["tolerance_change"] = tc
    a = kernel_schedule(ev, u0, **kw)
    b = lbfgs_schedule(ev, u0, **kw)
    _compare(a, b)
    for r in (a["reasons"], b["reasons"]):
        if case == "lack_of_progress":
            assert r["small_step"] + r["loss_change"] > 0, r
        elif case == "wrap":
            assert r["push"] == 11 * B, r
        elif case != "default":
            assert r[case] > 0, r
    if case in ("opt_cond_start", "gtd"):  # decided by six orders of magnitude: the counters agree as well
        assert torch.equal(a["n_iter"], b["n_iter"]) and a["reasons"] == b["reasons"]
    if case == "wrap" and hs < 11:
        assert int(a["pushes"].min()) > hs


def test_loss_change_is_taken_in_double():
    """|loss - prev_loss| < tolerance_change in double, not float32: the cost rises by one float32 ulp (2^-30 at 2^-7)
    per evaluation and tolerance_change is a hair above 2^-30, which rounds to 2^-30 in float32.  In double every step()
    breaks on the loss change at its first re-evaluation; a float32 comparison (2^-30 < 2^-30) would never break."""
    B, N = 2, 5
    calls = [0]

    def ev(u, rows):
        c = torch.full((u.shape[0],), 2.0 ** -7 + calls[0] * 2.0 ** -30)
        calls[0] += 1
        return c, torch.ones_like(u)

    kw = dict(lr=1.0, outer_steps=2, max_iter=4, tolerance_change=2.0 ** -30 * (1 + 1e-9))
    assert float(np.float32(kw["tolerance_change"])) == 2.0 ** -30
    a = kernel_schedule(ev, torch.zeros(B, N), **kw)
    calls[0] = 0
    b = lbfgs_schedule(ev, torch.zeros(B, N), **kw)
    assert a["reasons"] == b["reasons"] and a["reasons"]["loss_change"] == 2 * B, (a["reasons"], b["reasons"])
    assert torch.equal(a["n_iter"], b["n_iter"]) and torch.equal(a["func_evals"], b["func_evals"])


@pytest.mark.parametrize("hs", [1, 2, 3, 100])
def test_oracle_engine_cost_g13(hs):
    """The MPC closure of the G13 controller (H = 20, lr = 0.5) on the CPU oracle, per problem."""
    from oracle_engine import OracleEngine
    eng = OracleEngine(ol.load_weights("phnn_cartpole"))
    cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], 0.01, [0.0] * 4, -15.0, 15.0)
    rng = np.random.default_rng(0)
    B, H = 3, 20
    x0 = torch.tensor((rng.uniform(-1, 1, size=(B, 4)) * np.array([0.5, 0.1, 0.3, 0.3])).astype(np.float32))

    def ev(u, rows):
        c, g = torch.empty(u.shape[0]), torch.empty_like(u)
        for j, b in enumerate(rows):
            cj, gj = eng.rollout_cost_grad(x0[b:b + 1], u[j].reshape(1, H, 1), cost, "euler", 0.02)
            c[j], g[j] = cj[0], gj.reshape(-1)
        return c, g

    kw = dict(lr=0.5, outer_steps=2, max_iter=4, history_size=hs)
    a = kernel_schedule(ev, torch.zeros(B, H), **kw)
    _compare(a, lbfgs_schedule(ev, torch.zeros(B, H), **kw))
    assert a["reasons"]["push"] > 0


@pytest.mark.parametrize("rows", [[0], [5], [3, 1, 6]])
def test_model_does_not_depend_on_batch(rows):
    # problems of very different curvature take different paths through the masks of the batched model
    B, N = 8, 13
    parts = [tanh_quadratic(B, N, seed=9, scale=s) for s in (0.05, 1.0, 20.0)]

    def ev_full(u, rr):
        c, g = torch.empty(u.shape[0]), torch.empty_like(u)
        for j, b in enumerate(rr):
            cj, gj = parts[b % 3](u[j:j + 1], [b])
            c[j], g[j] = cj[0], gj[0]
        return c, g

    kw = dict(lr=1.0, outer_steps=3, max_iter=10, tolerance_change=1e-5, history_size=3)
    u0 = _init("randn", B, N)
    full = kernel_schedule(ev_full, u0, **kw)
    assert len(set(full["n_iter"].tolist())) > 1 and len(set(full["reasons"]) - {"push"}) > 1, full["reasons"]
    part = kernel_schedule(lambda u, r: ev_full(u, [rows[i] for i in r]), u0[rows], **kw)
    for k in ("u_last", "n_iter", "func_evals", "pushes"):
        assert torch.equal(part[k], full[k][rows]), k
    assert torch.equal(part["costs"], full["costs"][:, rows])
