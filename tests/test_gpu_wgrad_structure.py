"""The weight-gradient kernels entry by entry and at mixed scales: the record-emitting adjoint
(k_rollout_grad<..., WG=true>, k_model_vjp<..., true>), k_wgrad_reduce and k_wgrad_finish through model_wgrad,
rollout_wgrad and rollout_trajectory(tapes=True).  Inputs, metric and bound: tests/wgrad_checks.py; the same checks on
the float32 oracle: tests/test_wgrad_model.py (so W2 and W4 belong to the arithmetic, and a kernel that lacks one has a
defect).  The older criterion (every tensor within 1e-4 of its largest entry, tests/test_gpu_wgrad.py and the census)
keeps running beside this one.

W1  Entrywise accuracy against the float64 superposition sum_c contrib_c, every tensor within
    8 x max(float32 oracle on the same inputs, 2^-22) of r_t = max_e |ours - ref| / (scale_e + 2^-7 max scale):
    every wgrad spec in point mode (N = 37 and 1, with and without Hbar) and as an Euler rollout (37, 6); the families
    also RK4, on K1's tapes, with traj_bar or dx_bar alone, and at (B, H) = (1, 1) and (5, 3).
W2  Uniform 2^k homogeneity, bit for bit, k = -40, -13, 13, 40: grad_theta, grad_u / grad_x0 and xbar / ubar are 2^k
    times the k = 0 results as uint32; all cotangents exactly 0 give 0 everywhere.
W3  Scales 2^-40 .. 2^40 mixed inside every tile, two rollouts scaled by 0: grad_u / grad_x0 / xbar / ubar rows are
    bitwise 2^k_b x base, grad_theta is finite and within the W1 bound of sum_b 2^k_b contrib_b.
W4  Rollouts or points {0, 9, 15, 16, 36} with cotangent 0: replacing their states and controls by other finite values
    changes no value of grad_theta and no bit of the other rows.
W5  The record-emitting adjoint keeps rollouts isolated: a NaN / inf / 1e30 state or a NaN control in those rollouts
    leaves every traj, dX, grad_u, grad_x0, xbar, ubar row of the others unchanged as uint32 (grad_theta is not
    asserted: the sum is non-finite by definition).
W6  The shared workspace's earlier contents do not matter: after a (300, 16) call has grown it, every byte 0xFF or
    every byte 0 before a call gives the same bits; grad_theta pre-filled with NaN comes back finite without
    `accumulate`; the mass=full records carry exactly 0 beyond B.
W7  Record counts around the grid of the reduce (wgrad_rows = min(n_rec, n_cu), two exchange buffers): 1, 2, n_cu - 1,
    n_cu, n_cu + 1, 2 n_cu, 2 n_cu + 1, 3 n_cu + 2 records in point mode and n_cu + 3 or so on the tape-reading reduce;
    metric and bound as in W1, every call bitwise repeatable.

The non-finite values and the 0xFF fill are data in correctly sized buffers: no size, pointer or stride depends on them.

Measured on an MI355X, worst ratio of r_t to the float32 oracle's max(r_t, 2^-22) on the same inputs over every case
of this file, per tensor family (the bound is the factor: 8 unless stated; DESIGN 3.7 has the full table):
  all-f32 kernels (64- and 128-wide): every family <= 7.4 (H_net W2 bias 7.4, R_diag_raw 6.3, R_net V2 weight 5.9,
      H_net W2 weight 3.8, J 2.3 after the fix below; 24.6 before it)
  f16x2 kernels, factor 8: J 6.8, R_net V2 bias 5.9, R_net V1 4.7, H_net W2 bias 4.2, G_net V1 3.8, H_net W3 weight 3.3,
      H_net W2 weight 2.8
  f16x2 kernels, measured factor (wgrad_checks.FACTORS = 2 x these): H_net W1 bias 22.8 (r 1.4e-5; largest r 1.4e-4 at
      N = 1), R_net V2 weight 21.7, G_net V2 weight 20.3, R_diag_raw 10.0, H_net W1 weight 8.4
W2, W3's bitwise part, W4, W5, W6's bitwise part and the repeatability of W7 held on the first run.  W1 found one defect:
the diagonal of Jbar (test_j_gradient_is_antisymmetric_bit_for_bit).
"""
import numpy as np
import pytest

import heterogeneous as het
import oracle_lib as ol
import variant_census as vc
import wgrad_checks as wc
from test_gpu_heterogeneous import Bits, f32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def n_cu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


_CTX = {}


class Ctx:
    """Engine, oracles and layout of one spec (kept for the module: the tests of a spec share them)."""

    def __init__(self, sid):
        from phnn_mpc_amd.engine import RolloutEngine
        self.sid, (self.variant, self.s) = sid, vc.ALL_SPECS[sid]
        self.sd = vc.build_state_dict(sid, self.s)
        self.eng = RolloutEngine(self.sd, "cuda:0", **vc.engine_kwargs(self.s))
        assert self.eng.variant == self.variant and self.eng.has_wgrad
        self.m32, self.m64 = (ol.OracleModel(self.sd, p, activation=self.s["act"]) for p in ("f32", "f64"))
        self.lay = wc.layout_of(self.sd)
        self.mode = het.mode_of(self.variant)
        self.refs = {}


def ctx(sid):
    if sid not in _CTX:
        _CTX[sid] = Ctx(sid)
    return _CTX[sid]


# ----------------------------------------------------------------------------- the device side
def dev_point(c, d, use_hbar=True, grad_theta=None):
    g, xb, ub = c.eng.model_wgrad(d["x0"], d["u"], d["lam"], d["Hbar"] if use_hbar else None, grad_theta=grad_theta)
    return {"grad_theta": f32(g), "xbar": f32(xb), "ubar": f32(ub)}


def dev_rollout(c, d, integ, tapes, traj_bar=True, dx_bar=True, grad_theta=None, before_forward=None):
    eng = c.eng
    if before_forward is not None:
        before_forward()
    traj, dX = eng.rollout_trajectory(d["x0"], d["U"], integ, d["dt"], want_dx=True, tapes=tapes)
    tok = eng.tape_token if tapes else None
    assert (tok is not None) == tapes
    g, gu, gx = eng.rollout_wgrad(d["x0"], d["U"], traj, integ, d["dt"], traj_bar=d["traj_bar"] if traj_bar else None,
                                  dx_bar=d["dx_bar"] if dx_bar else None, grad_theta=grad_theta, tape_token=tok)
    return {"grad_theta": f32(g), "grad_u": f32(gu), "grad_x0": f32(gx), "traj": f32(traj), "dX": f32(dX)}


POINT_CASE = lambda use_hbar: (lambda m, r: wc.oracle_point(m, r, use_hbar))
ROLL_CASE = lambda integ, tb=True, db=True: (lambda m, r: wc.oracle_rollout(m, r, integ, tb, db)["grad_theta"])


def reference(c, key, fn, d, groups):
    """(total, scale, float32-oracle metric, bound per tensor) of one case, computed once per (spec, case)."""
    if key not in c.refs:
        tot, sc = wc.superpose(lambda r: fn(c.m64, r), d, groups)
        m32 = wc.entry_metric(c.lay, fn(c.m32, d), tot, sc)
        c.refs[key] = (tot, sc, m32, wc.bounds(c.lay, m32, tot, sc, c.mode))
    return c.refs[key]


def check_theta(rep, c, what, blob, ref):
    """W1's assertion on one gradient blob; prints the worst tensor of the call (every figure before the assert)."""
    tot, sc, m32, bound = ref
    met = wc.entry_metric(c.lay, blob, tot, sc, keep=lambda k: wc.owned(c.s, k))
    worst = (0.0, "")
    for k, (r, e) in met.items():
        rep.le(f"{what} {k}[{e}]", r, bound[k])
        if bound[k] > 0:
            ratio = r / max(m32[k][0], wc.ORACLE_FLOOR)
            fam = (c.mode, wc.family(k))
            if ratio > rep.worst.get(fam, (0.0, 0.0))[1]:
                rep.worst[fam] = (r, ratio, what)
            if ratio > worst[0]:
                worst = (ratio, f"{k}[{e}] r {r:.2e} = {ratio:.2f} x oracle32 (factor {wc.factor_of(c.mode, k):g})")
    print(f"WGM {c.sid} [{c.mode}] {what}: {worst[1]}")
    for k, e in wc.old_criterion(c.lay, blob, tot, keep=lambda k: wc.owned(c.s, k)).items():
        rep.le(f"{what} {k}: the older criterion, of max|ref|", e, wc.OLD_TOL)
    for k, off, shape in c.lay:  # the mass network's own slots stay exactly zero (its gradient comes from autograd)
        if not wc.owned(c.s, k):
            rep.true(f"{what} {k} left at zero", not blob[off:off + int(np.prod(shape))].any())


class Rep(Bits):
    def __init__(self, sid):
        super().__init__(sid)
        self.worst = {}

    def finish(self):
        for (mode, fam), (r, ratio, what) in sorted(self.worst.items()):
            print(f"WGFAM {self.sid} [{mode}] {fam}: r {r:.2e} ratio {ratio:.2f} ({what})")
        super().finish()


def scaled(a, k):
    return (np.asarray(a, np.float32) * np.float32(np.ldexp(1.0, k))).astype(np.float32)


# ----------------------------------------------------------------------------- W1
@pytest.mark.parametrize("sid", wc.WG_SPECS)
def test_w1_entrywise_accuracy(torch, sid):
    c, rep = ctx(sid), Rep(sid)
    d, d1 = wc.batch(sid, c.s), wc.batch(sid, c.s, 1, 1)
    for dd, tag in ((d, "N37"), (d1, "N1")):
        for hb in (True, False):
            key = f"point {tag} Hbar={hb}"
            out = dev_point(c, dd, hb)
            check_theta(rep, c, key, out["grad_theta"], reference(c, key, POINT_CASE(hb), dd, wc.groups_single(dd["nb"])))
    fam = sid in wc.WG_FAMILIES
    for integ in het.INTEGRATORS if fam else ("euler",):
        ref = reference(c, f"roll B37 H6 {integ}", ROLL_CASE(integ), d, wc.groups_single(d["nb"]))
        for tapes in (False, True) if fam else (False,):
            out = dev_rollout(c, d, integ, tapes)
            check_theta(rep, c, f"roll B37 H6 {integ} tapes={tapes}", out["grad_theta"], ref)
    if fam:
        for tb, db in ((True, False), (False, True)):
            key = f"roll B37 H6 euler traj_bar={tb} dx_bar={db}"
            ref = reference(c, key, ROLL_CASE("euler", tb, db), d, wc.groups_single(d["nb"]))
            for tapes in (False, True):
                out = dev_rollout(c, d, "euler", tapes, traj_bar=tb, dx_bar=db)
                check_theta(rep, c, f"{key} tapes={tapes}", out["grad_theta"], ref)
        for nb, hz in wc.SMALL_SHAPES:
            ds = wc.batch(sid, c.s, nb, hz)
            for integ in het.INTEGRATORS:
                key = f"roll B{nb} H{hz} {integ}"
                ref = reference(c, key, ROLL_CASE(integ), ds, wc.groups_single(nb))
                for tapes in (False, True):
                    check_theta(rep, c, f"{key} tapes={tapes}", dev_rollout(c, ds, integ, tapes)["grad_theta"], ref)
    torch.cuda.synchronize()
    rep.finish()


@pytest.mark.parametrize("sid", [sid for sid in wc.WG_FAMILIES if wc.spec(sid)["kind"] == "phnn"])
def test_j_gradient_is_antisymmetric_bit_for_bit(torch, sid):
    """Jbar = sum lam dH^T - dH lam^T: its diagonal is exactly 0 and Jbar[j][q] == -Jbar[q][j] as uint32, as in the
    reference.  (k_wgrad_reduce used to fuse the two products into its accumulator, a + l h - l h, which left the
    rounding of a - l h on the diagonal: 1.7e-7 of the largest entry where the true gradient is 0, 25 x the float32
    oracle's figure under the entrywise metric at N = 1.)"""
    c, rep = ctx(sid), Rep(sid)
    n = c.s["n"]
    off = next(o for k, o, _ in c.lay if k == "J")
    runs = {"point N37": dev_point(c, wc.batch(sid, c.s)), "point N1": dev_point(c, wc.batch(sid, c.s, 1, 1))}
    for integ in het.INTEGRATORS:
        for tapes in (False, True):
            runs[f"{integ} tapes={tapes}"] = dev_rollout(c, wc.batch(sid, c.s), integ, tapes)
    for name, o in runs.items():
        J = o["grad_theta"][off:off + n * n].reshape(n, n)
        rep.true(f"{name}: Jbar is not zero", bool(np.abs(J).max() > 0))
        rep.true(f"{name}: the diagonal of Jbar is exactly 0: {np.diag(J)}", not np.diag(J).any())
        od = ~np.eye(n, dtype=bool)
        rep.same(f"{name}: Jbar^T == -Jbar off the diagonal", J.T[od].reshape(1, -1), (-J)[od].reshape(1, -1))
    rep.finish()


# ----------------------------------------------------------------------------- W2
def _all_modes(c, d):
    """{name: outputs} of every way the weight gradient is reached: point mode, rollouts recomputed and on tapes."""
    out = {"point": dev_point(c, d)}
    for integ in het.INTEGRATORS:
        for tapes in (False, True):
            out[f"{integ} tapes={tapes}"] = dev_rollout(c, d, integ, tapes)
    return out


GRAD_KEYS = ("grad_theta", "grad_u", "grad_x0", "xbar", "ubar")


@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_w2_uniform_power_of_two_homogeneity(torch, sid):
    c, rep = ctx(sid), Rep(sid)
    d = wc.batch(sid, c.s)
    base = _all_modes(c, d)
    for name, o in base.items():
        rep.true(f"{name}: the unscaled results are finite and not zero",
                 all(np.isfinite(o[q]).all() and np.abs(o[q]).max() > 0 for q in GRAD_KEYS if q in o))
    for k in wc.EXPONENTS:
        got = _all_modes(c, wc.with_scales(d, np.float32(np.ldexp(1.0, k))))
        for name, o in got.items():
            for q in GRAD_KEYS:
                if q in o:
                    rep.same(f"k={k} {name} {q}", o[q].reshape(1, -1), scaled(base[name][q], k).reshape(1, -1))
            for q in ("traj", "dX"):
                if q in o:
                    rep.same(f"k={k} {name} {q}", o[q], base[name][q])
    for name, o in _all_modes(c, wc.with_scales(d, np.float32(0.0))).items():
        for q in GRAD_KEYS:
            if q in o:
                rep.true(f"zero cotangents {name} {q}: every entry 0", bool((o[q] == 0).all()))
    torch.cuda.synchronize()
    rep.finish()


# ----------------------------------------------------------------------------- W3
@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_w3_mixed_scales_inside_a_tile(torch, sid):
    c, rep = ctx(sid), Rep(sid)
    d = wc.batch(sid, c.s)
    sc = het.row_scales(d["nb"])
    dm = wc.with_scales(d, sc)
    base, got = _all_modes(c, d), _all_modes(c, dm)
    for name, o in got.items():
        for q in GRAD_KEYS[1:]:
            if q in o:
                rep.homogeneous(f"{name} {q}", o[q], base[name][q], sc)
        rep.true(f"{name} grad_theta finite", bool(np.isfinite(o["grad_theta"]).all()))
        if name == "point":
            ref = reference(c, "mixed point", POINT_CASE(True), dm, wc.groups_single(d["nb"]))
        else:
            integ = name.split(" ")[0]
            ref = reference(c, f"mixed {integ}", ROLL_CASE(integ), dm, wc.groups_single(d["nb"]))
        check_theta(rep, c, f"mixed scales {name}", o["grad_theta"], ref)
    torch.cuda.synchronize()
    rep.finish()


# ----------------------------------------------------------------------------- W4
@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_w4_zero_cotangent_rows_do_not_enter(torch, sid):
    c, rep = ctx(sid), Rep(sid)
    d = wc.with_zero_cotangents(wc.batch(sid, c.s))
    e = wc.replaced_rows(sid, c.s, d)
    keep = het.others(d["nb"])
    a, b = _all_modes(c, d), _all_modes(c, e)
    for name in a:
        rep.true(f"{name} grad_theta: equal values (np.array_equal)",
                 bool(np.array_equal(a[name]["grad_theta"], b[name]["grad_theta"])))
        rep.true(f"{name} grad_theta finite, not zero",
                 bool(np.isfinite(a[name]["grad_theta"]).all() and np.abs(a[name]["grad_theta"]).max() > 0))
        for q in GRAD_KEYS[1:]:
            if q in a[name]:
                rep.same(f"{name} {q} of the other rows", b[name][q], a[name][q], rows=keep)
    torch.cuda.synchronize()
    rep.finish()


# ----------------------------------------------------------------------------- W5
@pytest.mark.parametrize("kind", wc.ISOLATION_KINDS)
@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_w5_record_emitting_adjoint_isolates_rollouts(torch, sid, kind):
    c, rep = ctx(sid), Rep(f"{sid} {kind}")
    d = wc.batch(sid, c.s)
    keep = het.others(d["nb"])
    p = dict(d)
    p["x0"], p["U"], _ = het.poison_rollout(kind, d["x0"], d["U"], d["cost"])
    _, p["u"] = het.poison_point(kind, d["x0"], d["u"])
    clean, dirty = _all_modes(c, d), _all_modes(c, p)
    for name, o in clean.items():
        for q in GRAD_KEYS[1:] + ("traj", "dX"):
            if q in o:
                rep.same(f"{name} {q}", dirty[name][q], o[q], rows=keep)
                rep.true(f"{name} {q}: the clean run is finite", bool(np.isfinite(o[q]).all()))
    bad = ~np.isfinite(c.m64.rollout_wgrad(p["x0"], p["U"], "euler", d["dt"], d["traj_bar"], d["dx_bar"])["grad_u"]
                       ).reshape(d["nb"], -1).all(axis=1)
    rep.true("the float64 oracle is finite on the other rollouts", not bad[keep].any())
    rep.true("grad_u is not finite where the float64 oracle's is not",
             not np.isfinite(dirty["euler tapes=False"]["grad_u"].reshape(d["nb"], -1)[bad]).all(axis=1).any())
    torch.cuda.synchronize()
    rep.finish()


# ----------------------------------------------------------------------------- W6
FILL_SHAPES = ((5, 3), (17, 2), (37, 6))


def _filled_runs(c, torch, byte):
    """Every call of W6 with the whole workspace set to `byte` before it (tape mode: before the forward, never
    between forward and backward) and grad_theta pre-filled with NaN."""
    eng, sid, s = c.eng, c.sid, c.s
    ws = eng.wgrad_workspace
    size = ws.numel()
    P = eng.blob.size

    def fill():
        assert eng.wgrad_workspace is ws and ws.numel() == size  # the pre-grown buffer is reused, not replaced
        ws.fill_(byte)

    def nan_theta():
        return torch.full((P,), float("nan"), dtype=torch.float32, device=eng.device)

    out = {}
    for nb, hz in FILL_SHAPES:
        d = wc.batch(sid, s, nb, hz)
        for integ in het.INTEGRATORS:
            fill()
            out[f"B{nb} H{hz} {integ} recompute"] = dev_rollout(c, d, integ, False, grad_theta=nan_theta())
            if s["mass"] == "full" and integ == "euler":
                q, mbar = eng.mass_cotangents(nb, hz, integ)
                # records are tile-major, then step: rows of the last tile beyond the batch
                pts = f32(torch.cat([q, mbar.reshape(-1, 4)], dim=1)).reshape(-(-nb // 16), hz, 16, 6)
                out[f"B{nb} H{hz} mass cotangents beyond B"] = {"beyond": pts[-1, :, nb - 16 * (-(-nb // 16) - 1):, 2:]}
            out[f"B{nb} H{hz} {integ} tapes"] = dev_rollout(c, d, integ, True, grad_theta=nan_theta(), before_forward=fill)
    fill()
    out["point N5"] = dev_point(c, wc.batch(sid, s, 5, 1), grad_theta=nan_theta())
    return out


@pytest.mark.parametrize("sid", wc.WG_FAMILIES)
def test_w6_workspace_contents_do_not_matter(torch, sid):
    c, rep = ctx(sid), Rep(sid)
    big = wc.batch(sid, c.s, 300, 16)
    for integ in het.INTEGRATORS:  # grow the engine's workspace once, to the largest shape
        dev_rollout(c, big, integ, True)
    ff, zero = _filled_runs(c, torch, 0xFF), _filled_runs(c, torch, 0x00)
    assert ff.keys() == zero.keys()
    for name in ff:
        for q, a in ff[name].items():
            if q == "beyond":
                rep.true(f"{name}: exactly 0 after the 0xFF fill", bool(a.size > 0 and (a == 0).all()))
                continue
            rep.same(f"{name} {q}: 0xFF fill against zero fill", a.reshape(1, -1), zero[name][q].reshape(1, -1))
            rep.true(f"{name} {q}: finite after the 0xFF fill", bool(np.isfinite(a).all()))
    # and against the float64 superposition, so that two equally wrong runs do not pass
    d = wc.batch(sid, c.s)
    ref = reference(c, "roll B37 H6 euler", ROLL_CASE("euler"), d, wc.groups_single(d["nb"]))
    for mode in ("recompute", "tapes"):
        check_theta(rep, c, f"0xFF fill B37 H6 euler {mode}", ff[f"B37 H6 euler {mode}"]["grad_theta"], ref)
    torch.cuda.synchronize()
    rep.finish()


# ----------------------------------------------------------------------------- W7
@pytest.mark.parametrize("which", range(8))
@pytest.mark.parametrize("sid", wc.GRID_SPECS)
def test_w7_record_counts_around_the_reduce_grid(torch, n_cu, sid, which):
    c, rep = ctx(sid), Rep(sid)
    tiles = wc.grid_tiles(n_cu)[which]
    N = wc.grid_points(tiles)
    d = wc.point_inputs(sid, c.s, N)
    a, b = dev_point(c, d), dev_point(c, d)
    for q in a:
        rep.same(f"tiles={tiles} {q}: bitwise repeatable", a[q].reshape(1, -1), b[q].reshape(1, -1))
    ref = reference(c, f"grid tiles={tiles}", POINT_CASE(True), d, wc.groups_tiles(N))
    check_theta(rep, c, f"grid tiles={tiles} ({-(-tiles // min(tiles, n_cu))} records per workgroup at most)",
                a["grad_theta"], ref)
    torch.cuda.synchronize()
    rep.finish()


@pytest.mark.parametrize("sid", wc.GRID_SPECS)
def test_w7_tape_reading_reduce_past_the_grid(torch, n_cu, sid):
    """3 tiles x (n_cu // 3 + 1) Euler steps: more records than workgroups on reduce_t, which reads a2 / q1 from
    K1's tapes."""
    c, rep = ctx(sid), Rep(sid)
    hz = n_cu // 3 + 1
    d = wc.batch(sid, c.s, wc.B, hz)
    assert 3 * hz > n_cu
    a, b = dev_rollout(c, d, "euler", True), dev_rollout(c, d, "euler", True)
    for q in a:
        rep.same(f"H={hz} {q}: bitwise repeatable", a[q].reshape(1, -1), b[q].reshape(1, -1))
    ref = reference(c, f"grid roll H={hz}", ROLL_CASE("euler"), d, wc.groups_single(d["nb"]))
    check_theta(rep, c, f"grid roll B37 H={hz} euler tapes", a["grad_theta"], ref)
    torch.cuda.synchronize()
    rep.finish()
