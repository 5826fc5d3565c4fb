"""Every kernel variant of the census (tests/variant_census.py) against the float64 oracle, on seeded default-init
weights: selection, point operations, rollouts with cost and gradients, the general reverse pass, weight gradients,
split-tile equality and launch-geometry invariance.

Stated tolerances (tests/test_gpu_parity.py): cost rtol 1e-5; trajectory rtol 1e-5 + atol 1e-5; grad_u / grad_x0
<= 1e-4 max|grad| per rollout; f(x,u), VJP <= 2e-5 max|.|; parameter gradients <= 1e-4 of each tensor's largest entry
(tests/test_gpu_wgrad.py); ReLU gradients 2e-3 (one unit's mask may flip, tests/test_gpu_activations.py).  A variant's
census `tol` multiplies all of them.  Every check of a variant is measured and reported before the test asserts, so
one run shows where each variant stands."""
import numpy as np
import pytest

import oracle_lib as ol
import variant_census as vc

pytestmark = pytest.mark.gpu
NTHREADS = 8


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


@pytest.fixture(scope="module")
def n_cu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def npy(t):
    return t.detach().cpu().numpy().astype(np.float64)


class Report:
    """Collects (check, error, bound) and bitwise properties of one variant; asserts them all at the end."""

    def __init__(self, sid):
        self.sid, self.rows, self.bad = sid, [], []

    def le(self, what, err, bound):
        self.rows.append((what, err, bound))
        if not err <= bound:
            self.bad.append(f"{what}: {err:.3g} > {bound:.3g}")

    def eq(self, what, a, b):
        same = a.shape == b.shape and bool((a == b).all())
        self.rows.append((what, 0.0 if same else 1.0, 0.0))
        if not same:
            d = float((a.double() - b.double()).abs().max()) if a.shape == b.shape else float("nan")
            self.bad.append(f"{what}: not bitwise equal (max diff {d:.3g})")

    def finish(self, digits=2):
        worst = {}
        for what, err, bound in self.rows:
            k = what.split(" ")[0]
            if bound > 0:
                worst[k] = max(worst.get(k, 0.0), err / bound)
        print(f"\n{self.sid}: " + ", ".join(f"{k} {v:.{digits}f}" for k, v in worst.items()) + " (worst error / bound)")
        assert not self.bad, (self.sid, self.bad)


def _engine(sd, s, **kw):
    from phnn_mpc_amd.engine import RolloutEngine
    return RolloutEngine(sd, "cuda:0", **vc.engine_kwargs(s), **kw)


def _check_points(rep, eng, m64, s, d, tag):
    dx, H = eng.forward(d["x"], d["u"])
    rdx, rH = m64.forward(d["x"], d["u"])
    rep.le(f"point f {tag}", vc.err_max(npy(dx), rdx), vc.POINT_TOL * s["tol"])
    rep.le(f"point H {tag}", float(np.abs(npy(H) - rH).max() / max(1.0, np.abs(rH).max())), vc.POINT_TOL * s["tol"])
    xb, ub = eng.vjp(d["x"], d["u"], d["lam"])
    rxb, rub = m64.vjp(d["x"], d["u"], d["lam"])
    vt = (vc.POINT_TOL * s["tol"]) if s["act"] != "relu" else vc.grad_tol(s)
    rep.le(f"point vjp_x {tag}", vc.err_max(npy(xb), rxb), vt)
    rep.le(f"point vjp_u {tag}", vc.err_max(npy(ub), rub), vt)


def _check_rollouts(rep, eng, m64, s, d):
    gt = vc.grad_tol(s)
    for integ in ("euler", "rk4"):
        for B, H in vc.ROLL_SHAPES:
            x0, U = d[(B, H)]
            for ck in ("cost", "cost_barrier") if (B, H) == vc.BARRIER_SHAPE else ("cost",):
                cost = d[ck]
                ref = m64.rollout(x0, U, cost, integ, d["dt"], nthreads=NTHREADS)
                tag = f"{integ} B{B} H{H} {ck}"
                _, tr = eng.rollout_cost(x0, U, cost, integ, d["dt"], want_traj=True)
                rep.le(f"traj {tag}", vc.err_traj(npy(tr), ref["traj"]), s["tol"])
                for stash in (True, False):
                    eng.use_stash = stash
                    try:
                        c, gu, gx = eng.rollout_cost_grad(x0, U, cost, integ, d["dt"], want_grad_x0=True)
                        c, gu, gx = npy(c), npy(gu), npy(gx)
                    finally:
                        eng.use_stash = True
                    t2 = f"{tag} stash={stash}"
                    rep.le(f"cost {t2}", vc.err_cost(c, ref["cost"]), vc.COST_RTOL * s["tol"])
                    rep.le(f"grad_u {t2}", vc.err_rows(gu, ref["grad_u"]), gt)
                    rep.le(f"grad_x0 {t2}", vc.err_rows(gx, ref["grad_x0"]), gt)
                    outside = (U < vc.U_MIN) | (U > vc.U_MAX)
                    rep.le(f"clamp_outside {t2}", float(np.abs(gu[outside]).max()) if outside.any() else 0.0, 0.0)
                    on = (U == vc.U_MIN) | (U == vc.U_MAX)
                    if on.any():  # the mask is inclusive (torch.clamp): on-bound entries carry the oracle's gradient
                        gmax = np.abs(ref["grad_u"]).max(axis=(1, 2), keepdims=True)
                        e = np.abs(gu - ref["grad_u"]) / np.where(gmax > 0, gmax, 1.0)
                        rep.le(f"clamp_on_bound {t2}", float(e[on].max()), gt)
        # the general reverse pass: trajectory cotangents alone (no cost) and with cost cotangents
        x0, U = d[(37, 13)]
        _, tr = eng.rollout_cost(x0, U, d["cost"], integ, d["dt"], want_traj=True)
        for cb in (None, d["cost_bar"]):
            rgu, rgx = m64.rollout_vjp(x0, U, d["cost"], integ, d["dt"], traj_bar=d["traj_bar"], cost_bar=cb)
            gu, gx = eng.rollout_vjp(x0, U, tr, d["cost"], integ, d["dt"], traj_bar=d["traj_bar"], cost_bar=cb)
            tag = f"{integ} cost_bar={cb is not None}"
            rep.le(f"rollout_vjp_u {tag}", vc.err_rows(npy(gu), rgu), gt)
            rep.le(f"rollout_vjp_x0 {tag}", vc.err_rows(npy(gx), rgx), gt)


def _check_wgrad(rep, eng, m64, s, d, sd, torch):
    from phnn_mpc_amd import weights
    lay = weights.blob_layout(sd)
    wt = vc.WGRAD_TOL * s["tol"]

    def named(blob):
        """Parameter tensors the kernels own.  A MassMatrixNetwork's own parameters (M_net.*) get their gradient from
        an autograd pass of the module over the recorded mass cotangents (models.py), so the kernels leave them zero."""
        t = weights.unpack_grad_blob(None, blob, layout=lay)
        if s["mass"] == "cartpole":
            return t
        return {k: v for k, v in t.items() if not k.startswith("M_net.")}

    def mass_zero(what, blob):
        if s["mass"] != "cartpole":
            t = weights.unpack_grad_blob(None, blob, layout=lay)
            rep.le(f"wgrad_mass_zero {what}", max(float(np.abs(v).max()) for k, v in t.items() if k.startswith("M_net.")), 0.0)

    x0, U = d[(37, 13)]
    for integ in ("euler", "rk4"):
        ref = m64.rollout_wgrad(x0, U, integ, d["dt"], d["traj_bar"], d["dx_bar"])
        traj = eng.rollout_trajectory(x0, U, integ, d["dt"])
        g, gu, gx = eng.rollout_wgrad(x0, U, traj, integ, d["dt"], traj_bar=d["traj_bar"], dx_bar=d["dx_bar"])
        rep.le(f"wgrad_rollout {integ} recompute", vc.err_named(named(npy(g)), named(ref["grad_theta"])), wt)
        mass_zero(f"{integ} recompute", npy(g))
        rep.le(f"wgrad_gu {integ} recompute", vc.err_max(npy(gu), ref["grad_u"]), wt)
        rep.le(f"wgrad_gx0 {integ} recompute", vc.err_max(npy(gx), ref["grad_x0"]), wt)
        traj_t = eng.rollout_trajectory(x0, U, integ, d["dt"], tapes=True)
        tok = eng.tape_token
        rep.le(f"wgrad_tape_token {integ}", 0.0 if tok is not None else 1.0, 0.0)
        g2, gu2, _ = eng.rollout_wgrad(x0, U, traj_t, integ, d["dt"], traj_bar=d["traj_bar"], dx_bar=d["dx_bar"],
                                       tape_token=tok)
        rep.le(f"wgrad_rollout {integ} tapes", vc.err_named(named(npy(g2)), named(ref["grad_theta"])), wt)
        mass_zero(f"{integ} tapes", npy(g2))
        rep.le(f"wgrad_gu {integ} tapes", vc.err_max(npy(gu2), ref["grad_u"]), wt)
    g, _, _ = eng.model_wgrad(d["x"], d["u"], d["lam"], d["Hbar"])
    rep.le("wgrad_point", vc.err_named(named(npy(g)), named(m64.wgrad(d["x"], d["u"], d["lam"], d["Hbar"]))), wt)
    g, xb, ub = eng.model_wgrad(d["x"], d["u"], d["lam"])
    rxb, rub = m64.vjp(d["x"], d["u"], d["lam"])
    rep.le("wgrad_point no_Hbar", vc.err_named(named(npy(g)), named(m64.wgrad(d["x"], d["u"], d["lam"]))), wt)
    vt = (vc.POINT_TOL * s["tol"]) if s["act"] != "relu" else vc.grad_tol(s)
    rep.le("wgrad_point xbar", vc.err_max(npy(xb), rxb), vt)
    rep.le("wgrad_point ubar", vc.err_max(npy(ub), rub), vt)


def _check_split(rep, sd, s, d, torch):
    whole, split = _engine(sd, s, split="never"), _engine(sd, s, split="always")
    rng = np.random.default_rng(vc.seed_of(rep.sid + "/split", s))
    for B in (1, 17, 37):
        x0, U = vc.states(rng, s["n"], B), vc.controls(rng, B, 13, s["m"])
        for integ in ("euler", "rk4"):
            for stash in (True, False):
                res = []
                for eng in (whole, split):
                    eng.use_stash = stash
                    c, gu, gx = eng.rollout_cost_grad(x0, U, d["cost"], integ, d["dt"], want_grad_x0=True)
                    _, tr = eng.rollout_cost(x0, U, d["cost"], integ, d["dt"], want_traj=True)
                    traj, dX = eng.rollout_trajectory(x0, U, integ, d["dt"], want_dx=True)
                    res.append([t.clone() for t in (c, gu, gx, tr, traj, dX)])
                    eng.use_stash = True
                for a, b, what in zip(res[0], res[1], ("cost", "grad_u", "grad_x0", "traj", "train_traj", "dX")):
                    rep.eq(f"split {what} B{B} {integ} stash={stash}", a, b)


def _check_launch(rep, sd, s, d, m64, n_cu, torch):
    """A ragged batch above 8 x n_cu tiles (partially filled last workgroup at 8 waves) under several wave caps; rows
    of it against the same rows run alone and against the oracle."""
    rng = np.random.default_rng(vc.seed_of(rep.sid + "/launch", s))
    B, H = 16 * (8 * n_cu + 3) + 5, 4
    x0, U = vc.states(rng, s["n"], B), vc.controls(rng, B, H, s["m"])
    x0t, Ut = torch.tensor(x0, device="cuda"), torch.tensor(U, device="cuda")
    rows = np.concatenate([np.arange(64), np.sort(rng.choice(np.arange(64, B - 21), 64, replace=False)),
                           np.arange(B - 21, B)])
    gt = vc.grad_tol(s)
    for integ in ("euler", "rk4"):
        outs = {}
        for mw in (8, 5, 3, 1):
            eng = _engine(sd, s, split="never", max_waves=mw)
            c, gu, gx = [t.clone() for t in eng.rollout_cost_grad(x0t, Ut, d["cost"], integ, d["dt"], want_grad_x0=True)]
            outs[mw] = (c, gu, gx)
            if mw == 8:
                assert eng.kernel_info(B)["rollouts_per_workgroup"] == 128
                small = eng.rollout_cost_grad(x0[rows], U[rows], d["cost"], integ, d["dt"], want_grad_x0=True)
                for a, b, what in zip((c, gu, gx), small, ("cost", "grad_u", "grad_x0")):
                    rep.eq(f"rows_alone {what} {integ}", a[torch.tensor(rows, device="cuda")], b)
            del eng
        for mw in (5, 3, 1):
            for a, b, what in zip(outs[8], outs[mw], ("cost", "grad_u", "grad_x0")):
                rep.eq(f"max_waves {what} {mw} {integ}", a, b)
        ref = m64.rollout(x0[rows], U[rows], d["cost"], integ, d["dt"], nthreads=NTHREADS)
        c, gu, gx = (npy(t)[rows] for t in outs[8])
        rep.le(f"big_batch_cost {integ}", vc.err_cost(c, ref["cost"]), vc.COST_RTOL * s["tol"])
        rep.le(f"big_batch_grad_u {integ}", vc.err_rows(gu, ref["grad_u"]), gt)
        rep.le(f"big_batch_grad_x0 {integ}", vc.err_rows(gx, ref["grad_x0"]), gt)


def _check_grid_stride(rep, eng, sd, s, d, m64, n_cu, torch):
    """Point kernels launched grid-stride (grid capped at 4 x n_cu workgroups): at least two stride passes and a
    ragged tail."""
    rng = np.random.default_rng(vc.seed_of(rep.sid + "/stride", s))
    n, m = s["n"], s["m"]
    N = 16 * (4 * n_cu * 8 * 2 + 1) + 7
    x, u = vc.states(rng, n, N), rng.uniform(vc.U_MIN, vc.U_MAX, size=(N, m)).astype(np.float32)
    lam = rng.normal(size=(N, n)).astype(np.float32)
    rows = np.concatenate([np.arange(64), np.sort(rng.choice(np.arange(64, N - 23), 64, replace=False)),
                           np.arange(N - 23, N)])
    ri = torch.tensor(rows, device="cuda")
    dx, H = eng.forward(x, u)
    xb, ub = eng.vjp(x, u, lam)
    dxs, Hs = eng.forward(x[rows], u[rows])
    xbs, ubs = eng.vjp(x[rows], u[rows], lam[rows])
    for a, b, what in ((dx, dxs, "f"), (H, Hs, "H"), (xb, xbs, "vjp_x"), (ub, ubs, "vjp_u")):
        rep.eq(f"stride_rows_alone {what}", a[ri], b)
    rdx, rH = m64.forward(x[rows], u[rows])
    rxb, rub = m64.vjp(x[rows], u[rows], lam[rows])
    vt = (vc.POINT_TOL * s["tol"]) if s["act"] != "relu" else vc.grad_tol(s)
    rep.le("stride f", vc.err_max(npy(dx)[rows], rdx), vc.POINT_TOL * s["tol"])
    rep.le("stride H", float(np.abs(npy(H)[rows] - rH).max() / max(1.0, np.abs(rH).max())), vc.POINT_TOL * s["tol"])
    rep.le("stride vjp_x", vc.err_max(npy(xb)[rows], rxb), vt)
    rep.le("stride vjp_u", vc.err_max(npy(ub)[rows], rub), vt)
    if s["wgrad"]:
        from phnn_mpc_amd import weights
        lay = weights.blob_layout(sd)
        K = -(-N // 37)
        rep_x, rep_u, rep_l = (np.tile(a[:37], (K, 1)) for a in (x, u, lam))
        g, _, _ = eng.model_wgrad(rep_x, rep_u, rep_l)
        ref = K * m64.wgrad(x[:37], u[:37], lam[:37])
        keep = (lambda k: True) if s["mass"] == "cartpole" else (lambda k: not k.startswith("M_net."))
        ours, theirs = (weights.unpack_grad_blob(None, a, layout=lay) for a in (npy(g), ref))
        rep.le(f"stride wgrad_point K={K}", vc.err_named({k: v for k, v in ours.items() if keep(k)},
                                                         {k: v for k, v in theirs.items() if keep(k)}),
               vc.WGRAD_TOL * s["tol"])


@pytest.mark.parametrize("sid", list(vc.ALL_SPECS))
def test_variant(torch, n_cu, sid):
    variant, s = vc.ALL_SPECS[sid]
    rep = Report(sid)
    sd = vc.build_state_dict(sid, s)
    d = vc.inputs(sid, s)
    m64 = ol.OracleModel(sd, "f64", activation=s["act"])
    eng = _engine(sd, s)
    # selection
    assert eng.variant == variant, (sid, eng.variant)
    assert eng.has_wgrad == s["wgrad"], (sid, eng.has_wgrad)
    always = _engine(sd, s, split="always")
    Bbig = 16 * 8 * n_cu * 2
    assert always.kernel_info(64)["rollouts_per_workgroup"] == 16
    assert (always.kernel_info(Bbig)["rollouts_per_workgroup"] == 16) == s["split"], sid
    del always
    # point operations, at the census scale and with every MLP weight matrix x3 (tanh saturates, f16x2 scales move)
    _check_points(rep, eng, m64, s, d, "x1")
    sd3 = vc.build_state_dict(sid, s, hidden_scale=3.0)
    e3 = _engine(sd3, s)
    _check_points(rep, e3, ol.OracleModel(sd3, "f64", activation=s["act"]), s, d, "x3")
    del e3
    _check_rollouts(rep, eng, m64, s, d)
    if s["wgrad"]:
        _check_wgrad(rep, eng, m64, s, d, sd, torch)
    if s["split"]:
        _check_split(rep, sd, s, d, torch)
    _check_launch(rep, sd, s, d, m64, n_cu, torch)
    _check_grid_stride(rep, eng, sd, s, d, m64, n_cu, torch)
    torch.cuda.synchronize()
    rep.finish()


@pytest.mark.parametrize("sid", list(vc.REFUSED))
def test_refused(torch, sid):
    from phnn_mpc_amd.engine import PhnnError
    s, why = vc.REFUSED[sid]
    with pytest.raises(PhnnError, match=why):
        _engine(vc.build_state_dict(sid, s), s)


@pytest.mark.parametrize("sid", list(vc.FALLBACKS))
def test_fallback_selection(torch, sid):
    """Requests served by another kernel than the options name, without an error: pins what pick_variant does."""
    s, variant = vc.FALLBACKS[sid]
    sd = vc.build_state_dict(sid, s)
    eng = _engine(sd, s)
    assert eng.variant == variant
    d = vc.inputs(sid, s)
    dx, _ = eng.forward(d["x"], d["u"])
    rdx, _ = ol.OracleModel(sd, "f64", activation=s["act"]).forward(d["x"], d["u"])
    assert vc.err_max(npy(dx), rdx) <= vc.POINT_TOL
