"""Batches whose rollouts differ: per-rollout isolation and power-of-two scale exactness of K1 (k_rollout_fwd), K2
(k_rollout_grad), k_model_forward and k_model_vjp, which put 16 rollouts in one wave, and of the solves on top.

A  Power-of-two homogeneity, bit for bit, every spec of the census (tests/test_heterogeneous_model.py shows the same on
   the float32 oracle, so the property belongs to the arithmetic): per-rollout cotangent scales 2^k_b, -40 .. 40 mixed
   inside every tile and two rollouts scaled by 0, through rollout_vjp and vjp (A1); Q, R and barrier_weight x 2^k
   through rollout_cost_grad, stash and recompute (A2); at the same scales the gradients of one spec per family against
   the float64 oracle (A3), so that a consistently wrong kernel does not pass.
B  Isolation, bit for bit: rollouts {0, 9, 15, 16, 36} carry a NaN / +inf / 1e30 / 7e4 state, a NaN control without
   and with bounds (the clamp passes a NaN on, as torch.clamp does: cost, trajectory from x_2 on and gradients are
   non-finite where the float64 oracle's are) or +-inf controls under the clamp; every output row of every other
   rollout equals the clean batch's.  The
   same for one problem of a solve, Adam, L-BFGS, MPPI and CEM.
C  The state-magnitude ladder against the float64 oracle: on every admitted rung (heterogeneous.DROPPED) the device is
   within the stated tolerance or non-finite, never finite and outside it; f32 and bf16x3 kernels are within tolerance
   everywhere, f16x2 kernels up to and including the 6.0e4 rung, and non-finite at 7.0e4 (the input layers of the march
   kernels and of k_model_forward split the raw state into float16 hi + lo: 7.0e4 -> inf - inf).

Shapes: B = 37 (two full tiles and a ragged one of 5), H = 6, Euler and RK4, use_stash on and off; variants with
split-tile kernels run split='never' and split='always', the latter also at B = 1 and 17.  Nothing here depends on a
state, control or cotangent VALUE for an address, a loop bound or the launch geometry: the non-finite inputs are data.
"""
import numpy as np
import pytest

import heterogeneous as het
import oracle_lib as ol
import variant_census as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def f32(t):
    return np.asarray(t, np.float32) if isinstance(t, np.ndarray) else t.detach().cpu().numpy().astype(np.float32)


_ENGINES = {}


def engines(sid, keep=False):
    """[(tag, engine, batch sizes)] of a spec: the whole-tile kernels, and for variants that have them the split-tile
    kernels (which also run the small batches).  keep: cached for the specs several tests share."""
    if sid in _ENGINES:
        return _ENGINES[sid]
    from phnn_mpc_amd.engine import RolloutEngine
    s = vc.ALL_SPECS[sid][1]
    sd = vc.build_state_dict(sid, s)
    out = [("never", RolloutEngine(sd, "cuda:0", **vc.engine_kwargs(s), split="never"), (het.B,))]
    if s["split"]:
        out.append(("always", RolloutEngine(sd, "cuda:0", **vc.engine_kwargs(s), split="always"),
                    (het.B,) + het.SPLIT_BATCHES))
        assert out[1][1].kernel_info(het.B)["rollouts_per_workgroup"] == 16
    if keep:
        _ENGINES[sid] = out
    return out


class Bits:
    """Collects failed bitwise properties of one test; asserts at the end, so one run shows every place."""

    def __init__(self, sid):
        self.sid, self.bad, self.n = sid, [], 0

    def homogeneous(self, what, got, base, sc):
        """got[b] == sc[b] * base[b] as uint32 where sc[b] != 0; got[b] == 0 where sc[b] == 0"""
        got, base = f32(got), f32(base)
        nz = sc != 0
        self.n += 1
        want = het.scaled_rows(base, sc)
        if not het.same_bits(got[nz], want[nz]):
            rows = np.flatnonzero(nz)[(got[nz].view(np.uint32) != want[nz].view(np.uint32)).reshape(int(nz.sum()), -1).any(axis=1)]
            self.bad.append(f"{what}: rollouts {rows.tolist()} (k = {het.row_exponents(len(sc))[rows].tolist()}) are "
                            "not 2^k times the unscaled result")
        if not (got[~nz] == 0).all():
            self.bad.append(f"{what}: a rollout scaled by 0 is not 0: {got[~nz].reshape(int((~nz).sum()), -1)[:, :4]}")

    def same(self, what, a, b, rows=None):
        a, b = f32(a), f32(b)
        if rows is not None:
            a, b = a[rows], b[rows]
        self.n += 1
        if not het.same_bits(a, b):
            d = (a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(axis=1)
            idx = np.flatnonzero(d) if rows is None else np.flatnonzero(rows)[d]
            self.bad.append(f"{what}: rows {idx.tolist()} differ")

    def le(self, what, err, bound):
        self.n += 1
        if not err <= bound:
            self.bad.append(f"{what}: {err:.3g} > {bound:.3g}")

    def true(self, what, ok):
        self.n += 1
        if not ok:
            self.bad.append(what)

    def finish(self):
        assert self.n > 0
        for b in self.bad:
            print(f"MISSED {self.sid}: {b}")
        assert not self.bad, (self.sid, self.bad)


def _cost_grad(eng, x0, U, cost, integ, dt, stash):
    """-> cost, grad_u, grad_x0, traj of K1 + K2 (fresh buffers)."""
    eng.use_stash = stash
    try:
        ws = {}
        c, gu, gx = eng.rollout_cost_grad(x0, U, cost, integ, dt, want_grad_x0=True, workspace=ws)
        return c, gu, gx, ws["traj"]
    finally:
        eng.use_stash = True


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize("sid", list(vc.ALL_SPECS))
def test_power_of_two_homogeneity(torch, sid):
    s = vc.ALL_SPECS[sid][1]
    rep = Bits(sid)
    m64 = ol.OracleModel(vc.build_state_dict(sid, s), "f64", activation=s["act"]) if sid in het.FAMILIES else None
    for tag, eng, batches in engines(sid, keep=sid in het.LADDER_SPECS):
        for nb in batches:
            d, sc = het.batch(sid, s, nb), het.row_scales(nb)
            one = np.ones(nb, np.float32)
            Tsc = het.scaled_rows(d["T"], sc)
            for integ in het.INTEGRATORS:
                t = f"{tag} B{nb} {integ}"
                # A1: per-rollout scales on the cotangents of the general reverse pass
                _, traj = eng.rollout_cost(d["x0"], d["U"], d["cost"], integ, d["dt"], want_traj=True)
                gu0, gx0 = eng.rollout_vjp(d["x0"], d["U"], traj, d["cost"], integ, d["dt"], traj_bar=d["T"], cost_bar=one)
                gu, gx = eng.rollout_vjp(d["x0"], d["U"], traj, d["cost"], integ, d["dt"], traj_bar=Tsc, cost_bar=sc)
                rep.true(f"A1 {t}: the unscaled gradient is finite and not zero",
                         bool(np.isfinite(f32(gu0)).all() and np.abs(f32(gu0)).max() > 0 and np.abs(f32(gx0)).max() > 0))
                rep.homogeneous(f"A1 rollout_vjp grad_u {t}", gu, gu0, sc)
                rep.homogeneous(f"A1 rollout_vjp grad_x0 {t}", gx, gx0, sc)
                if m64 is not None:  # A3: the scaled gradients against the float64 oracle
                    rgu, rgx = m64.rollout_vjp(d["x0"], d["U"], d["cost"], integ, d["dt"], traj_bar=Tsc, cost_bar=sc)
                    eu, ex = vc.err_rows(f32(gu), rgu), vc.err_rows(f32(gx), rgx)
                    print(f"A3 {sid} {t}: grad_u {eu / vc.grad_tol(s):.3f} grad_x0 {ex / vc.grad_tol(s):.3f} of the tolerance")
                    rep.le(f"A3 grad_u {t}", eu, vc.grad_tol(s))
                    rep.le(f"A3 grad_x0 {t}", ex, vc.grad_tol(s))
                # A2: the cost's weights times 2^k through K1 + K2
                for stash in (True, False):
                    base = [f32(a) for a in _cost_grad(eng, d["x0"], d["U"], d["cost_barrier"], integ, d["dt"], stash)]
                    plain = f32(_cost_grad(eng, d["x0"], d["U"], d["cost"], integ, d["dt"], stash)[0])
                    rep.true(f"A2 {t}: the barrier is active", bool((base[0] > plain).any()) or nb == 1)
                    for k in het.COST_EXPONENTS:
                        got = _cost_grad(eng, d["x0"], d["U"], het.scale_cost(d["cost_barrier"], k), integ, d["dt"], stash)
                        fk = np.full(nb, np.ldexp(1.0, k), np.float32)
                        for a, b, q in zip(got[:3], base[:3], ("cost", "grad_u", "grad_x0")):
                            rep.homogeneous(f"A2 {q} k={k} {t} stash={stash}", a, b, fk)
                        rep.same(f"A2 traj k={k} {t} stash={stash}", got[3], base[3])
            # A1 on the point VJP
            xb0, ub0 = eng.vjp(d["x0"], d["u"], d["lam"])
            xb, ub = eng.vjp(d["x0"], d["u"], het.scaled_rows(d["lam"], sc))
            rep.homogeneous(f"A1 vjp xbar {tag} B{nb}", xb, xb0, sc)
            rep.homogeneous(f"A1 vjp ubar {tag} B{nb}", ub, ub0, sc)
    torch.cuda.synchronize()
    rep.finish()


# ----------------------------------------------------------------------------- B
def _rollout_outputs(eng, x0, U, cost, integ, dt, T):
    """Every rollout operation's outputs, by name."""
    out = {}
    c, tr = eng.rollout_cost(x0, U, cost, integ, dt, want_traj=True)
    out["K1 cost"], out["K1 traj"] = f32(c), f32(tr)
    for stash in (True, False):
        c, gu, gx, _ = _cost_grad(eng, x0, U, cost, integ, dt, stash)
        out[f"K2 cost stash={stash}"], out[f"K2 grad_u stash={stash}"], out[f"K2 grad_x0 stash={stash}"] = f32(c), f32(gu), f32(gx)
    gu, gx = eng.rollout_vjp(x0, U, tr, cost, integ, dt, traj_bar=T, cost_bar=np.ones(len(x0), np.float32))
    out["vjp grad_u"], out["vjp grad_x0"] = f32(gu), f32(gx)
    traj, dX = eng.rollout_trajectory(x0, U, integ, dt, want_dx=True)
    out["train traj"], out["train dX"] = f32(traj), f32(dX)
    return out


@pytest.mark.parametrize("kind", het.POISONS)
@pytest.mark.parametrize("sid", het.ISOLATION_SPECS)
def test_isolation(torch, sid, kind):
    s = vc.ALL_SPECS[sid][1]
    rep = Bits(f"{sid} {kind}")
    m64 = ol.OracleModel(vc.build_state_dict(sid, s), "f64", activation=s["act"])
    for tag, eng, batches in engines(sid, keep=True):
        for nb in batches:
            if nb == 1:
                continue  # no neighbour
            d = het.batch(sid, s, nb)
            keep = het.others(nb)
            rows = np.flatnonzero(~keep)
            x0p, Up, cost = het.poison_rollout(kind, d["x0"], d["U"], d["cost"])
            for integ in het.INTEGRATORS:
                t = f"{tag} B{nb} {integ}"
                clean = _rollout_outputs(eng, d["x0"], d["U"], cost, integ, d["dt"], d["T"])
                dirty = _rollout_outputs(eng, x0p, Up, cost, integ, d["dt"], d["T"])
                for name in clean:
                    rep.same(f"{name} {t}", dirty[name], clean[name], rows=keep)
                rep.true(f"clean run finite {t}", all(np.isfinite(v).all() for v in clean.values()))
                # the poisoned rollouts themselves
                ref = m64.rollout(x0p, Up, cost, integ, d["dt"], nthreads=8)
                bad = ~np.isfinite(ref["cost"])
                rep.true(f"float64 oracle finite on the other rollouts {t}", not bad[keep].any())
                for name in ("K1 cost", "K2 cost stash=True", "K2 cost stash=False"):
                    rep.true(f"{name} {t}: finite where the float64 oracle's cost is not",
                             not np.isfinite(dirty[name][bad]).any())
                if kind == "nan_control_clamped":  # the clamp passes the NaN on (torch.clamp): it first reaches x_2
                    rep.true(f"oracle's cost non-finite on exactly the poisoned rollouts {t}", bool(bad[rows].all()))
                    rep.same(f"K1 traj rows 0..1 of the poisoned rollouts {t}", dirty["K1 traj"][rows][:, :2],
                             clean["K1 traj"][rows][:, :2])
                    rep.true(f"oracle's traj non-finite from row 2 on {t}",
                             bool((~np.isfinite(ref["traj"][rows][:, 2:])).any(axis=2).all()))
                    rep.true(f"K1 traj rows >= 2 non-finite where the float64 oracle's are {t}",
                             bool((~np.isfinite(dirty["K1 traj"][rows][:, 2:])).any(axis=2).all())
                             and not np.isfinite(dirty["K1 traj"][rows][:, 2:][~np.isfinite(ref["traj"][rows][:, 2:])]).any())
                    at_nan = np.isnan(Up[rows])  # the mask of the clamp zeroes the gradient entry at the NaN itself
                    for stash in (True, False):
                        for q in ("grad_u", "grad_x0"):
                            nf = ~np.isfinite(ref[q][rows])
                            if q == "grad_u":
                                nf &= ~at_nan
                            rep.true(f"oracle's {q} is non-finite somewhere {t}", bool(nf.any()))
                            rep.true(f"K2 {q} stash={stash} {t}: finite where the float64 oracle's is not",
                                     not np.isfinite(dirty[f"K2 {q} stash={stash}"][rows][nf]).any())
                if kind == "inf_control_clamped":  # the clamp makes them finite: the whole batch against the oracle
                    rep.true(f"oracle finite {t}", not bad.any())
                    rep.le(f"clamped cost {t}", vc.err_cost(dirty["K1 cost"], ref["cost"]), vc.COST_RTOL * s["tol"])
                    rep.le(f"clamped traj {t}", vc.err_traj(dirty["K1 traj"], ref["traj"]), s["tol"])
                    for stash in (True, False):
                        rep.le(f"clamped grad_u {t} stash={stash}",
                               vc.err_rows(dirty[f"K2 grad_u stash={stash}"], ref["grad_u"]), vc.grad_tol(s))
                        rep.le(f"clamped grad_x0 {t} stash={stash}",
                               vc.err_rows(dirty[f"K2 grad_x0 stash={stash}"], ref["grad_x0"]), vc.grad_tol(s))
                        rep.true(f"clamped controls carry no gradient {t}",
                                 bool((dirty[f"K2 grad_u stash={stash}"][rows][:, [0, 2]] == 0).all()))
            # the point operations
            xp, up = het.poison_point(kind, d["x0"], d["u"])
            for name, a, b in zip(("f", "H", "vjp xbar", "vjp ubar"),
                                  eng.forward(xp, up) + eng.vjp(xp, up, d["lam"]),
                                  eng.forward(d["x0"], d["u"]) + eng.vjp(d["x0"], d["u"], d["lam"])):
                rep.same(f"point {name} {tag} B{nb}", a, b, rows=keep)
                rep.true(f"point {name} clean finite", bool(np.isfinite(f32(b)).all()))
            badp = ~np.isfinite(m64.forward(xp, up)[0]).all(axis=1)
            rep.true(f"float64 oracle's f finite on the other rows {tag} B{nb}", not badp[keep].any())
            rep.true(f"point f {tag} B{nb}: finite where the float64 oracle's is not",
                     not np.isfinite(f32(eng.forward(xp, up)[0])[badp]).all(axis=1).any())
    torch.cuda.synchronize()
    rep.finish()


SOLVE_SPEC, SOLVE_B, SOLVE_BAD = het.FAMILIES[0], 19, 7


def _solve_inputs(torch):
    s = vc.ALL_SPECS[SOLVE_SPEC][1]
    d = het.batch(SOLVE_SPEC, s, SOLVE_B)
    x0p = d["x0"].copy()
    x0p[SOLVE_BAD, 2] = np.nan
    eng = engines(SOLVE_SPEC, keep=True)[0][1]
    keep = het.others(SOLVE_B, rows=(SOLVE_BAD,))
    return eng, d, x0p, keep


def test_solve_adam_isolates_a_nan_problem(torch):
    eng, d, x0p, keep = _solve_inputs(torch)
    rep = Bits("solve")
    kw = dict(integrator="euler", dt=d["dt"], lr=0.05, iters=4, track_best=True)
    clean, dirty = eng.solve(d["x0"], d["U"], d["cost"], **kw), eng.solve(x0p, d["U"], d["cost"], **kw)
    for k in ("u_last", "best_u", "best_cost"):
        rep.same(k, dirty[k], clean[k], rows=keep)
    rep.same("costs", dirty["costs"].T, clean["costs"].T, rows=keep)
    rep.true("clean finite", bool(np.isfinite(f32(clean["costs"])).all() and np.isfinite(f32(clean["best_cost"])).all()))
    rep.true("best_cost of the NaN problem stays +inf", f32(dirty["best_cost"])[SOLVE_BAD] == np.inf)
    rep.true("its costs are NaN", bool(np.isnan(f32(dirty["costs"])[:, SOLVE_BAD]).all()))
    rep.finish()


def test_solve_lbfgs_isolates_a_nan_problem(torch):
    from lbfgs_kernel_model import kernel_schedule
    eng, d, x0p, keep = _solve_inputs(torch)
    rep = Bits("solve_lbfgs")
    B, H, m = d["U"].shape
    kw = dict(lr=0.5, outer_steps=2, max_iter=3)
    clean = eng.solve_lbfgs(d["x0"], d["U"], d["cost"], "euler", d["dt"], **kw)
    dirty = eng.solve_lbfgs(x0p, d["U"], d["cost"], "euler", d["dt"], **kw)
    for k in ("u_last", "n_iter", "func_evals"):
        rep.true(f"{k} of the other problems", bool(torch.equal(dirty[k][torch.tensor(keep)], clean[k][torch.tensor(keep)])))
    rep.same("costs", dirty["costs"].T, clean["costs"].T, rows=keep)
    rep.true("the clean solve moves", bool((clean["n_iter"] >= 2).all()))
    ws = {}

    def ev(u, rows):  # the poisoned batch's K1 / K2 evaluations
        c, g = eng.rollout_cost_grad(x0p, u.to(eng.device).reshape(B, H, m), d["cost"], "euler", d["dt"], workspace=ws)
        return c.cpu().clone(), g.reshape(B, H * m).cpu().clone()

    with np.errstate(invalid="ignore"):
        model = kernel_schedule(ev, torch.tensor(d["U"]).reshape(B, H * m), **kw)
    # bit for bit on the other problems; on the NaN problem the same values, NaN for NaN (a NaN's sign and payload
    # are not part of the model)
    rep.same("u_last against the kernel model", dirty["u_last"].reshape(B, H * m), model["u_last"], rows=keep)
    rep.same("costs against the kernel model", dirty["costs"].T, model["costs"].T, rows=keep)
    for k, a in (("u_last", f32(dirty["u_last"]).reshape(B, H * m)), ("costs", f32(dirty["costs"]).T)):
        b = f32(model[k]) if k == "u_last" else f32(model[k]).T
        rep.true(f"{k} of the NaN problem against the kernel model: device {a[SOLVE_BAD]} model {b[SOLVE_BAD]}",
                 bool(np.array_equal(a[SOLVE_BAD], b[SOLVE_BAD], equal_nan=True)))
    for k in ("n_iter", "func_evals"):
        rep.true(f"{k} against the kernel model", bool(torch.equal(dirty[k].cpu(), model[k])))
    rep.true("the NaN problem's cost is NaN", bool(np.isnan(f32(dirty["costs"])[:, SOLVE_BAD]).all()))
    rep.finish()


def test_solve_mppi_isolates_a_nan_problem(torch):
    eng, d, x0p, keep = _solve_inputs(torch)
    rep = Bits("solve_mppi")
    kw = dict(integrator="euler", dt=d["dt"], iters=2, samples=30, lam=1.0, sigma=0.5, seed=5)
    clean, dirty = eng.solve_mppi(d["x0"], d["U"], d["cost"], **kw), eng.solve_mppi(x0p, d["U"], d["cost"], **kw)
    for k in ("u_last", "best_u", "best_cost"):
        rep.same(k, dirty[k], clean[k], rows=keep)
    rep.same("costs", dirty["costs"].T, clean["costs"].T, rows=keep)
    rep.true("clean finite", bool(np.isfinite(f32(clean["best_cost"])).all()))
    rep.true("the nominal moves in the clean solve", not het.same_bits(f32(clean["u_last"]), np.clip(d["U"], vc.U_MIN, vc.U_MAX)))
    # every sample cost of the NaN problem is non-finite: weight 0 each, the clamped nominal is kept, nothing is a best
    rep.same("u_last of the NaN problem is the clamped nominal", dirty["u_last"][SOLVE_BAD],
             np.clip(d["U"][SOLVE_BAD], np.float32(vc.U_MIN), np.float32(vc.U_MAX)))
    rep.true("best_cost of the NaN problem is +inf", f32(dirty["best_cost"])[SOLVE_BAD] == np.inf)
    rep.finish()


def test_solve_cem_isolates_a_nan_problem(torch):
    eng, d, x0p, keep = _solve_inputs(torch)
    rep = Bits("solve_cem")
    kw = dict(integrator="euler", dt=d["dt"], iters=3, samples=30, elites=6, alpha=0.25, sigma=0.5, sigma_min=0.05, seed=5)
    clean, dirty = eng.solve_cem(d["x0"], d["U"], d["cost"], **kw), eng.solve_cem(x0p, d["U"], d["cost"], **kw)
    for k in ("u_last", "sigma_last", "best_u", "best_cost"):
        rep.same(k, dirty[k], clean[k], rows=keep)
    rep.same("costs", dirty["costs"].T, clean["costs"].T, rows=keep)
    rep.true("clean finite", bool(np.isfinite(f32(clean["best_cost"])).all() and np.isfinite(f32(clean["costs"])).all()))
    nominal = np.clip(d["U"], np.float32(vc.U_MIN), np.float32(vc.U_MAX))
    rep.true("mean and standard deviation move in the clean solve",
             not het.same_bits(f32(clean["u_last"]), nominal) and bool((f32(clean["sigma_last"]) != np.float32(0.5)).any()))
    # no sample cost of the NaN problem is finite: no elite, mean and standard deviation are kept, nothing is a best
    rep.same("u_last of the NaN problem is the clamped nominal", dirty["u_last"][SOLVE_BAD], nominal[SOLVE_BAD])
    rep.true("sigma_last of the NaN problem is the initial sigma", bool((f32(dirty["sigma_last"])[SOLVE_BAD] == np.float32(0.5)).all()))
    rep.true("best_cost of the NaN problem is +inf", f32(dirty["best_cost"])[SOLVE_BAD] == np.inf)
    rep.true("its costs are not finite", not np.isfinite(f32(dirty["costs"])[:, SOLVE_BAD]).any())
    rep.finish()


# ----------------------------------------------------------------------------- C
def _device_group(eng, d, x, group):
    if group == "point":
        f, Hval = eng.forward(x, d["u"])
        xb, ub = eng.vjp(x, d["u"], d["lam"])
        return dict(f=f32(f), Hval=f32(Hval), xb=f32(xb), ub=f32(ub))
    c, gu, gx, tr = _cost_grad(eng, x, d["U"], d["cost"], group, d["dt"], True)
    return dict(cost=f32(c), traj=f32(tr), grad_u=f32(gu), grad_x0=f32(gx))


@pytest.mark.parametrize("sid", het.LADDER_SPECS)
def test_state_magnitude_ladder(torch, sid):
    """Within tolerance or non-finite on every admitted rung, never finite and outside tolerance; finite on every rung
    but f16x2's 7.0e4 (every figure is printed as a LADDER line before the test asserts).

    Measured on an MI355X, worst error / tolerance per rung over specs, groups and engines:
      f32:    x1e-12 .. x1e1 <= 0.03, x1e2 0.09, x1e3 0.45 (canonical point VJP), x1e4 0.05, theta <= 0.36, 6.0e4 and
              7.0e4 0.03
      bf16x3: x1e-12 .. x1e1 <= 0.02, x1e2 0.10, x1e3 0.52 (canonical point VJP), x1e4 0.03, theta <= 0.45, 6.0e4 0.03,
              7.0e4 0.04
      f16x2:  x1e-12 .. x1e2 <= 0.25, x1e3 0.48 (canonical point VJP), x1e4 0.15, theta <= 0.41, 6.0e4 0.04; 7.0e4: NaN
              on every row of the pHNN and canonical models (the input layers of the march kernels and of
              k_model_forward split the raw state into float16 hi + lo: inf - inf), finite and within 0.04 for ODEFunc
              (its first layer is an f32 product).
    This test found the f16x2 point VJP finite and OUTSIDE POINT_TOL at x1e3 for three pHNN specs (1.33, 1.03, 2.50 of the
    tolerance; the float32 oracle 0.16 .. 0.30): the f16 input layers carry 22 bits of the state and of W1, and the
    float64 oracle evaluated at those 22-bit images is off by 1.65, 0.85, 2.82.  k_model_vjp now takes the f32 input
    layers (0.20, 0.20, 0.30); the march kernels keep the f16 form, which their rollout tolerances absorb (<= 0.16)."""
    s = vc.ALL_SPECS[sid][1]
    rep = Bits(sid)
    mode = het.mode_of(sid)
    sd = vc.build_state_dict(sid, s)
    m64 = ol.OracleModel(sd, "f64", activation=s["act"])
    d = het.batch(sid, s)
    for rung, group in het.admitted(sid, s):
        x = het.ladder_states(s, d["x0"], rung)
        ref = het.oracle_group_outputs(m64, d, x, group)
        for tag, eng, _ in engines(sid, keep=True):
            e, fin = het.group_errors(s, group, _device_group(eng, d, x, group), ref)
            worst = max(e.values()) if e else float("nan")
            print(f"LADDER {sid} [{mode}] {rung} {group} {tag}: worst error/tolerance {worst:.3f} "
                  f"({max(e, key=e.get) if e else '-'}), finite rows {int(fin.sum())}/{len(fin)}")
            for k, v in e.items():
                rep.le(f"{rung} {group} {tag} {k} (finite rows)", v, 1.0)
            if mode == "f16x2" and rung == "big70000" and s["kind"] != "odefunc":
                rep.true(f"{rung} {group} {tag}: f16x2 past the float16 range is non-finite on every row", not fin.any())
            else:
                rep.true(f"{rung} {group} {tag}: finite on every row ({int(fin.sum())}/{len(fin)})", bool(fin.all()))
    torch.cuda.synchronize()
    rep.finish()


def test_gelu_second_derivative_far_out(torch):
    """phi''(z) = pdf(z) (2 - z^2) at |z| = 1e19 and 2e19 (z^2 overflows float32 past 1.8e19): the point VJP of a pHNN
    (which holds the Hessian of H) stays finite and within POINT_TOL of the float64 oracle."""
    from phnn_mpc_amd.engine import RolloutEngine
    sid = het.GELU_SPEC
    s = vc.ALL_SPECS[sid][1]
    d = het.batch(sid, s)
    rep = Bits(sid)
    eng = RolloutEngine(vc.build_state_dict(sid, s), "cuda:0", **vc.engine_kwargs(s))
    for z in het.GELU_Z:
        sd = het.gelu_state_dict(sid, s, z)
        eng.update_weights(sd)
        m64 = ol.OracleModel(sd, "f64", activation="gelu")
        xb, ub = (f32(a) for a in eng.vjp(d["x0"], d["u"], d["lam"]))
        rxb, rub = m64.vjp(d["x0"], d["u"], d["lam"])
        print(f"GELU z={z:g}: finite {bool(np.isfinite(xb).all())}, xbar {vc.err_max(xb, rxb) / vc.POINT_TOL:.3f} "
              f"ubar {vc.err_max(ub, rub) / vc.POINT_TOL:.3f} of POINT_TOL")
        rep.true(f"z={z:g}: finite", bool(np.isfinite(xb).all() and np.isfinite(ub).all()))
        rep.le(f"z={z:g} xbar", vc.err_max(xb, rxb), vc.POINT_TOL * s["tol"])
        rep.le(f"z={z:g} ubar", vc.err_max(ub, rub), vc.POINT_TOL * s["tol"])
    rep.finish()
