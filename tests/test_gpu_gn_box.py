"""The box-constrained LQ step on the GPU (phnn_gn_direction_box, phnn_solve_gn_ex with PHNN_GN_BOX):

  1 direction    k_gn_direction_box == gn_box_model.direction_box bit for bit (du, dV, status, nclamp) on the device's own
                 float32 A, Bm, traj and u: B in {1, 17, 65} x H in {1, 2, 7}, Euler and RK4, one spec per (n, m) in
                 {(2,1), (3,1), (4,1), (4,2), (4,3), (4,4)}.  The inputs reach every branch, asserted on the model: nominals on the
                 upper and on the lower bound pushed outwards, interior nominals whose step ends on a bound, all-free
                 steps, steps only the forward sweep clips (asserted on the headline spec), per-problem mu, an active
                 barrier, no / a shared / a per-problem reference with a device offset; >= 25 % of the problem-steps hold
                 a component and >= 10 % of the problems hold none.  The failure cases: a nominal outside the bounds, a NaN control, NaN in B_t, a
                 negative definite R.  (A step that no active set passes needs a box-QP on a degenerate vertex to the
                 last bit; float32 inputs do not reach one, test_gn_box_model.py has it on the model.)
  2 plain        without has_u_bounds, and with bounds nothing reaches, every output equals phnn_gn_direction's
  3 solve        phnn_solve_gn_ex(PHNN_GN_BOX) == the five launches issued by hand (solver.gn_solve(box=True)) in every
                 output, nclamp_hist included; flags = 0 == phnn_solve_gn; eager == graph replay; one call == two half
                 batches; costs never rise and iterates stay in bounds on the golden cart-pole models; iters = 0, B = 0
  4 arguments    the refusals: unknown flag bits, nclamp_hist without the flag, and what phnn_solve_gn refuses
  5 footprint    both entry points in guarded buffers of exactly the reported sizes
  6 closed loop  8 plants x 5 steps of DeviceClosedLoop with gn_box=True == the host-driven loop
  7 slope        with nothing clamped, sum(grad_u * du) = -dV at test_gpu_gn.py's allowance"""
import ctypes as C

import numpy as np
import pytest

import footprint as fp
import gn_box_model as gb
import gn_model as gm
import oracle_lib as ol
import tvlqr_model as tm
import variant_census as vc
from test_gpu_footprint import Report, engine, footprint, rng_of
from test_gpu_gn import BATCHES, CFG, GN, HEADLINE, HORIZONS, INVALID, OUT_KEYS, SPECS, GnSolveOp, dev, npf, solve_case

pytestmark = pytest.mark.gpu

BOX_KEYS = OUT_KEYS + ("nclamp_hist",)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


def check_direction(what, out, ref):
    assert np.array_equal(npf(out["status"]), ref["status"]), (what, npf(out["status"]), ref["status"])
    assert np.array_equal(npf(out["nclamp"]), ref["nclamp"]), (what, npf(out["nclamp"]), ref["nclamp"])
    assert tm.same_floats(npf(out["du"]), ref["du"]), (what, "du")
    assert tm.same_floats(npf(out["dV"]), ref["dV"]), (what, "dV")


def same_outputs(torch, a, b, what, keys=BOX_KEYS):
    for k in keys:
        assert fp.same_bytes(torch, fp.as_bytes(torch, a[k]), fp.as_bytes(torch, b[k])), (what, k)


def box_controls(rng, B, H, m):
    """In-bounds controls with about 60 % on a bound, and every third problem inside the bounds."""
    u = np.clip(vc.controls(rng, B, H, m), vc.U_MIN, vc.U_MAX).astype(np.float32)
    on = rng.random(size=u.shape) < 0.4
    u[on] = np.where(rng.random(size=int(on.sum())) < 0.5, vc.U_MIN, vc.U_MAX).astype(np.float32)
    u[::3] = (0.25 + rng.uniform(-1, 1, size=u[::3].shape)).astype(np.float32)
    return u


# ----------------------------------------------------------------------------- 1. direction
@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("sid", SPECS)
def test_box_direction_equals_the_stated_order_model(torch, sid, integ):
    s, eng = vc.CENSUS[sid], engine(sid)
    n, m = s["n"], s["m"]
    seen = dict(steps=0, held=0, problems=0, free=0, upper=0, lower=0, interior=0, forward_only=0, active=0, ok=0)
    for B in BATCHES:
        for H in HORIZONS:
            rng = rng_of("gn-box-dir", sid, integ, B, H)
            x0 = vc.states(rng, n, B)
            u = box_controls(rng, B, H, m)
            cost = vc.cost_of(s, rng, barrier=True)
            mu = rng.choice([0.0, 1e-6, 0.125, 1.0], size=B)
            # the interior nominals: a third with a step that stays inside, the others with one of about the box's size
            mu[::3] = rng.choice([1e4, 1e4, 1.0, 3.0, 10.0, 30.0], size=mu[::3].shape)
            A, Bm, traj = eng.rollout_linearize(x0, u, cost, integ, vc.dt_of(s))
            An, Bn, tn = npf(A), npf(Bm), npf(traj)
            ldiag, _, _ = gm.gradients(tn, u, cost, n, m)
            seen["active"] += int((ldiag != np.diag(tm.cost_matrices_of(cost, n, m)[0])).sum())
            rows = 3
            shared = rng.uniform(-0.2, 0.2, size=(rows, n)).astype(np.float32)
            own = rng.uniform(-0.2, 0.2, size=(B, rows, n)).astype(np.float32)
            off = dev(torch, [1], torch.int32)
            for tag, kw, ref in (("target", {}, None),
                                 ("shared", dict(x_ref=shared, ref_offset=0), gm.reference_rows(shared, 0, H, B, n)),
                                 ("own+offset", dict(x_ref=own, ref_offset=off), gm.reference_rows(own, 1, H, B, n))):
                out = eng.gn_direction(A, Bm, traj, u, cost, dev(torch, mu), box=True, **kw)
                want = gb.direction_box(An, Bn, tn, u, cost, n, m, mu, ref)
                check_direction((sid, integ, B, H, tag), out, want)
                lo, hi = gb.step_bounds(u, cost)
                good = want["status"] == 0
                held = (want["clamped"] > 0) & good[:, None]
                k = want["k"]
                seen["steps"] += int(good.sum()) * H
                seen["held"] += int(held.sum())
                seen["problems"] += B
                seen["free"] += int((good & (want["clamped"].sum(axis=1) == 0) & (want["clipped"].sum(axis=1) == 0)).sum())
                seen["upper"] += int(((hi == 0) & (k == 0) & held[:, :, None]).sum())
                seen["lower"] += int(((lo == 0) & (k == 0) & held[:, :, None]).sum())
                seen["interior"] += int(((lo < 0) & (hi > 0) & ((k == lo) | (k == hi)) & held[:, :, None]).sum())
                seen["forward_only"] += int(((want["clipped"] > 0) & (want["clamped"] == 0) & good[:, None]).sum())
                seen["ok"] += int(good.sum())
                # u + du stays inside the bounds up to the one rounding of du
                v = u.astype(np.float64) + want["du"].astype(np.float64)
                assert v.min() >= vc.U_MIN - 2.0 ** -22 and v.max() <= vc.U_MAX + 2.0 ** -22
    print(f"\n{sid} {integ}: {seen}")
    assert seen["ok"] == seen["problems"], "these inputs are all feasible"
    assert 4 * seen["held"] >= seen["steps"] and 10 * seen["free"] >= seen["problems"]
    assert min(seen[k] for k in ("upper", "lower", "interior", "active")) > 0
    # a free step that only the forward sweep clips needs k_t + K_t dx_t to cross a bound that k_t alone respects: these
    # inputs give a dozen on the headline spec, and a handful, not a guaranteed one, on the others
    assert seen["forward_only"] > 0 or sid != HEADLINE


@pytest.mark.parametrize("sid", [SPECS[0], SPECS[2], SPECS[5]])
def test_box_direction_failure_cases(torch, sid):
    from phnn_mpc_amd import _capi
    s, eng = vc.CENSUS[sid], engine(sid)
    n, m = s["n"], s["m"]
    B, H = 17, 7
    rng = rng_of("gn-box-fail", sid)
    x0 = 0.5 * vc.states(rng, n, B)
    u = box_controls(rng, B, H, m)
    cost = vc.cost_of(s, rng)
    A, Bm, traj = eng.rollout_linearize(x0, u, cost, "euler", vc.dt_of(s))
    An, Bn, tn = npf(A), npf(Bm), npf(traj)
    un = u.copy()
    un[1, 4, 0] = np.float32(vc.U_MAX) + np.float32(0.5)   # a nominal above the bounds: status 5
    un[2, 0, m - 1] = np.float32(vc.U_MIN) - np.float32(2.0 ** -20)  # just below: status 1
    un[3, 2, 0] = np.nan                                   # a NaN control with bounds: status 3
    Bn[4, 5, 0, 0] = np.nan                                # the pivot of its own step: status 6
    tn[5, 3, n - 1] = np.nan                               # a trajectory row: no pivot, no bound -- status 0, no step
    out = eng.gn_direction(An, Bn, tn, un, cost, 1e-3, box=True)
    want = gb.direction_box(An, Bn, tn, un, cost, n, m, 1e-3)
    check_direction((sid, "failures"), out, want)
    assert list(want["status"][:6]) == [0, 5, 1, 3, 6, 0]
    for b in (1, 2, 3, 4, 5):
        assert np.all(want["du"][b] == 0) and np.isnan(want["dV"][b]) and want["nclamp"][b] == 0
    assert np.isfinite(want["dV"][[0] + list(range(6, B))]).all() and want["nclamp"].sum() > 0
    Q = np.ctypeslib.as_array(cost.Q)[: n * n].reshape(n, n)
    bad = _capi.make_cost(n, m, Q, -np.eye(m), None, vc.U_MIN, vc.U_MAX)
    out = eng.gn_direction(A, Bm, traj, u, bad, 0.0, box=True)
    want = gb.direction_box(npf(A), npf(Bm), npf(traj), u, bad, n, m, 0.0)
    check_direction((sid, "negative R"), out, want)
    assert (want["status"] == H).all() and np.isnan(want["dV"]).all() and not want["nclamp"].any()


# ----------------------------------------------------------------------------- 2. against the plain kernel
@pytest.mark.parametrize("sid", SPECS)
def test_without_active_bounds_every_output_is_the_plain_kernels(torch, sid):
    from phnn_mpc_amd import _capi
    s, eng = vc.CENSUS[sid], engine(sid)
    n, m = s["n"], s["m"]
    for B, H in ((1, 1), (17, 2), (65, 7)):
        rng = rng_of("gn-box-plain", sid, B, H)
        x0 = 0.5 * vc.states(rng, n, B)
        u = box_controls(rng, B, H, m)
        base = vc.cost_of(s, rng, barrier=True)
        mu = rng.choice([0.0, 1e-6, 0.125, 3.0], size=B)
        un = u.copy()
        if B > 1:
            un[1, H - 1, 0] = np.nan  # fails in both, with the same status
        for tag in ("no bounds", "wide bounds"):
            cost = _capi.Cost.from_buffer_copy(base)
            if tag == "no bounds":
                cost.has_u_bounds = 0
            else:
                cost.u_min, cost.u_max = -1e6, 1e6
            A, Bm, traj = eng.rollout_linearize(x0, u, cost, "euler", vc.dt_of(s))
            plain = eng.gn_direction(A, Bm, traj, un, cost, dev(torch, mu))
            box = eng.gn_direction(A, Bm, traj, un, cost, dev(torch, mu), box=True)
            if tag == "wide bounds" and B > 1:  # a NaN control with bounds is refused at its step instead
                assert int(box["status"][1]) == H and int(plain["status"][1]) == 0
                keep = [b for b in range(B) if b != 1]
            else:
                keep = list(range(B))
            for k in ("du", "dV", "status"):
                assert fp.same_bytes(torch, fp.as_bytes(torch, box[k][keep]), fp.as_bytes(torch, plain[k][keep])), (sid, B, H, tag, k)
            assert not bool(box["nclamp"].any()) and int((plain["status"] == 0).sum()) >= B - 1


# ----------------------------------------------------------------------------- 3. the composed solve
def solve_ex(torch, eng, x0, u_init, cost, integ, dt, iters, flags, want_nclamp, **opt):
    """phnn_solve_gn_ex called directly (engine.solve_gn reaches it only with the flag set)."""
    x0 = eng._t(x0, (-1, eng.n))
    B = x0.shape[0]
    u_init, H = eng._controls(u_init, B)
    o = eng._gn_options(iters, **opt)
    ws = torch.empty(max(eng.gn_workspace_bytes(B, H, o.line_steps), 256), dtype=torch.uint8, device=eng.device)
    f = dict(dtype=torch.float32, device=eng.device)
    out = {"u_last": u_init.detach().clone().contiguous(), "cost": torch.empty(B, **f), "costs": torch.empty(iters, B, **f),
           "mu": torch.empty(B, dtype=torch.float64, device=eng.device), "accepts": torch.empty(B, dtype=torch.int32, device=eng.device),
           "alpha_hist": torch.empty(iters, B, **f),
           "nclamp_hist": torch.full((iters, B), -7, dtype=torch.int32, device=eng.device) if want_nclamp else None}
    rc = eng.lib.phnn_solve_gn_ex(eng.h, eng._p(x0), eng._p(out["u_last"]), B, H, C.byref(cost), None, eng._integ(integ), float(dt),
                                  C.byref(o), eng._p(ws), ws.numel(), eng._p(out["cost"]), eng._p(out["costs"]), eng._p(out["mu"]),
                                  eng._p(out["accepts"]), eng._p(out["alpha_hist"]), flags, eng._p(out["nclamp_hist"]), eng._stream())
    fp.check_rc(eng, rc)
    return out


@pytest.mark.parametrize("integ", ["euler", "rk4"])
@pytest.mark.parametrize("sid", SPECS)
def test_solve_with_the_flag_equals_the_sequence_issued_by_hand(torch, sid, integ):
    from phnn_mpc_amd import _capi, solver
    eng = engine(sid)
    fell = held = 0
    for B, H, L, iters in ((1, 1, 1, 2), (17, 2, 4, 3), (65, 7, 4, 4)):
        s, x0, u0, cost, rng = solve_case(sid, B, H, ("box", integ))
        x0d, u0d = dev(torch, x0), dev(torch, u0)
        own = rng.uniform(-0.1, 0.1, size=(B, 3, s["n"])).astype(np.float32)
        off = dev(torch, [1], torch.int32)
        opt = dict(GN, line_steps=L)
        for tag, kw in (("target", {}), ("shared", dict(x_ref=own[0], ref_offset=1)), ("own+offset", dict(x_ref=own, ref_offset=off))):
            lib = eng.solve_gn(x0d, u0d, cost, integ, vc.dt_of(s), iters=iters, box=True, **opt, **kw)
            hand = solver.gn_solve(eng, x0d, u0d, cost, integ, vc.dt_of(s), iters, box=True, **opt, **kw)
            same_outputs(torch, lib, hand, (sid, integ, B, H, tag))
            chain = np.vstack([npf(lib["costs"]), npf(lib["cost"])[None]])
            assert np.isfinite(chain).all() and np.all(chain[1:] <= chain[:-1])
            fell += int((chain[-1] < chain[0]).sum())
            held += int(lib["nclamp_hist"].sum())
            ul = npf(lib["u_last"])
            assert ul.min() >= vc.U_MIN and ul.max() <= vc.U_MAX
            assert torch.equal(u0d, dev(torch, u0)) and torch.equal(x0d, dev(torch, x0))  # inputs untouched
        # the flag without a history, and no flag at all
        ex = solve_ex(torch, eng, x0d, u0d, cost, integ, vc.dt_of(s), iters, _capi.PHNN_GN_BOX, False, **opt)
        same_outputs(torch, ex, eng.solve_gn(x0d, u0d, cost, integ, vc.dt_of(s), iters=iters, box=True, **opt), (sid, "no history"), OUT_KEYS)
        ex = solve_ex(torch, eng, x0d, u0d, cost, integ, vc.dt_of(s), iters, 0, False, **opt)
        same_outputs(torch, ex, eng.solve_gn(x0d, u0d, cost, integ, vc.dt_of(s), iters=iters, **opt), (sid, "flags = 0"), OUT_KEYS)
    assert fell > 0 and held > 0


def test_graph_replay_and_half_batches_equal_the_eager_box_solve(torch):
    from phnn_mpc_amd import solver
    sid = HEADLINE
    eng = engine(sid)
    B, H = 18, 7
    s, x0, u0, cost, rng = solve_case(sid, B, H, "box-graph")
    x0d, u0d = dev(torch, x0), dev(torch, u0)
    own = rng.uniform(-0.1, 0.1, size=(B, 3, 4)).astype(np.float32)
    kw = dict(iters=3, box=True, **GN)
    for ref in (None, own):
        rkw = {} if ref is None else dict(x_ref=dev(torch, ref), ref_offset=1)
        eager = eng.solve_gn(x0d, u0d, cost, "euler", 0.02, **kw, **rkw)
        assert int(eager["nclamp_hist"].sum()) > 0
        graphed = solver.GraphedGN(eng)
        for _ in range(2):
            same_outputs(torch, graphed(eng, x0d, u0d, cost, "euler", 0.02, **kw, **rkw), eager, "graph")
        x1 = x0d * 0.5  # new inputs reach the captured buffers
        same_outputs(torch, graphed(eng, x1, u0d, cost, "euler", 0.02, **kw, **rkw), eng.solve_gn(x1, u0d, cost, "euler", 0.02, **kw, **rkw),
                     "graph, new x0")
        h = B // 2
        for lo, hi in ((0, h), (h, B)):
            hkw = {} if ref is None else dict(x_ref=dev(torch, ref[lo:hi]), ref_offset=1)
            part = eng.solve_gn(x0d[lo:hi], u0d[lo:hi], cost, "euler", 0.02, **kw, **hkw)
            for k in BOX_KEYS:
                whole = eager[k][:, lo:hi] if k in ("costs", "alpha_hist", "nclamp_hist") else eager[k][lo:hi]
                assert torch.equal(part[k], whole), (k, lo)


@pytest.mark.parametrize("name", ["phnn_cartpole", "canonical_cartpole"])
def test_costs_never_rise_and_iterates_stay_in_bounds_on_the_golden_models(torch, name):
    from phnn_mpc_amd import _capi
    from phnn_mpc_amd.engine import RolloutEngine
    eng = RolloutEngine(ol.load_weights(name), "cuda:0")
    x0 = gb.HARD_X0
    cost = _capi.make_cost(4, 1, [10.0, 200.0, 1.0, 10.0], 0.01, None, -3.0, 3.0)  # tight enough to bind at H = 10
    out = eng.solve_gn(x0, torch.zeros(4, 10, 1), cost, "euler", 0.02, iters=6, line_steps=4, box=True)
    chain = np.vstack([npf(out["costs"]), npf(out["cost"])[None]])
    assert np.isfinite(chain).all() and np.all(chain[1:] <= chain[:-1]) and np.all(chain[-1] < chain[0])
    assert bool((out["u_last"].abs() <= 3.0).all()) and int(out["nclamp_hist"].sum()) > 0
    assert torch.equal(eng.rollout_cost(x0, out["u_last"], cost, "euler", 0.02), out["cost"])


# ----------------------------------------------------------------------------- 4. arguments
def test_bad_arguments(torch):
    from phnn_mpc_amd import _capi
    sid = HEADLINE
    s, eng = vc.CENSUS[sid], engine(sid)
    lib, h, st = eng.lib, eng.h, eng._stream()
    assert lib.phnn_version() == 290
    B, H, n, m, L, iters = 5, 3, 4, 1, 4, 2
    f = dict(dtype=torch.float32, device="cuda:0")
    i32 = dict(dtype=torch.int32, device="cuda:0")
    t = dict(x0=torch.zeros(B, n, **f), u=torch.full((B, H, m), 0.25, **f), cost=torch.full((B,), 7.0, **f),
             costs=torch.full((iters, B), 7.0, **f), mu=torch.full((B,), 7.0, dtype=torch.float64, device="cuda:0"),
             accepts=torch.full((B,), 7, **i32), alpha=torch.full((iters, B), 7.0, **f), nclamp=torch.full((iters, B), 7, **i32),
             ws=torch.zeros(eng.gn_workspace_bytes(B, H, L), dtype=torch.uint8, device="cuda:0"))
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    cost = vc.cost_of(s, np.random.default_rng(0))
    bad_cost = vc.cost_of(s, np.random.default_rng(0))
    bad_cost.u_min, bad_cost.u_max = 1.0, -1.0
    BOX = _capi.PHNN_GN_BOX

    def opt(**kw):
        a = dict(iters=iters, line_steps=L, mu_init=1e-6, mu_min=1e-9, mu_max=1e6, mu_up=10.0, mu_down=0.1)
        a.update(kw)
        return C.byref(eng._gn_options(**a))

    def solve(x0=p["x0"], u=p["u"], nb=B, hh=H, c=C.byref(cost), integ=0, dt=0.02, o=None, ws=p["ws"], size=None,
              cost_out=p["cost"], mu=p["mu"], accepts=p["accepts"], flags=BOX, nclamp=p["nclamp"]):
        return lib.phnn_solve_gn_ex(h, x0, u, nb, hh, c, None, integ, dt, o or opt(), ws, t["ws"].numel() if size is None else size,
                                    cost_out, p["costs"], mu, accepts, p["alpha"], flags, nclamp, st)

    cases = [
        (lambda: solve(flags=2), "unknown flag bits"), (lambda: solve(flags=BOX | 4), "unknown flag bits"),
        (lambda: solve(flags=-1), "unknown flag bits"), (lambda: solve(flags=0), "without PHNN_GN_BOX"),
        (lambda: solve(x0=None), "NULL"), (lambda: solve(u=None), "NULL"), (lambda: solve(c=None), "cost is NULL"),
        (lambda: solve(cost_out=None), "required"), (lambda: solve(mu=None), "required"), (lambda: solve(accepts=None), "required"),
        (lambda: solve(ws=None), "workspace"), (lambda: solve(size=t["ws"].numel() - 1), "workspace"),
        (lambda: solve(nb=-1), "negative batch"), (lambda: solve(hh=0), "horizon < 1"), (lambda: solve(integ=2), "integrator"),
        (lambda: solve(dt=float("nan")), "dt"), (lambda: solve(c=C.byref(bad_cost)), "u_min > u_max"),
        (lambda: solve(o=opt(line_steps=33)), "line_steps"), (lambda: solve(o=opt(iters=-1)), "iters"),
        (lambda: solve(o=opt(mu_up=0.5)), "mu_up"),
    ]
    for k, (call, why) in enumerate(cases):
        rc = call()
        msg = lib.phnn_last_error(h).decode()
        assert rc == INVALID, (k, rc, msg)
        assert why in msg, (k, why, msg)
    # the direction itself: the checks of phnn_gn_direction, u_min > u_max among them
    A = torch.zeros(B, H, n, n, **f)
    Bm, traj = torch.zeros(B, H, n, m, **f), torch.zeros(B, H + 1, n, **f)
    du, dV, status = torch.full((B, H, m), 7.0, **f), torch.full((B,), 7.0, dtype=torch.float64, device="cuda:0"), torch.full((B,), 7, **i32)
    scratch = torch.zeros(B * H * (m * n + m), dtype=torch.float64, device="cuda:0")

    def direction(c=C.byref(cost), nb=B, hh=H, du_=du, scr=scratch):
        return lib.phnn_gn_direction_box(h, eng._p(A), eng._p(Bm), eng._p(traj), p["u"], nb, hh, c, None, p["mu"], eng._p(du_),
                                         eng._p(dV), eng._p(status), None, eng._p(scr), st)

    for call, why in ((lambda: direction(c=C.byref(bad_cost)), "u_min > u_max"), (lambda: direction(c=None), "cost is NULL"),
                      (lambda: direction(nb=-1), "negative batch"), (lambda: direction(hh=0), "horizon < 1"),
                      (lambda: direction(du_=None), "phnn_gn_direction_box: NULL tensor"), (lambda: direction(scr=None), "NULL tensor")):
        assert call() == INVALID and why in lib.phnn_last_error(h).decode(), why
    torch.cuda.synchronize()
    for k in ("cost", "costs", "mu", "accepts", "alpha", "nclamp"):
        assert bool((t[k] == 7).all()), k  # nothing was launched
    assert bool((t["u"] == 0.25).all()) and bool((du == 7).all()) and bool((status == 7).all())
    assert direction(nb=0) == 0 and direction() == 0  # a NULL nclamp is allowed
    assert lib.phnn_solve_gn_ex(h, None, None, 0, H, C.byref(cost), None, 0, 0.02, opt(), None, 0, None, None, None, None, None, BOX, None, st) == 0
    # iters = 0: the set-up alone
    assert solve(o=opt(iters=0)) == 0
    torch.cuda.synchronize()
    c0 = eng.rollout_cost(t["x0"], t["u"], cost, "euler", 0.02)
    assert torch.equal(t["cost"], c0) and bool((t["mu"] == 1e-6).all()) and bool((t["accepts"] == 0).all())
    assert bool((t["costs"] == 7).all()) and bool((t["nclamp"] == 7).all())
    assert solve() == 0 and solve(nclamp=None) == 0 and solve(flags=0, nclamp=None) == 0
    torch.cuda.synchronize()
    assert not bool((t["costs"] == 7).any()) and not bool((t["nclamp"] == 7).any())


# ----------------------------------------------------------------------------- 5. footprint
class GnBoxSolveOp(GnSolveOp):
    """phnn_solve_gn_ex(PHNN_GN_BOX) in a workspace of exactly phnn_gn_workspace_bytes, every output given."""

    def __init__(self, eng, cost, x0, U, integ, dt, L, iters=2):
        super().__init__(eng, cost, x0, U, integ, dt, L, iters)
        self.name = "box " + self.name
        self.add("nclamp", np.int32, (iters, self.B), fp.OUT)

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        opt = eng._gn_options(self.iters, self.L, GN["mu_init"], GN["mu_min"], GN["mu_max"], GN["mu_up"], GN["mu_down"])
        fp.check_rc(eng, eng.lib.phnn_solve_gn_ex(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), None, self.integ,
                                                  float(self.dt), C.byref(opt), p["ws"], self.nws, p["cost_out"], p["costs"],
                                                  p["mu"], p["accepts"], p["alpha"], _capi.PHNN_GN_BOX, p["nclamp"], eng._stream()))

    def engine(self, eng):
        r = eng.solve_gn(self.input("x0"), self.input("u"), self.cost, {0: "euler", 1: "rk4"}[self.integ], self.dt,
                         iters=self.iters, box=True, **dict(GN, line_steps=self.L))
        return {"u": r["u_last"], "cost_out": r["cost"], "costs": r["costs"], "mu": r["mu"], "accepts": r["accepts"],
                "alpha": r["alpha_hist"], "nclamp": r["nclamp_hist"]}


class GnBoxDirectionOp(fp.Op):
    """phnn_gn_direction_box with a scratch of exactly B*H*(m*n + m) float64."""

    def __init__(self, eng, cost, A, Bm, traj, u, mu):
        super().__init__()
        B, H, m = u.shape
        n = traj.shape[2]
        self.name = f"gn_direction_box B{B} H{H} n{n} m{m}"
        self.cost, self.B, self.H = cost, B, H
        f = np.float32
        self.add("A", f, (B, H, n, n), fp.IN, A)
        self.add("Bm", f, (B, H, n, m), fp.IN, Bm)
        self.add("traj", f, (B, H + 1, n), fp.IN, traj)
        self.add("u", f, (B, H, m), fp.IN, u)
        self.add("mu", np.float64, (B,), fp.IN, mu)
        self.add("du", f, (B, H, m), fp.OUT)
        self.add("dV", np.float64, (B,), fp.OUT)
        self.add("status", np.int32, (B,), fp.OUT)
        self.add("nclamp", np.int32, (B,), fp.OUT)
        self.add("scratch", np.float64, (B * H * (m * n + m),), fp.WS)

    def call(self, eng, p):
        fp.check_rc(eng, eng.lib.phnn_gn_direction_box(eng.h, p["A"], p["Bm"], p["traj"], p["u"], self.B, self.H, C.byref(self.cost),
                                                       None, p["mu"], p["du"], p["dV"], p["status"], p["nclamp"], p["scratch"],
                                                       eng._stream()))

    def engine(self, eng):
        import torch
        return eng.gn_direction(self.input("A"), self.input("Bm"), self.input("traj"), self.input("u"), self.cost,
                                torch.as_tensor(np.asarray(self.input("mu"))), box=True)


@pytest.mark.parametrize("sid", [SPECS[0], SPECS[2], SPECS[5]])
def test_footprint(torch, sid):
    """Both entry points: nothing outside the outputs and the workspace is written, the inputs are unchanged, the outputs
    do not depend on what the buffers held nor on what lies around the inputs, at a row-slice skew and with ragged B."""
    s, eng = vc.CENSUS[sid], engine(sid)
    rep = Report(f"gauss-newton box {sid}")
    for B in (1, 17):
        for H, L in ((1, 1), (7, 4)):
            rng = rng_of("gn-box-fp", sid, B, H)
            x0, cost = 0.3 * vc.states(rng, s["n"], B), vc.cost_of(s, rng, barrier=True)
            U = box_controls(rng, B, H, s["m"])
            footprint(rep, torch, eng, GnBoxSolveOp(eng, cost, x0, U, (B + H) % 2, vc.dt_of(s), L))
            A, Bm, traj = eng.rollout_linearize(x0, U, cost, "euler", vc.dt_of(s))
            mu = rng.choice([0.0, 1e-6, 0.125], size=B)
            footprint(rep, torch, eng, GnBoxDirectionOp(eng, cost, npf(A), npf(Bm), npf(traj), U, mu))
    rep.finish()


# ----------------------------------------------------------------------------- 6. the closed loop
def _load(cls, name, torch):
    m = cls(CFG)
    m.load_state_dict({k: torch.tensor(v) for k, v in ol.load_weights(name).items()})
    return m


def test_device_closed_loop_with_gn_box_equals_host_loop(torch):
    import yaml
    from phnn_mpc_amd.closed_loop import BatchedCartPole, run_mpc_batch, run_mpc_batch_device
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
    cfg = yaml.safe_load(open(CFG))
    cfg["mpc"].update(optimizer="GaussNewton", optimizer_steps=2, gn_line_steps=4, gn_box=True, u_min=-1.0, u_max=1.0)
    rng = np.random.default_rng(12)
    X = rng.uniform(-1, 1, size=(8, 4)) * [0.2, 0.08, 0.1, 0.1]
    T = 5
    for c in (create_mpc_from_config(_load(pHNN, "phnn_cartpole", torch), cfg),
              create_mpc_controller(_load(pHNN_Canonical, "canonical_cartpole", torch), cfg)):
        assert c.gn_box and c.gn_options()["box"] is True
        host = run_mpc_batch(BatchedCartPole(0.02), c, X, T)
        assert len(np.unique(host["controls"])) > T and np.abs(host["controls"]).max() == 1.0  # the bounds are reached
        c.gn_box = False
        assert not np.array_equal(run_mpc_batch(BatchedCartPole(0.02), c, X, T)["controls"], host["controls"])
        c.gn_box = True
        for use_graph in (False, True):
            dev_ = run_mpc_batch_device(c, X, T, use_graph=use_graph)
            assert np.array_equal(dev_["controls"], host["controls"])
            assert np.allclose(dev_["states"], host["states"], rtol=0, atol=1e-12)
            assert np.array_equal(dev_["done_step"], host["done_step"])


# ----------------------------------------------------------------------------- 7. the slope, against K2
@pytest.mark.parametrize("sid", SPECS)
def test_slope_is_minus_dv_where_nothing_is_clamped(torch, sid):
    """sum(grad_u * du) = -dV, test_gpu_gn.py's cross-check with K2 at its allowance, on its inputs with the control bounds
    moved out of reach.  The identity does NOT hold once a component is clamped: dV is then -(2 qu.k + k.Quu.k), which
    predicts the change of the model at the full step (-dV/2) but is no longer the slope -- do not add that check."""
    from phnn_mpc_amd import _capi
    s, eng = vc.CENSUS[sid], engine(sid)
    c = gm.slope_case(sid)
    cost = _capi.Cost.from_buffer_copy(c["cost"])
    cost.u_min, cost.u_max = -1e6, 1e6
    _, g = eng.rollout_cost_grad(c["x0"], c["u"], cost, "euler", c["dt"])
    g = npf(g).copy()
    A, Bm, traj = eng.rollout_linearize(c["x0"], c["u"], cost, "euler", c["dt"])
    d = eng.gn_direction(A, Bm, traj, c["u"], cost, 0.0, box=True)
    assert not bool(d["status"].any()) and not bool(d["nclamp"].any())
    dV = npf(d["dV"])
    miss, scale = gm.slope_mismatch(g, npf(d["du"]), dV)
    tol = vc.grad_tol(s) * scale + 64 * gm.SLOPE_F32_ORACLE * dV
    print(f"\n{sid}: worst |sum(g du) + dV| / dV {float((miss / dV).max()):.2e}, worst miss / tolerance {float((miss / tol).max()):.2e}")
    assert np.all(dV > 0) and np.all(miss <= tol)
