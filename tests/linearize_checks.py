"""The checks of one engine's linearisation kernels (TEST INFRASTRUCTURE), shared by tests/test_gpu_linearize.py (one
spec per code path, the wrapper's shapes) and tests/test_gpu_linearize_census.py (every census spec).  Each returns what it
measured and a list of the bitwise properties that did not hold, so that a caller may report before it asserts.

"As floats": -0 == +0, NaN at the same positions.

The composed reference at a NaN control.  A one-step rollout from a NaN control ends in a NaN state, and the reverse pass
multiplies the stage-cost gradient there by cost_bar = 0: 0 * NaN = NaN enters the costate, so at that rollout-step the
composed form returns NaN in every entry the clamp mask does not zero -- whatever the Jacobian is.  The kernel has no
such term (its cotangent is e_i itself), so an entry that does not depend on that control (the A rows of an Euler step
with a constant G) stays finite.  At that one rollout-step the comparison is therefore: equal as floats, or the reference
is NaN and the kernel's entry equals, bit for bit, what it returns with the NaN control replaced by 0."""
import numpy as np

import linearize_cases as lc
import linearize_model as lm
import variant_census as vc
from tvlqr_model import same_floats


def npf(t):
    return t.detach().cpu().numpy()


def first_diff(a, b):
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    k = np.argwhere(bad)
    return f"{int(bad.sum())} entries differ, first at {tuple(k[0])}: {a[tuple(k[0])]!r} vs {b[tuple(k[0])]!r}" if len(k) else "equal"


def unit(npts, n, i):
    e = np.zeros((npts, n), np.float32)
    e[:, i] = 1.0
    return e


# ----------------------------------------------------------------------------- point Jacobian
def point_rows(eng, x, u, what):
    """eng.jacobian(x, u) -> (A, Bm as numpy, [rows that are not eng.vjp(x, u, e_i) as floats])."""
    B, n, m = len(x), eng.n, eng.m
    A, Bm = eng.jacobian(x, u)
    assert A.shape == (B, n, n) and Bm.shape == (B, n, m), (what, A.shape, Bm.shape)
    A, Bm = npf(A), npf(Bm)
    bad = []
    for i in range(n):
        xb, ub = eng.vjp(x, u, unit(B, n, i))
        for name, got, ref in (("A", A[:, i], npf(xb)), ("Bm", Bm[:, i], npf(ub))):
            if not same_floats(got, ref):
                bad.append(f"{what} B{B} {name} row {i} against the VJP of e_{i}: {first_diff(got, ref)}")
    return A, Bm, bad


def point_errors(m64, x, u, A, Bm):
    """-> (error of A, error of Bm) against the float64 oracle Jacobian, each of its largest entry."""
    rA, rB = lm.oracle_jacobian(m64, x, u)
    return vc.err_max(A, rA), vc.err_max(Bm, rB)


# ----------------------------------------------------------------------------- step Jacobians
def composed(eng, traj, u, cost, integ, dt, points=None):
    """The only way to these numbers without the kernel: n general reverse passes over the B*H one-step rollouts (or
    over the listed points, each run alone)."""
    B, H, m = u.shape
    n = traj.shape[2]
    x0 = np.ascontiguousarray(traj[:, :H].reshape(B * H, n))
    ur = np.ascontiguousarray(u.reshape(B * H, 1, m))
    if points is not None:
        out = [composed(eng, x0[p].reshape(1, 1, n).repeat(2, axis=1), ur[p].reshape(1, 1, m), cost, integ, dt) for p in points]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    _, tr = eng.rollout_cost(x0, ur, cost, integ, dt, want_traj=True)
    zero = np.zeros(B * H, np.float32)
    A, Bm = np.empty((B * H, n, n), np.float32), np.empty((B * H, n, m), np.float32)
    for i in range(n):
        tb = np.zeros((B * H, 2, n), np.float32)
        tb[:, 1, i] = 1.0
        gu, gx = eng.rollout_vjp(x0, ur, tr, cost, integ, dt, traj_bar=tb, cost_bar=zero)
        A[:, i], Bm[:, i] = npf(gx), npf(gu)[:, 0]
    return A, Bm


def against_composed(what, got, ref, got_clean_u, nan_points):
    """-> [] or one line: got == ref as floats, with the rule of the module docstring at a NaN control."""
    ok = (got == ref) | (np.isnan(got) & np.isnan(ref))
    if nan_points.any():
        plain = int(ok[nan_points].sum())
        ok[nan_points] |= np.isnan(ref[nan_points]) & (got[nan_points].view(np.uint32) == got_clean_u[nan_points].view(np.uint32))
        if int(ok[nan_points].sum()) != plain:
            print(f"\n{what}: {int(ok[nan_points].sum()) - plain} of {ok[nan_points].size} entries at the NaN control are finite "
                  f"where the composed form is NaN")
    if ok.all():
        return []
    k = tuple(np.argwhere(~ok)[0])
    return [f"{what} against the composed form: {int((~ok).sum())} entries differ, first at {k}: {got[k]!r} vs {ref[k]!r}"]


def step_jacobians(torch, eng, m64, s, c, integ, bounded, what):
    """eng.rollout_linearize on one case of linearize_cases.case: bitwise against the composed form through
    eng.rollout_vjp, exactly zero Bm columns where the control is outside the bounds, and the error against
    linearize_model.oracle_linearize on the stored trajectory, per rollout-step.
    -> dict(A, Bm (B*H, ..), traj, rA, rB (the composed form), err, bad)."""
    n, m = s["n"], s["m"]
    x0, u, cost, dt = c["x0"], c["u"], c["cost"], c["dt"]
    B, H = u.shape[:2]
    bad = []
    A, Bm, traj = eng.rollout_linearize(x0, u, cost, integ, dt)
    assert A.shape == (B, H, n, n) and Bm.shape == (B, H, n, m) and traj.shape == (B, H + 1, n), what
    A2, B2, _ = eng.rollout_linearize(x0, u, cost, integ, dt, traj=traj)  # the trajectory given == K1 run here
    if not (torch.equal(A.view(torch.int32), A2.view(torch.int32)) and torch.equal(Bm.view(torch.int32), B2.view(torch.int32))):
        bad.append(f"{what}: the trajectory given against K1 run by the call, other bits")
    A, Bm, traj = npf(A).reshape(B * H, n, n), npf(Bm).reshape(B * H, n, m), npf(traj)
    assert np.isfinite(traj[:, :H]).all(), what
    # bitwise against the composed form
    rA, rB = composed(eng, traj, u, cost, integ, dt)
    nan_pts = ~lc.finite_points(u)
    assert int(nan_pts.sum()) == (1 if bounded and B * H > 1 else 0)
    Ac, Bc, _ = eng.rollout_linearize(x0, np.nan_to_num(u), cost, integ, dt, traj=traj)
    bad += against_composed(what + " A", A, rA, npf(Ac).reshape(A.shape), nan_pts)
    bad += against_composed(what + " Bm", Bm, rB, npf(Bc).reshape(Bm.shape), nan_pts)
    # the mask: a control outside the bounds, the NaN among them, gives an exactly zero column
    if bounded:
        cols = np.broadcast_to(lc.outside(u).reshape(B * H, 1, m), Bm.shape)
        if not np.all(Bm[cols] == 0.0):
            bad.append(f"{what}: {int((Bm[cols] != 0.0).sum())} nonzero entries of Bm in the columns of clamped controls")
    # parity against the float64 oracle on the same stored trajectory, per rollout-step
    keep = ~nan_pts
    oA, oB = lm.oracle_linearize(m64, traj, u, cost, integ, dt)
    err = max(vc.err_rows(A.reshape(B * H, -1)[keep], lm.rows_of(oA)[keep]),
              vc.err_rows(Bm.reshape(B * H, -1)[keep], lm.rows_of(oB)[keep]))
    return dict(A=A, Bm=Bm, traj=traj, rA=rA, rB=rB, err=err, bad=bad)
