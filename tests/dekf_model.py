"""The disturbance-augmented extended Kalman filter (phnn_dekf_update / phnn_dekf_step / phnn_dist_compensate, DESIGN.md
section 23), stated as a thin assembly around ekf_model.update (TEST INFRASTRUCTURE).  Per problem the state is z = (x in
R^n, d in R^m), nz = n + m, the model x+ = F(x, c(u) + d), d+ = d, the measurement a selection of STATE components:

  update      ekf_model.update at size nz on  the prediction (x-, dhat) (float32),  A_z = [[A, Bm], [0, I]] assembled from
              the float32 A and Bm and exact 0 / 1,  Qz (nz,nz),  Rn read at the measured state components;  every
              statement of ekf_model.update carries over (float64, no fused multiply-adds, ascending inner products from
              0.0, L D L^T with k_tvlqr's pivot rule, the unmeasured rows -- all of d -- held as the identity in S, Joseph
              form, symmetrisation, (xhat, dhat) rounded once to float32, the special cases).  k_dekf_update equals it bit
              for bit (tests/test_gpu_dekf.py).
  textbook    ekf_model.textbook on the same assembled system (numpy.linalg)
  clamp32     c: the library's float32 clamp to the cost's bounds, a NaN stays NaN
  controls_row   row[b,k] = c(u[b,k]) + dhat[b,k], float32, the sum rounded once            (k_dekf_controls)
  compensate     u_cmd[b,k] = c(c(v[b,k]) - dhat[b,k]), float32, the difference rounded once; where dhat[b,k] is not
                 finite u_cmd = c(v) and status[b] = 1                                         (k_dist_compensate)
  DekfOracleEngine  EkfOracleEngine + dekf_update / dist_compensate, so that estimation.DisturbanceEKF.step and the
                 closed loop with it run without a GPU
"""
import numpy as np
import torch

import ekf_model as em
from ekf_model import same_floats  # noqa: F401  (re-exported for the tests)

NM = [(2, 1), (3, 1), (4, 1), (4, 2)]  # the (n, m) with a k_dekf_update


def assemble(A, Bm):
    """A (B,n,n), Bm (B,n,m) float32 -> A_z (B,nz,nz) float32 = [[A, Bm], [0, I]]."""
    A = np.asarray(A, np.float32)
    nb, n = A.shape[0], A.shape[1]
    Bm = np.asarray(Bm, np.float32).reshape(nb, n, -1)
    m = Bm.shape[2]
    Az = np.zeros((nb, n + m, n + m), np.float32)
    Az[:, :n, :n] = A
    Az[:, :n, n:] = Bm
    Az[:, n:, n:] = np.eye(m, dtype=np.float32)
    return Az


def _augmented(xpred, dhat, A, Bm, y, mask, Rn):
    xpred = np.asarray(xpred, np.float32)
    nb, n = xpred.shape
    dhat = np.asarray(dhat, np.float32).reshape(nb, -1)
    m = dhat.shape[1]
    assert not (mask >> n), "the measurement is a selection of state components"
    zpred = np.concatenate([xpred, dhat], axis=1)
    yz = np.full((nb, n + m), np.nan, np.float32)  # the d entries are never read
    yz[:, :n] = np.asarray(y, np.float32).reshape(nb, n)
    Rz = np.zeros(n + m)
    Rz[:n] = np.asarray(Rn, np.float64).reshape(-1)[:n]
    return zpred, assemble(np.asarray(A, np.float32).reshape(nb, n, n), Bm), yz, Rz, n, m


def update(xpred, dhat, A, Bm, Pz, y, mask, Qz, Rn):
    """xpred (B,n), dhat (B,m), A (B,n,n), Bm (B,n,m) float32, Pz (B,nz,nz) float64, y (B,n) float32 (unmeasured entries
    are not read), mask int (bits < n), Qz (nz,nz), Rn (n,) -> dict(xhat (B,n) float32, dhat (B,m) float32, P (B,nz,nz),
    nis (B), innov (B,n), status (B) int32, zhat64 (B,nz))."""
    zpred, Az, yz, Rz, n, m = _augmented(xpred, dhat, A, Bm, y, mask, Rn)
    r = em.update(zpred, Az, Pz, yz, mask, Qz, Rz)
    return dict(xhat=np.ascontiguousarray(r["xhat"][:, :n]), dhat=np.ascontiguousarray(r["xhat"][:, n:]), P=r["P"], nis=r["nis"],
                innov=np.ascontiguousarray(r["innov"][:, :n]), status=r["status"], zhat64=r["xhat64"])


def textbook(xpred, dhat, A, Bm, Pz, y, mask, Qz, Rn):
    """-> (xhat (B,n) float64, dhat (B,m) float64, Pz (B,nz,nz), nis (B)) by ekf_model.textbook on the assembled system."""
    zpred, Az, yz, Rz, n, m = _augmented(xpred, dhat, A, Bm, y, mask, Rn)
    zh, Pn, nis = em.textbook(zpred, Az, Pz, np.nan_to_num(yz.astype(np.float64)), mask, Qz, Rz)
    return zh[:, :n], zh[:, n:], Pn, nis


# ----------------------------------------------------------------------------- the two float32 kernels
def bounds_of(cost):
    """cost (_capi.Cost or None) -> (on, u_min, u_max) as float32."""
    if cost is None or not cost.has_u_bounds:
        return False, np.float32(0), np.float32(0)
    return True, np.float32(cost.u_min), np.float32(cost.u_max)


def clamp32(v, cost):
    """c(v): float32 clamp to the cost's bounds, a NaN stays NaN; None or no bounds: v."""
    v = np.asarray(v, np.float32)
    on, lo, hi = bounds_of(cost)
    if not on:
        return v.copy()
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), v, np.minimum(np.maximum(v, lo), hi)).astype(np.float32)


def controls_row(u, dhat, cost):
    """-> (B,m) float32: c(u) + dhat, the sum rounded once."""
    dhat = np.asarray(dhat, np.float32)
    with np.errstate(invalid="ignore"):
        return (clamp32(np.asarray(u, np.float32).reshape(dhat.shape), cost) + dhat).astype(np.float32)


def compensate(v, dhat, cost):
    """-> (u_cmd (B,m) float32, status (B) int32)."""
    dhat = np.asarray(dhat, np.float32)
    cv = clamp32(np.asarray(v, np.float32).reshape(dhat.shape), cost)
    ok = np.isfinite(dhat)
    with np.errstate(invalid="ignore"):
        diff = (cv - np.where(ok, dhat, np.float32(0))).astype(np.float32)
    u = np.where(ok, clamp32(diff, cost), cv).astype(np.float32)
    return u, (~ok).any(axis=1).astype(np.int32)


# ----------------------------------------------------------------------------- seeded problems
def seeded_problem(seed, nb, n, m, mask):
    """ekf_model.seeded_problem at size nz, cut into the augmented filter's inputs: A and Bm are the x rows of its A
    (I + 0.05 N(0,1): Bm = 0.05 N(0,1)), Pz and Qz full SPD (nz,nz), dhat = 0.5 N(0,1), y the x part ->
    dict(xpred, dhat, A, Bm, Pz, y, mask, Qz, Rn)."""
    p = em.seeded_problem(seed, nb, n + m, mask)
    return dict(xpred=np.ascontiguousarray(p["xpred"][:, :n]), dhat=np.ascontiguousarray(p["xpred"][:, n:]),
                A=np.ascontiguousarray(p["A"][:, :n, :n]), Bm=np.ascontiguousarray(p["A"][:, :n, n:]), Pz=p["P"],
                y=np.ascontiguousarray(p["y"][:, :n]), mask=mask, Qz=p["Qn"], Rn=p["Rn"][:n].copy())


def plant_cases(p, rng):
    """ekf_model.plant_cases for the augmented inputs, IN PLACE: a dropped measurement, an indefinite S, a NaN x-, a NaN
    dhat, an infinite A entry, an infinite Bm entry (where the batch is large enough) -> dict(case -> problem index)."""
    nb, n = p["xpred"].shape
    idx = em.measured_of(p["mask"], n)
    where = {}
    slots = list(rng.permutation(nb))
    if idx and nb >= 7:
        b = where["dropout"] = int(slots.pop())
        p["y"][b, idx[-1]] = np.inf
        b = where["indefinite"] = int(slots.pop())
        p["Pz"][b] = np.diag(np.full(p["Pz"].shape[1], -50.0))
    if nb >= 7:
        b = where["nan_xpred"] = int(slots.pop())
        p["xpred"][b, n - 1] = np.nan
        b = where["nan_dhat"] = int(slots.pop())
        p["dhat"][b, -1] = np.nan
        b = where["inf_A"] = int(slots.pop())
        p["A"][b, 0, n - 1] = np.inf
        b = where["inf_Bm"] = int(slots.pop())
        p["Bm"][b, n - 1, 0] = -np.inf
    return where


FAILS = ("indefinite", "nan_xpred", "nan_dhat", "inf_A", "inf_Bm")


def dekf_options(p):
    """A seeded problem's (or any dict with mask, Qz, Rn) _capi.DekfOptions."""
    from phnn_mpc_amd import _capi
    o = _capi.DekfOptions()
    o.meas_mask = int(p["mask"])
    q = np.asarray(p["Qz"], np.float64).reshape(-1)
    for i in range(q.size):
        o.Qz[i] = float(q[i])
    for i, r in enumerate(np.asarray(p["Rn"], np.float64).reshape(-1)):
        o.Rn[i] = float(r)
    return o


class DekfOracleEngine(em.EkfOracleEngine):
    """EkfOracleEngine with dekf_update and dist_compensate served by this file (CPU tensors)."""

    def dekf_update(self, xpred, A, Bm, y, Pz, dhat, opt, xhat=None, nis=True, innov=True, status=None, log=None):
        self.calls.append("dekf_update")
        n, nz = self.n, self.n + self.m
        Qz = np.array(opt.Qz[: nz * nz], np.float64).reshape(nz, nz)
        Rn = np.array(opt.Rn[:n], np.float64)
        r = update(np.asarray(xpred), np.asarray(dhat), np.asarray(A), np.asarray(Bm), np.asarray(Pz), np.asarray(y),
                   int(opt.meas_mask), Qz, Rn)
        self.last_Pz = r["P"]  # for the tests: the closed-loop drivers do not return the covariance
        Pz.copy_(torch.from_numpy(r["P"]))
        dhat.copy_(torch.from_numpy(r["dhat"]))
        return dict(xhat=torch.from_numpy(r["xhat"]), dhat=dhat, P=Pz, nis=torch.from_numpy(r["nis"]),
                    innov=torch.from_numpy(r["innov"]), status=torch.from_numpy(r["status"]))

    def dist_compensate(self, v, v_stride, dhat, cost, u_cmd=None, status=None):
        self.calls.append("dist_compensate")
        d = np.asarray(dhat, np.float32).reshape(-1, self.m)
        flat = np.asarray(v, np.float32).reshape(-1)
        vv = np.stack([flat[b * int(v_stride): b * int(v_stride) + self.m] for b in range(d.shape[0])])
        u, st = compensate(vv, d, cost)
        return torch.from_numpy(u), torch.from_numpy(st)


# ----------------------------------------------------------------------------- consistency with an unknown constant bias
def bias_system(seed, n, m, mask, nb=64, T=200, rho=0.98, Pd0=0.25):
    """ekf_model.consistency_system with an unknown constant input bias: x+ = F x + Bm d + w, d ~ N(0, Pd0 I) per problem,
    Bm a seeded float32 (n,m) matrix; F, Qn, Rn, P0 are the base system's, the trajectories are drawn anew with the bias
    in them -> the base dict plus Bm, d (nb,m), Pd0, and xs / ys / xhat0 replaced."""
    s = em.consistency_system(seed, n, mask, nb=nb, T=T, rho=rho)
    rng = np.random.default_rng(10_000 + seed)
    Bm = rng.normal(size=(n, m)).astype(np.float32).astype(np.float64)
    d = rng.normal(size=(nb, m)) * np.sqrt(Pd0)
    rng2 = np.random.default_rng(20_000 + seed)
    Lq = np.linalg.cholesky(s["Qn"])
    xs = np.zeros((T + 1, nb, n))
    ys = np.full((T, nb, n), np.nan, np.float32)
    for t in range(T):
        xs[t + 1] = xs[t] @ s["F"].T + d @ Bm.T + rng2.normal(size=(nb, n)) @ Lq.T
        v = rng2.normal(size=(nb, n)) * np.sqrt(s["Rn"])
        ys[t][:, s["idx"]] = (xs[t + 1] + v)[:, s["idx"]].astype(np.float32)
    xhat0 = (xs[0] + rng2.normal(size=(nb, n)) * np.sqrt(0.5)).astype(np.float32)
    s.update(Bm=Bm, d=d, xs=xs, ys=ys, xhat0=xhat0, Pd0=Pd0)
    return s


def nees_z(dhat, d, Pdd):
    """The z score of the d-block NEES averaged over the batch: mean m, standard deviation sqrt(2 m / B)."""
    e = np.asarray(dhat, np.float64) - d
    nees = np.einsum("bi,bij,bj->b", e, np.linalg.inv(Pdd), e)
    nb, m = e.shape
    return (nees.mean() - m) / np.sqrt(2.0 * m / nb)
