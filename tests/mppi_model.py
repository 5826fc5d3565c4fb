"""NumPy restatement of the MPPI kernels (phnn_mpc_amd/csrc/phnn_sampling.hip).  TEST INFRASTRUCTURE.

  philox4x32_10   Philox4x32-10 in integer arithmetic (uint64 products split into high / low words)
  counter / key   the counter layout of phnn_sampling.h: which (seed, epoch, iteration, problem, sample, float4) feeds a call
  normals         Box-Muller on the four words of a call: uniforms ((x >> 8) + 0.5) * 2^-24
  sample          v = clamp(u + sigma o z), sample 0 with z = 0
  update          u = clamp(sum_k w_k v_k / sum_k w_k), w_k = exp(-(S_k - min S) / lambda), best-sample tracking
each in a float32 form ('f32': every operation rounded to float32, reductions in the kernel's order: lane l of 16 takes
k = l, l + 16, ..., then the DPP butterfly; the weighted sum k ascending) and a float64 form ('f64': the yardstick).
MppiOracleEngine adds the two primitives (float64 form) to tests/oracle_engine.OracleEngine, so that solver.mppi_solve and
the controllers run on the CPU.
"""
import numpy as np
import torch

from oracle_engine import OracleEngine

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
LANES = 16
# supported ranges of the counter fields (phnn_sampling.h)
MAX_ITERS, MAX_SAMPLES, MAX_PROBLEM, MAX_J = 1 << 16, 1 << 26, 1 << 48, 64


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) unsigned 32-bit values -> (..., 4) uint32."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & MASK for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def key(seed):
    return np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)


def counter(epoch, iteration, gid, k, j):
    """The four counter words of (epoch, iteration, global problem id, sample, float4 index); arguments broadcast."""
    epoch, iteration, gid, k, j = (np.asarray(a, dtype=np.int64) for a in (epoch, iteration, gid, k, j))
    assert np.all((0 <= iteration) & (iteration < MAX_ITERS)) and np.all((0 <= gid) & (gid < MAX_PROBLEM))
    assert np.all((0 <= k) & (k < MAX_SAMPLES)) and np.all((0 <= j) & (j < MAX_J))
    g = gid.astype(np.uint64)
    c0 = g & MASK
    c1 = (g >> np.uint64(32)) | (iteration.astype(np.uint64) << np.uint64(16))
    c2 = epoch.astype(np.uint64) & MASK  # the int32 epoch's bit pattern
    c3 = (k.astype(np.uint64) << np.uint64(6)) | j.astype(np.uint64)
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def _unit(x, dtype):
    n = (x >> np.uint32(8)).astype(dtype)
    return (n + dtype(0.5)) * dtype(2.0 ** -24)


def box_muller(a, b, dtype):
    """words a, b -> (z0, z1) = r cos(2 pi u2), r sin(2 pi u2), r = sqrt(-2 ln u1); the kernel takes sin / cos of
    pi * (2 u2) (sincospi), the float32 form rounds that argument."""
    r = np.sqrt(dtype(-2.0) * np.log(_unit(a, dtype)))
    ang = dtype(np.pi) * (dtype(2.0) * _unit(b, dtype))
    return r * np.cos(ang), r * np.sin(ang)


def normals(seed, epoch, iteration, gids, K, N, dtype=np.float64):
    """-> z (len(gids), K, N): the noise of samples 0 .. K-1 of the given global problems; z[:, 0] = 0."""
    nv4 = (N + 3) // 4
    gids = np.asarray(gids, dtype=np.int64)
    c = counter(epoch, iteration, gids[:, None, None], np.arange(K)[None, :, None], np.arange(nv4)[None, None, :])
    o = philox4x32_10(c, key(seed))
    z = np.empty(o.shape, dtype)
    z[..., 0], z[..., 1] = box_muller(o[..., 0], o[..., 1], dtype)
    z[..., 2], z[..., 3] = box_muller(o[..., 2], o[..., 3], dtype)
    z = z.reshape(len(gids), K, 4 * nv4)[:, :, :N]
    z[:, 0] = 0
    return z


def sample(u, sigma, m, seed, epoch, iteration, problem_offset, K, u_min=None, u_max=None, dtype=np.float64):
    """u (B, N) float32 nominal -> v (B * K, N) of `dtype`: clamp(u + sigma o z)."""
    u = np.asarray(u, dtype=np.float32).astype(dtype)
    B, N = u.shape
    z = normals(seed, epoch, iteration, problem_offset + np.arange(B), K, N, dtype)
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float32).reshape(-1), (m,)).astype(dtype)
    v = u[:, None, :] + np.tile(sig, N // m)[None, None, :] * z
    if u_min is not None:
        v = np.minimum(np.maximum(v, dtype(np.float32(u_min))), dtype(np.float32(u_max)))
    return v.reshape(B * K, N)


def _row_sum(p):
    """The DPP butterfly of row_sum on 16 lane partials (..., 16) -> (...): quad_perm [1,0,3,2], quad_perm [2,3,0,1],
    row_half_mirror, row_mirror."""
    i = np.arange(LANES)
    for perm in (i ^ 1, i ^ 2, (i & 8) | (7 - (i & 7)), 15 - i):
        p = p + p[..., perm]
    return p[..., 0]


def update(u, v, s, lam, dtype=np.float64, u_min=None, u_max=None):
    """u (B, N), v (B * K, N), s (B * K) -> dict(u (B, N) new nominal, p (B, K) normalised weights, beta (B) lowest finite
    cost (+inf: none), kmin (B) its lowest sample index (-1: none))."""
    u = np.asarray(u).astype(dtype)
    B, N = u.shape
    K = np.asarray(s).size // B
    v = np.asarray(v).astype(dtype).reshape(B, K, N)
    s = np.asarray(s).astype(dtype).reshape(B, K)
    lam = dtype(np.float32(lam))
    fin = np.isfinite(s)
    beta = np.where(fin, s, np.inf).min(axis=1).astype(dtype)
    any_ = np.isfinite(beta)
    kmin = np.where(any_, np.argmax(fin & (s == beta[:, None]), axis=1), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(fin, np.exp(-((s - beta[:, None]) / lam)), 0).astype(dtype)
    w[~any_] = 0
    if dtype == np.float32:  # the kernel's order
        pad = (-K) % LANES
        part = np.zeros((B, LANES), dtype)
        for row in np.pad(w, ((0, 0), (0, pad))).reshape(B, -1, LANES).transpose(1, 0, 2):
            part = part + row
        W = _row_sum(part)
        acc = np.zeros((B, N), dtype)
        for k in range(K):
            acc = acc + np.where(fin[:, k, None], w[:, k, None] * v[:, k], dtype(0))
    else:
        W = w.sum(axis=1)
        acc = (w[:, :, None] * np.where(fin[:, :, None], v, 0)).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = acc / W[:, None]
        if u_min is not None:
            mean = np.minimum(np.maximum(mean, dtype(np.float32(u_min))), dtype(np.float32(u_max)))
        new = np.where(any_[:, None], mean, u)
        p = np.where(any_[:, None], w / W[:, None], 0)
    return {"u": new, "p": p, "beta": beta, "kmin": kmin}


def track_best(best_cost, best_u, v, res):
    """In place: the best-sample rule of k_mppi_update (strict '<') on float32 arrays."""
    B, N = best_u.shape
    v = np.asarray(v).reshape(B, -1, N)
    better = (res["kmin"] >= 0) & (res["beta"].astype(np.float32) < best_cost)
    for b in np.nonzero(better)[0]:
        best_cost[b] = res["beta"][b]
        best_u[b] = v[b, res["kmin"][b]]


class MppiOracleEngine(OracleEngine):
    """OracleEngine with the two MPPI primitives, served by the float64 form above (outputs rounded to float32 tensors, as
    everything this engine returns)."""

    def mppi_reference(self, x_ref, B, samples):
        raise NotImplementedError("the CPU stand-in has no reference tracking")

    def mppi_sample(self, x0, u, cost, samples, sigma, seed, iteration, epoch=0, problem_offset=0, workspace=None):
        x0 = np.asarray(x0, dtype=np.float32).reshape(-1, self.n)
        B = x0.shape[0]
        u = np.asarray(u, dtype=np.float32).reshape(B, -1)
        if samples < 2 or np.any(np.asarray(sigma) < 0) or not np.all(np.isfinite(sigma)):
            raise ValueError("samples < 2 or a negative / non-finite sigma")
        if isinstance(epoch, torch.Tensor):
            epoch = int(epoch.reshape(-1)[0])
        lo, hi = (float(cost.u_min), float(cost.u_max)) if cost.has_u_bounds else (None, None)
        v = sample(u, sigma, self.m, int(seed), int(epoch), int(iteration), int(problem_offset), int(samples), lo, hi)
        return self._out(v.reshape(B * samples, -1, self.m)), self._out(np.repeat(x0, samples, axis=0))

    def mppi_update(self, u, v, s, lam, cost, costs_row=None, best_cost=None, best_u=None):
        if not (lam > 0 and np.isfinite(lam)):
            raise ValueError("lambda must be > 0 and finite")
        B = u.shape[0]
        lo, hi = (float(cost.u_min), float(cost.u_max)) if cost.has_u_bounds else (None, None)
        res = update(u.numpy().reshape(B, -1), v.numpy().reshape(s.numel(), -1), s.numpy(), lam, u_min=lo, u_max=hi)
        if costs_row is not None:
            costs_row.copy_(s.reshape(B, -1)[:, 0])
        if best_cost is not None:
            track_best(best_cost.numpy(), best_u.numpy().reshape(B, -1), v.numpy(), res)
        u.copy_(self._out(res["u"]).reshape(u.shape))
