"""NumPy restatement of the CEM kernels (phnn_mpc_amd/csrc/phnn_sampling.hip).  TEST INFRASTRUCTURE.

  sample          v = clamp(u + sig o z) with a standard deviation per problem and element, sample 0 with z = 0; the
                  noise is mppi_model's (Philox4x32-10, the counter layout of phnn_sampling.h, Box-Muller)
  elite_order     the elite rule: among the finite costs the E lowest in the order (cost as floats with -0 == +0, then k
                  ascending), stated with a stable sort -- not with the kernel's key descent, which it is the check of
  update          em = mean of the elite rows, ev = mean of their squared deviations from em (two passes, k ascending),
                  u = clamp(alpha u + (1 - alpha) em), sig = max(sigma_min, sqrt(alpha sig^2 + (1 - alpha) ev))
each in a float32 form ('f32': every operation rounded to float32, in the kernel's order; the kernel has no
transcendental, so update's f32 form is what k_cem_update must return bit for bit) and a float64 form ('f64': the
yardstick).  CemOracleEngine adds the two primitives (float64 form) to mppi_model.MppiOracleEngine, so that
solver.cem_solve and the controllers run on the CPU.
"""
import numpy as np
import torch

import mppi_model as mm


def sample(u, sig, seed, epoch, iteration, problem_offset, K, u_min=None, u_max=None, dtype=np.float64):
    """u, sig (B, N) float32 mean and standard deviation -> v (B * K, N) of `dtype`: clamp(u + sig o z)."""
    u = np.asarray(u, dtype=np.float32).astype(dtype)
    sig = np.asarray(sig, dtype=np.float32).astype(dtype)
    B, N = u.shape
    z = mm.normals(seed, epoch, iteration, problem_offset + np.arange(B), K, N, dtype)
    v = u[:, None, :] + sig[:, None, :] * z
    if u_min is not None:
        v = np.minimum(np.maximum(v, dtype(np.float32(u_min))), dtype(np.float32(u_max)))
    return v.reshape(B * K, N)


def elite_order(s, E):
    """s (K,) float32 costs -> the sample indices of the elites, best first: the finite costs sorted by (cost, k) with
    -0 equal to +0, the first min(E, number of finite costs) of them."""
    s = np.asarray(s, dtype=np.float32)
    k = np.nonzero(np.isfinite(s))[0]
    order = k[np.argsort(s[k] + np.float32(0.0), kind="stable")]  # x + 0 turns -0 into +0; stable: k ascending on ties
    return order[:E]


def elite_mask(s, E):
    """s (B, K) -> (B, K) bool."""
    s = np.asarray(s, dtype=np.float32)
    mask = np.zeros(s.shape, bool)
    for b in range(s.shape[0]):
        mask[b, elite_order(s[b], E)] = True
    return mask


def update(u, sig, v, s, E, alpha, sigma_min, dtype=np.float64, u_min=None, u_max=None):
    """u, sig (B, N), v (B * K, N), s (B * K) -> dict(u, sig (B, N) of `dtype`: the refitted mean and standard deviation
    (kept where no cost is finite), elite (B, K) bool, n_elite (B), beta (B) cost of the best sample (+inf: none), kmin
    (B) its index (-1: none))."""
    u0 = np.asarray(u, dtype=np.float32).astype(dtype)
    B, N = u0.shape
    sig0 = np.asarray(sig, dtype=np.float32).astype(dtype).reshape(B, N)
    s32 = np.asarray(s, dtype=np.float32).reshape(B, -1)
    K = s32.shape[1]
    v = np.asarray(v, dtype=np.float32).astype(dtype).reshape(B, K, N)
    elite = elite_mask(s32, E)
    n_el = elite.sum(axis=1)
    any_ = n_el > 0
    kmin = np.array([elite_order(s32[b], 1)[0] if any_[b] else -1 for b in range(B)])
    beta = np.where(any_, s32[np.arange(B), np.maximum(kmin, 0)], np.float32(np.inf)).astype(np.float32)
    Ef = np.maximum(n_el, 1).astype(dtype)[:, None]
    a = dtype(np.float32(alpha))
    oma = dtype(np.float32(1.0) - np.float32(alpha)) if dtype == np.float32 else dtype(1.0) - a
    smin = dtype(np.float32(sigma_min))
    acc = np.zeros((B, N), dtype)
    for k in range(K):  # k ascending; a row that is no elite is not added at all
        acc = np.where(elite[:, k, None], acc + v[:, k], acc)
    em = acc / Ef
    acc = np.zeros((B, N), dtype)
    for k in range(K):
        d = v[:, k] - em
        acc = np.where(elite[:, k, None], acc + d * d, acc)
    ev = acc / Ef
    assert not np.any(ev < 0)  # a NaN sample or mean gives a NaN variance, never a negative one
    mean = a * u0 + oma * em
    if u_min is not None:
        mean = np.minimum(np.maximum(mean, dtype(np.float32(u_min))), dtype(np.float32(u_max)))
    new_sig = np.maximum(smin, np.sqrt(a * (sig0 * sig0) + oma * ev))
    return {"u": np.where(any_[:, None], mean, u0), "sig": np.where(any_[:, None], new_sig, sig0), "elite": elite,
            "n_elite": n_el, "beta": beta, "kmin": kmin}


track_best = mm.track_best  # the best-sample rule is k_mppi_update's


class CemOracleEngine(mm.MppiOracleEngine):
    """MppiOracleEngine with the two CEM primitives, served by the float64 form above (outputs rounded to float32)."""

    def cem_sample(self, x0, u, sig, cost, samples, seed, iteration, epoch=0, problem_offset=0, workspace=None):
        x0 = np.asarray(x0, dtype=np.float32).reshape(-1, self.n)
        B = x0.shape[0]
        u = np.asarray(u, dtype=np.float32).reshape(B, -1)
        sig = np.asarray(sig, dtype=np.float32).reshape(B, -1)
        if samples < 2:
            raise ValueError("samples < 2")
        if isinstance(epoch, torch.Tensor):
            epoch = int(epoch.reshape(-1)[0])
        lo, hi = (float(cost.u_min), float(cost.u_max)) if cost.has_u_bounds else (None, None)
        v = sample(u, sig, int(seed), int(epoch), int(iteration), int(problem_offset), int(samples), lo, hi)
        return self._out(v.reshape(B * samples, -1, self.m)), self._out(np.repeat(x0, samples, axis=0))

    def cem_update(self, u, sig, v, s, elites, alpha, sigma_min, cost, costs_row=None, best_cost=None, best_u=None):
        B = u.shape[0]
        K = s.numel() // max(B, 1)
        if not 1 <= elites <= K:
            raise ValueError("elites outside 1 .. samples")
        if not 0 <= alpha < 1:
            raise ValueError("alpha must be in [0, 1)")
        if not (sigma_min >= 0 and np.isfinite(sigma_min)):
            raise ValueError("sigma_min must be >= 0 and finite")
        lo, hi = (float(cost.u_min), float(cost.u_max)) if cost.has_u_bounds else (None, None)
        res = update(u.numpy().reshape(B, -1), sig.numpy().reshape(B, -1), v.numpy().reshape(s.numel(), -1), s.numpy(),
                     int(elites), alpha, sigma_min, u_min=lo, u_max=hi)
        if costs_row is not None:
            costs_row.copy_(s.reshape(B, -1)[:, 0])
        if best_cost is not None:
            track_best(best_cost.numpy(), best_u.numpy().reshape(B, -1), v.numpy(), res)
        u.copy_(self._out(res["u"]).reshape(u.shape))
        sig.copy_(self._out(res["sig"]).reshape(sig.shape))


NO_KEY = np.uint32(0xFFFFFFFF)


def cost_keys(s):
    """k_cem_update's 32-bit keys: unsigned integers that order as the finite float32 costs do, -0 and +0 sharing one,
    every non-finite cost on NO_KEY (above all of them)."""
    s = np.asarray(s, dtype=np.float32)
    b = np.where(s == 0, np.uint32(0), s.view(np.uint32))
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isfinite(s), key, NO_KEY)


def descent_order(s, E):
    """The kernel's selection method on one problem's costs s (K,): the E-th smallest key T by a 32-step descent over
    the key's bits, then the stream k = 0, 1, ...: key < T, or key == T while fewer than E - #{key < T} such rows have
    been taken.  -> the elite indices, k ascending."""
    keys = cost_keys(s).astype(np.uint64)
    nf = int((keys != np.uint64(NO_KEY)).sum())
    if nf == 0:
        return np.zeros(0, np.int64)
    E = min(int(E), nf)
    T, below = 0, 0
    for bit in range(31, -1, -1):
        trial = T | (1 << bit)
        c = int((keys < np.uint64(trial)).sum())
        if c < E:
            T, below = trial, c
    ties, taken, out = E - below, 0, []
    for k, key in enumerate(int(x) for x in keys):
        if key < T:
            out.append(k)
        elif key == T and taken < ties:
            taken += 1
            out.append(k)
    return np.array(out, np.int64)
