"""NumPy restatement of the shaped sampler (k_shaped_sample, phnn_mpc_amd/csrc/phnn_sampling.hip).  TEST INFRASTRUCTURE.

  white           eps (B, K, P, m): the white normals of a row of length P * m, mppi_model's (Philox4x32-10, the counter
                  layout of phnn_sampling.h, Box-Muller); element s * m + c of the row is eps[s, c]
  shape           z[t, c] = sum_s L[t, s] eps[s, c]; the float32 form in the kernel's stated order: acc = 0, then
                  acc = acc + L[t, s] * eps[s, c] for s ascending, the product rounded, then the sum
  sample          v = clamp(u + sigma o z), sample 0 with z = 0; sigma a per-component table (MPPI: `m` given) or a (B, N)
                  tensor (CEM: m None)
each in a float64 form (the yardstick) and a float32 form.  ShapedMppiOracleEngine / ShapedCemOracleEngine are the CPU
oracle engines of mppi_model / cem_model whose *_sample take `noise`, so that the solvers and controllers run shaped on
the CPU.
"""
import numpy as np
import torch

import cem_model as cm
import mppi_model as mm


def white(seed, epoch, iteration, gids, K, P, m, dtype=np.float64):
    """-> eps (len(gids), K, P, m); sample 0's row is zero as in mm.normals (it is never used)."""
    return mm.normals(seed, epoch, iteration, gids, K, P * m, dtype).reshape(len(gids), K, P, m)


def shape(L, eps, dtype=np.float64):
    """L (H, P) float32, eps (..., P, m) -> z (..., H, m) of `dtype`."""
    L = np.asarray(L, dtype=np.float32).astype(dtype)
    eps = np.asarray(eps).astype(dtype)
    H, P = L.shape
    assert eps.shape[-2] == P
    if dtype == np.float64:
        return np.einsum("ts,...sc->...tc", L, eps)
    acc = np.zeros(eps.shape[:-2] + (H, eps.shape[-1]), np.float32)
    for s in range(P):  # the kernel's order; every product and every sum rounded to float32
        prod = (L[:, s][:, None] * eps[..., s, None, :]).astype(np.float32)
        acc = (acc + prod).astype(np.float32)
    return acc


def noise(L, m, seed, epoch, iteration, gids, K, dtype=np.float64, eps=None):
    """-> z (len(gids), K, H * m): the shaped noise rows, z[:, 0] = 0.  eps: the white normals to use instead of the
    counter's (tests that alter them)."""
    L = np.asarray(L, dtype=np.float32)
    H, P = L.shape
    if eps is None:
        eps = white(seed, epoch, iteration, gids, K, P, m, dtype)
    z = shape(L, eps, dtype).reshape(eps.shape[0], K, H * m)
    z[:, 0] = 0
    return z


def sample(u, sigma, m, L, seed, epoch, iteration, problem_offset, K, u_min=None, u_max=None, dtype=np.float64):
    """u (B, N) float32 -> v (B * K, N) of `dtype`: clamp(u + sigma o z).  sigma: MPPI's table (one value or one per
    component); CEM's tensor: sample_tensor."""
    u = np.asarray(u, dtype=np.float32).astype(dtype)
    B, N = u.shape
    z = noise(L, m, seed, epoch, iteration, problem_offset + np.arange(B), K, dtype)
    sig = np.broadcast_to(np.asarray(sigma, dtype=np.float32).reshape(-1), (m,)).astype(dtype)
    v = u[:, None, :] + np.tile(sig, N // m)[None, None, :] * z
    if u_min is not None:
        v = np.minimum(np.maximum(v, dtype(np.float32(u_min))), dtype(np.float32(u_max)))
    return v.reshape(B * K, N)


def sample_tensor(u, sig, m, L, seed, epoch, iteration, problem_offset, K, u_min=None, u_max=None, dtype=np.float64):
    """CEM's form: sig (B, N) float32 standard deviations per problem and element."""
    u = np.asarray(u, dtype=np.float32).astype(dtype)
    sig = np.asarray(sig, dtype=np.float32).astype(dtype)
    B, N = u.shape
    z = noise(L, m, seed, epoch, iteration, problem_offset + np.arange(B), K, dtype)
    v = u[:, None, :] + sig[:, None, :] * z
    if u_min is not None:
        v = np.minimum(np.maximum(v, dtype(np.float32(u_min))), dtype(np.float32(u_max)))
    return v.reshape(B * K, N)


def _L_of(noise_arg):
    return np.asarray(noise_arg.L if hasattr(noise_arg, "L") else noise_arg, dtype=np.float32)


class ShapedMppiOracleEngine(mm.MppiOracleEngine):
    """MppiOracleEngine whose mppi_sample takes `noise` (a noise.Noise or an (H, P) array): the float64 form above."""

    def mppi_sample(self, x0, u, cost, samples, sigma, seed, iteration, epoch=0, problem_offset=0, workspace=None, noise=None):
        if noise is None:
            return super().mppi_sample(x0, u, cost, samples, sigma, seed, iteration, epoch, problem_offset, workspace)
        x0 = np.asarray(x0, dtype=np.float32).reshape(-1, self.n)
        B = x0.shape[0]
        u = np.asarray(u, dtype=np.float32).reshape(B, -1)
        L = _L_of(noise)
        if L.shape[0] * self.m != u.shape[1]:
            raise ValueError("the noise shape's rows are not the horizon")
        if isinstance(epoch, torch.Tensor):
            epoch = int(epoch.reshape(-1)[0])
        lo, hi = (float(cost.u_min), float(cost.u_max)) if cost.has_u_bounds else (None, None)
        v = sample(u, sigma, self.m, L, int(seed), int(epoch), int(iteration), int(problem_offset), int(samples), lo, hi)
        return self._out(v.reshape(B * samples, -1, self.m)), self._out(np.repeat(x0, samples, axis=0))


class ShapedCemOracleEngine(cm.CemOracleEngine, ShapedMppiOracleEngine):
    """CemOracleEngine whose cem_sample (and mppi_sample) take `noise`."""

    def cem_sample(self, x0, u, sig, cost, samples, seed, iteration, epoch=0, problem_offset=0, workspace=None, noise=None):
        if noise is None:
            return super().cem_sample(x0, u, sig, cost, samples, seed, iteration, epoch, problem_offset, workspace)
        x0 = np.asarray(x0, dtype=np.float32).reshape(-1, self.n)
        B = x0.shape[0]
        u = np.asarray(u, dtype=np.float32).reshape(B, -1)
        sig = np.asarray(sig, dtype=np.float32).reshape(B, -1)
        L = _L_of(noise)
        if L.shape[0] * self.m != u.shape[1]:
            raise ValueError("the noise shape's rows are not the horizon")
        if isinstance(epoch, torch.Tensor):
            epoch = int(epoch.reshape(-1)[0])
        lo, hi = (float(cost.u_min), float(cost.u_max)) if cost.has_u_bounds else (None, None)
        v = sample_tensor(u, sig, self.m, L, int(seed), int(epoch), int(iteration), int(problem_offset), int(samples), lo, hi)
        return self._out(v.reshape(B * samples, -1, self.m)), self._out(np.repeat(x0, samples, axis=0))
