"""Time-correlated (shaped) sampling noise for the MPPI and CEM solves.

A noise shape is a matrix L (H, P), 1 <= P <= H, shared by the batch: per rollout the sampler draws P white normals per
control component, eps (P, m), and perturbs step t of component c with z[t, c] = sum_s L[t, s] eps[s, c] instead of an
independent normal (include/phnn_mpc.h: phnn_noise_shape).  When L's rows have unit Euclidean norm every z[t, c] has unit
variance, so sigma, CEM's refit of it and sigma_min keep their meaning.  The library does not normalise; the builders
here do.  Each builder computes in float64 and returns a float32 (H, P) array with unit-norm rows:

  ar1(H, rho)              AR(1) / Ornstein-Uhlenbeck noise: Cholesky factor of the covariance rho^|t - s|
  colored(H, beta)         power-law ("coloured") noise as in iCEM: Cholesky factor of the unit-diagonal Toeplitz covariance
                           whose spectrum falls as f^-beta; beta = 0 is white (the identity, exactly)
  knots(H, P, "linear")    P knots spread over the horizon and interpolated between: P normals drive H steps
  from_covariance(C)       Cholesky factor of a given (H, H) covariance (its correlation matrix: rows are normalised)
  normalize_rows(L)        any (H, P) matrix with its rows scaled to unit norm

Noise is the holder the engine, the solvers and the controllers pass around: the array, its device tensor and (H, P).  It
hashes by identity, so a captured graph (solver.GraphedMPPI / GraphedCEM) keys on the object and reads its device tensor
through the pointer it was captured with -- keep the object, and change the tensor in place if at all.
resolve() turns what a controller or a config gives (None, a Noise, {"type": ...}, an array) into an array for a horizon.

The last section restates the library's generator (csrc/phnn_rows.hip.h: Philox4x32-10, Box-Muller) in numpy float64 at
the counters of the extended plant step (include/phnn_mpc.h: phnn_plant_step_ex): plant_normals() gives the host plant
closed_loop.BatchedCartPole the force and measurement normals the device plant draws, up to float32 rounding.
"""
import numpy as np


def normalize_rows(L):
    """L (H, P) -> float32 (H, P) with rows of unit Euclidean norm (computed in float64)."""
    L = np.array(L, dtype=np.float64, ndmin=2)
    if L.ndim != 2 or L.shape[0] < 1 or not 1 <= L.shape[1] <= L.shape[0]:
        raise ValueError(f"a noise shape is (H, P) with 1 <= P <= H, got {L.shape}")
    if not np.all(np.isfinite(L)):
        raise ValueError("a noise shape must be finite")
    norm = np.sqrt((L * L).sum(axis=1, keepdims=True))
    if np.any(norm == 0):
        raise ValueError("a noise shape with a zero row cannot be normalised")
    return (L / norm).astype(np.float32)


def from_covariance(C):
    """C (H, H) symmetric positive definite -> the lower Cholesky factor of its correlation matrix, float32 (H, H)."""
    C = np.array(C, dtype=np.float64, ndmin=2)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or not np.allclose(C, C.T, rtol=0, atol=1e-12 * max(np.abs(C).max(), 1e-300)):
        raise ValueError(f"a covariance is a symmetric (H, H) matrix, got shape {C.shape}")
    try:
        L = np.linalg.cholesky(C)
    except np.linalg.LinAlgError as e:
        raise ValueError(f"the covariance is not positive definite: {e}") from None
    return normalize_rows(L)


def _check_horizon(H):
    if int(H) != H or H < 1:
        raise ValueError(f"horizon must be an integer >= 1, got {H!r}")
    return int(H)


def ar1(H, rho):
    """AR(1) noise z_t = rho z_{t-1} + sqrt(1 - rho^2) w_t in its stationary state: the Cholesky factor of rho^|t - s|.
    |rho| < 1; rho = 0 is white (the identity)."""
    H = _check_horizon(H)
    rho = float(rho)
    if not abs(rho) < 1:
        raise ValueError(f"ar1: |rho| must be < 1, got {rho}")
    t = np.arange(H)
    return from_covariance(rho ** np.abs(t[:, None] - t[None, :]))


def colored_covariance(H, beta):
    """The unit-diagonal Toeplitz covariance (H, H), float64, of noise with spectrum S(f) ~ f^-beta: r[tau] = sum_j S_j
    cos(2 pi j tau / M) / sum_j S_j on the periodic grid of M = 2H frequencies f_j = min(j, M - j) / M, the zero
    frequency given the weight of the lowest one (a principal block of a positive definite circulant matrix)."""
    H = _check_horizon(H)
    beta = float(beta)
    if not (beta >= 0 and np.isfinite(beta)):
        raise ValueError(f"colored: beta must be >= 0 and finite, got {beta}")
    M = 2 * H
    j = np.arange(M)
    f = np.minimum(j, M - j) / M
    f[0] = f[1]
    S = f ** -beta
    r = np.array([(S * np.cos(2 * np.pi * j * tau / M)).sum() for tau in range(H)]) / S.sum()
    t = np.arange(H)
    return r[np.abs(t[:, None] - t[None, :])]


def colored(H, beta):
    """Power-law noise: the Cholesky factor of colored_covariance(H, beta).  beta = 0: white, the identity exactly;
    1: pink; 2: red (Brownian-like).  Tested up to beta = 3 at H = 256."""
    H = _check_horizon(H)
    if float(beta) == 0.0:
        return np.eye(H, dtype=np.float32)
    return from_covariance(colored_covariance(H, beta))


def knot_steps(H, P):
    """The steps of the P knots: round(k (H - 1) / (P - 1)), distinct for P <= H; one knot sits at step 0."""
    H = _check_horizon(H)
    if int(P) != P or not 1 <= P <= H:
        raise ValueError(f"knots: 1 <= count <= H, got count = {P!r} at H = {H}")
    P = int(P)
    if P == 1:
        return np.zeros(1, dtype=np.int64)
    return np.floor(np.arange(P) * (H - 1) / (P - 1) + 0.5).astype(np.int64)


def knots(H, P, kind="linear"):
    """P knots at knot_steps(H, P), interpolated over the horizon: row t of L holds the interpolation weights of step t
    (at a knot step the unit vector of that knot, so z there is that knot's normal), rows normalised.  P = 1: one normal
    for the whole horizon.  kind: "linear"."""
    if kind != "linear":
        raise ValueError(f"knots: unknown kind {kind!r} (\"linear\")")
    steps = knot_steps(H, P)
    H, P = int(H), int(P)
    L = np.zeros((H, P))
    if P == 1:
        L[:, 0] = 1.0
        return normalize_rows(L)
    for k in range(P - 1):
        a, b = steps[k], steps[k + 1]
        for t in range(a, b + 1):
            w = (t - a) / (b - a)
            L[t, k], L[t, k + 1] = 1.0 - w, w
    return normalize_rows(L)


BUILDERS = {"ar1": lambda H, rho=0.9: ar1(H, rho), "colored": lambda H, beta=2.0: colored(H, beta),
            "knots": lambda H, count=8, kind="linear": knots(H, min(int(count), H) if int(count) == count else count, kind)}


class Noise:
    """Holder of one noise shape: .L the float32 (H, P) array, .H, .P, and .tensor(device) its device copy (made once
    per device and kept).  Hashable by identity."""

    def __init__(self, L):
        L = np.ascontiguousarray(np.array(L, dtype=np.float32, ndmin=2))
        if L.ndim != 2 or L.shape[0] < 1 or not 1 <= L.shape[1] <= L.shape[0] or not np.all(np.isfinite(L)):
            raise ValueError(f"a noise shape is a finite (H, P) matrix with 1 <= P <= H, got shape {L.shape}")
        self.L, (self.H, self.P) = L, L.shape
        self._dev = {}

    def tensor(self, device):
        import torch
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = torch.tensor(self.L, dtype=torch.float32, device=device).contiguous()
        return self._dev[device]

    def struct(self, device):
        """-> phnn_noise_shape pointing at tensor(device)."""
        from . import _capi
        s = _capi.NoiseShape()
        s.L_dev, s.rows, s.cols = self.tensor(device).data_ptr(), self.H, self.P
        return s

    def __repr__(self):
        return f"Noise(H={self.H}, P={self.P})"


def resolve(spec, H):
    """What a controller or the `mpc.noise` config key holds -> Noise for horizon H, or None.  spec: None; a Noise;
    {"type": "ar1", "rho": 0.9} | {"type": "colored", "beta": 2.0} | {"type": "knots", "count": 8[, "kind": "linear"]};
    or an (H, P) array, used as given (normalize_rows is the caller's).  ValueError for an unknown type or a shape whose
    row count is not H."""
    if spec is None:
        return None
    if isinstance(spec, dict):
        kw = dict(spec)
        kind = kw.pop("type", None)
        if kind not in BUILDERS:
            raise ValueError(f"unknown noise type {kind!r}: one of {sorted(BUILDERS)}")
        try:
            spec = BUILDERS[kind](int(H), **kw)
        except TypeError as e:
            raise ValueError(f"noise type {kind!r}: {e}") from None
    noise = spec if isinstance(spec, Noise) else Noise(spec)
    if noise.H != int(H):
        raise ValueError(f"the noise shape has {noise.H} rows, the horizon is {H}")
    return noise


# ----------------------------------------------------------------------------- the library's generator, in float64
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10: ctr (..., 4), key (2,) unsigned 32-bit values -> (..., 4) uint32."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) & _MASK for i in range(4)]
    k = [np.uint64(int(key[i]) & 0xFFFFFFFF) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> _32) ^ c[1] ^ k[0], p1 & _MASK, (p0 >> _32) ^ c[3] ^ k[1], p0 & _MASK]
        k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def _unit(x):
    """top 24 bits -> (0, 1]: (n + 0.5) * 2^-24"""
    return ((x >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def _box_muller(a, b):
    r = np.sqrt(-2.0 * np.log(_unit(a)))
    ang = np.pi * (2.0 * _unit(b))
    return r * np.cos(ang), r * np.sin(ang)


def plant_normals(seed, step, gids, j):
    """The four float64 normals of float4 j (0: component 0 is the force normal z0; 1: the measurement normals) of the
    plants with global ids `gids` at control step `step`: one Philox call each, key = seed, counter (gid & 0xffffffff,
    gid >> 32, step, 1 << 6 | j) -- sample 1 of problem gid at (epoch = step, iteration = 0) in the sampler's layout
    (csrc/phnn_sampling.h).  -> (len(gids), 4)."""
    g = np.asarray(gids, dtype=np.int64).reshape(-1)
    if np.any(g < 0) or np.any(g >= 1 << 48) or j not in (0, 1):
        raise ValueError("plant_normals: 0 <= gid < 2^48, j in (0, 1)")
    g = g.astype(np.uint64)
    step = np.uint64(int(step) & 0xFFFFFFFF)  # the int32 step's bit pattern
    ctr = np.stack([g & _MASK, g >> _32, np.full_like(g, step), np.full_like(g, (1 << 6) | j)], axis=-1)
    o = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    z = np.empty(o.shape, np.float64)
    z[:, 0], z[:, 1] = _box_muller(o[:, 0], o[:, 1])
    z[:, 2], z[:, 3] = _box_muller(o[:, 2], o[:, 3])
    return z
