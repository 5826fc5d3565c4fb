"""The float32 model of K3 (k_adam + k_best_cost, phnn_kernels.hip.h): one Adam step on the controls in the operation
order of torch.optim.Adam's single-tensor path, the best-iterate tracking of src/mpc_controller_canonical.py:208-214, and
the loop of phnn_solve around them.  TEST INFRASTRUCTURE (no tests in here): tests/test_adam_model.py pins it on the CPU,
tests/test_gpu_adam_kernel.py pins the kernels to it bit for bit.

  step        oracle_adam_f32 / oracle_adam_f64 of oracle/phnn_oracle.c (chosen by the dtype of u)
  step_numpy  the same arithmetic in NumPy, one rounding per line, with an exact fused multiply-add; every intermediate
              can be read back (trace=True), so a device mismatch can be narrowed down to one operation
  track       best-iterate tracking of one iteration
  solve       phnn_solve / solver.shooting_solve over a caller-supplied cost and gradient function

Hyper-parameters: torch hands lr, betas and eps to the step as Python floats (doubles), and so do step / step_numpy /
solve.  phnn_adam_step takes them as C floats and widens them back, so the kernel sees float_arg(0.9), not 0.9 (its
lerp weight is 3 ulp and its 1 - beta2 110 ulp from torch's): a comparison with the device passes every one of them
through float_arg first.
"""
import ctypes as C
import math

import numpy as np

import oracle_lib as ol


def float_arg(x):
    """What a C float argument makes of a Python float (phnn_adam_step, phnn_solve_options), as a Python float."""
    return float(np.float32(x))


def step(u, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8):
    """One Adam step by the oracle.  u, g, m, v: arrays of one dtype (float32 or float64) and size; `step` is 1-based.
    -> (u, m, v) as new arrays of u's shape; the arguments are left alone."""
    dt = np.dtype(u.dtype)
    suf = {np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[dt]
    for a in (g, m, v):
        assert a.dtype == dt and a.size == u.size
    g = np.ascontiguousarray(g)
    u, m, v = (np.array(a, dtype=dt, order="C", copy=True) for a in (u, m, v))
    getattr(ol.lib(), f"oracle_adam_{suf}")(u.ctypes.data_as(C.c_void_p), g.ctypes.data_as(C.c_void_p),
                                            m.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), u.size,
                                            float(lr), float(beta1), float(beta2), float(eps), int(step))
    return u, m, v


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays.  The float64 product of two float32 numbers is exact; the
    float64 sum is not, and rounding it twice (to float64, then to float32) can land on the wrong side of a float32
    tie.  So the sum is rounded to odd: where it is inexact (two-sum error != 0) and its last mantissa bit is even, it
    moves one float64 ulp towards the error.  A float64 rounded to odd carries 53 >= 24 + 2 bits, which makes the
    final rounding to float32 the correct one."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def host_constants(lr, step, beta1, beta2, eps):
    """The scalars phnn_adam_step / oracle_adam_f32 hand to the element-wise arithmetic: bias corrections in double (they
    are Python floats in torch/optim/adam.py), rounded to float32 once."""
    bc1 = 1.0 - math.pow(beta1, float(step))
    bc2 = 1.0 - math.pow(beta2, float(step))
    return {"w1": np.float32(1.0 - beta1), "w2": np.float32(1.0 - beta2), "b2": np.float32(beta2),
            "bc2s": np.float32(math.sqrt(bc2)), "step_neg": np.float32(-(lr / bc1)), "eps": np.float32(eps)}


def step_numpy(u, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, trace=False):
    """The float32 step in NumPy, one IEEE operation per line.  -> (u, m, v), or with trace a dict of every
    intermediate (d, m, t1, t2, t3, v, s, q, denom, n, r, u)."""
    k = host_constants(lr, step, beta1, beta2, eps)
    u, g, m, v = (np.asarray(a, np.float32) for a in (u, g, m, v))
    with np.errstate(all="ignore"):
        d = g - m
        m1 = fma32(k["w1"], d, m)   # exp_avg.lerp_(g, 1 - beta1): m + w1 * (g - m), fused
        t1 = v * k["b2"]            # exp_avg_sq.mul_(beta2)
        t2 = k["w2"] * g            # .addcmul_(g, g, value = 1 - beta2): (w2 * g) * g
        t3 = t2 * g
        v1 = t1 + t3
        s = np.sqrt(v1)
        q = s / k["bc2s"]
        denom = q + k["eps"]
        n = k["step_neg"] * m1      # param.addcdiv_(exp_avg, denom, value = -lr / bc1)
        r = n / denom
        u1 = u + r
    if trace:
        return {"d": d, "m": m1, "t1": t1, "t2": t2, "t3": t3, "v": v1, "s": s, "q": q, "denom": denom, "n": n, "r": r,
                "u": u1}
    return u1, m1, v1


def track(u, cost, best_cost, best_u, per, u_min=None, u_max=None, has_bounds=False):
    """Best-iterate tracking of one iteration, in place on best_cost (B) and best_u (B * per entries): where cost[b] <
    best_cost[b] (strict; false for a NaN on either side), row b of best_u becomes clamp(u_b) -- u being the iterate that
    produced the cost, before its Adam step; a NaN entry stays NaN as in torch.clamp -- and best_cost[b] becomes cost[b].
    Every other row is left untouched.  -> the mask of the rows that improved."""
    B = best_cost.shape[0]
    rows = np.asarray(u).reshape(B, per)
    with np.errstate(invalid="ignore"):
        better = np.asarray(cost) < best_cost
        if has_bounds:
            lo, hi = rows.dtype.type(u_min), rows.dtype.type(u_max)
            rows = np.minimum(np.maximum(rows, lo), hi)  # both propagate NaN
    best_u.reshape(B, per)[better] = rows[better]
    best_cost[better] = np.asarray(cost)[better]
    return better


def solve(cost_grad, u0, lr, iters, beta1=0.9, beta2=0.999, eps=1e-8, track_best=False, u_min=None, u_max=None,
          record_costs=True, step_fn=step):
    """The loop of phnn_solve: zero optimizer state, best_cost = +inf, best_u = 0; `iters` times { cost and gradient of
    the current iterate; cost history; tracking on the iterate and best_cost from before the step; Adam step k + 1 }.
    cost_grad(u (B,H,m)) -> (cost (B), grad (B,H,m)) in u0's dtype.  -> dict(u_last, costs | None[, best_u, best_cost])."""
    u = np.array(u0, order="C", copy=True)
    dt = u.dtype
    B = u.shape[0]
    per = u[0].size
    m, v = np.zeros_like(u), np.zeros_like(u)
    costs = np.empty((iters, B), dt) if record_costs else None
    best_cost = np.full(B, np.inf, dt) if track_best else None
    best_u = np.zeros_like(u) if track_best else None
    has_b = u_min is not None and u_max is not None
    for k in range(iters):
        c, g = cost_grad(u)
        c, g = np.asarray(c, dt), np.ascontiguousarray(np.asarray(g, dt).reshape(u.shape))
        if record_costs:
            costs[k] = c
        if track_best:
            track(u, c, best_cost, best_u, per, u_min, u_max, has_b)
        u, m, v = (a.reshape(u.shape) for a in step_fn(u, g, m, v, lr, k + 1, beta1, beta2, eps))
    out = {"u_last": u, "costs": costs}
    if track_best:
        out["best_u"], out["best_cost"] = best_u, best_cost
    return out
