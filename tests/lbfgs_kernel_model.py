"""Bit-exact float32 model of k_lbfgs and the slot loop of phnn_solve_lbfgs (TEST INFRASTRUCTURE).

lbfgs_reference.lbfgs_schedule() restates the schedule with torch's own tensor ops, so it equals torch.optim.LBFGS but
only approaches the device to rounding: torch's dot products sum in another order.  kernel_schedule() below restates
phnn_lbfgs.hip operation by operation instead, in NumPy float32, so that fed the same K1 / K2 evaluations it equals the
device bit for bit.  What that rests on:

  * phnn_lbfgs.hip is built with -ffp-contract=off: every a + b*c is a rounded product and a rounded sum.  The only
    FMAs in the code object are those inside the three correctly rounded divisions (1/ys, ys/(y.y), 1/sum|g|), and
    NumPy's float32 division is correctly rounded too (tests/test_static_isa.py pins this on the ISA).
  * Every length-N vector is padded to Np = 4*ceil(N/4) floats in memory and to E4*64 floats in registers; lane l of a
    problem's 16 lanes holds float4 l + 16k (k < E4).  Here a vector is an array (B, E4, 16 lanes, 4).  vload() gives
    zeros past Np, eload() zeros past N, and register values past Np (e.g. the -0 of d = -g) never reach memory.
  * dot(): each lane sums its products serially from 0.f, float4 k = 0, 1, ... and components x, y, z, w, padding
    included; row_sum() then adds the 16 lane sums as the DPP butterfly does, a pairwise tree
    ((l0+l1)+(l2+l3)) + ((l4+l5)+(l6+l7)), halves added last.  No np.sum / np.dot anywhere.
  * Scalars (t, H_diag, ro, al, be, ys, gtd) are float32; the loss is the float32 cost widened to double and
    |loss - prev_loss| < tolerance_change is taken in double.  lr, tolerance_grad and tolerance_change are compared as
    float32, ys against float32(1e-10).

Same signature and return dict as lbfgs_schedule (plus 'pushes', the number of pairs stored per problem); evaluate() is
called once per slot with all B rows.
"""
from collections import Counter

import numpy as np
import torch

F32 = np.float32
LANES = 16


def kernel_e4(N):
    """float4 per lane of the k_lbfgs<E4> instantiation lbfgs_launch picks for N = H*m (0: refused, N > 256)."""
    nv4 = (N + 3) // 4
    for e4 in (1, 2, 3, 4):
        if nv4 <= e4 * LANES:
            return e4
    return 0


def to_lanes(flat, E4):
    """(B, n <= E4*64) row-major -> (B, E4, 16, 4), zero padded (element e = 4*(lane + 16k) + c)."""
    B, n = flat.shape
    out = np.zeros((B, E4 * LANES * 4), F32)
    out[:, :n] = flat
    return out.reshape(B, E4, LANES, 4)


def row_sum(v):
    """row_sum(): the DPP butterfly quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror over the 16
    lane values (B, 16) -> (B,); as a tree, neighbours first, halves last."""
    for _ in range(4):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def dot(a, b):
    """dot(): s = 0.f; s = s + a.x*b.x; ... per lane over k, then row_sum."""
    s = np.zeros(a.shape[:1] + (LANES,), F32)
    for k in range(a.shape[1]):
        for c in range(4):
            s = s + a[:, k, :, c] * b[:, k, :, c]
    return row_sum(s)


def abs_sum(g):
    """The first step length's sa = sa + |x| + |y| + |z| + |w| per lane, then row_sum."""
    s = np.zeros(g.shape[:1] + (LANES,), F32)
    for k in range(g.shape[1]):
        for c in range(4):
            s = s + np.abs(g[:, k, :, c])
    return row_sum(s)


def axpy(a, alpha, b):
    """axpy(): a + alpha*b, a rounded product and a rounded sum (alpha per problem)."""
    return a + alpha[:, None, None, None] * b


def abs_max(a, c):
    """abs_max(): NaN-propagating max of |a*c| from 0.f (nmax, row_max); the product is rounded before the abs."""
    m = np.abs(a * c[:, None, None, None]).reshape(a.shape[0], -1).max(axis=1, initial=F32(0))
    return m.astype(F32)


def kernel_schedule(evaluate, u_init, lr, outer_steps, max_iter=20, max_eval=None, tolerance_grad=1e-7,
                    tolerance_change=1e-9, history_size=100):
    """-> dict(u_last (B,N), costs (outer_steps,B), n_iter (B), func_evals (B), pushes (B), reasons) as
    lbfgs_reference.lbfgs_schedule, computed as k_lbfgs computes it."""
    reasons = Counter()
    if max_eval is None or max_eval == 0:
        max_eval = max_iter * 5 // 4  # phnn_solve_lbfgs: max_eval 0 -> torch's default
    u = u_init.detach().cpu().to(torch.float32).numpy().copy()
    B, N = u.shape
    E4, hs = kernel_e4(N), history_size
    assert E4 > 0, "k_lbfgs holds N = H*m <= 256"
    nv4 = (N + 3) // 4
    j4 = (np.arange(E4)[:, None] * LANES + np.arange(LANES)[None, :])[None, :, :, None]  # float4 index lane + 16k
    in_row = j4 < nv4  # vload / vstore: float4s inside the Np-float row
    lr32, tol_grad, tol_change = F32(lr), F32(tolerance_grad), F32(tolerance_change)
    ys_min, one = F32(1e-10), F32(1.0)
    rows = np.arange(B)

    def vload(v):
        return np.where(in_row, v, F32(0))

    # the workspace (memory) and the per-problem LbfgsState, zeroed by the state reset
    d_mem = np.zeros((B, E4, LANES, 4), F32)
    pg_mem = np.zeros_like(d_mem)
    hist = np.zeros((B, hs, 2, E4, LANES, 4), F32)  # entry e: (s, y)
    ro_mem = np.zeros((B, hs), F32)
    al_mem = np.zeros((B, hs), F32)
    n_iter, func_evals, it, evals = (np.zeros(B, np.int64) for _ in range(4))
    status, count, head, pushes = (np.zeros(B, np.int64) for _ in range(4))
    t_st, hdiag_st = np.zeros(B, F32), np.zeros(B, F32)
    prev_loss = np.zeros(B, np.float64)
    costs = np.zeros((outer_steps, B), F32)

    def count_reasons(name, mask):
        if mask.any():
            reasons[name] += int(mask.sum())

    for k_out in range(outer_steps):
        for slot in range(max_iter):
            c, g_all = evaluate(torch.from_numpy(u.copy()), list(range(B)))
            cost = c.detach().cpu().to(torch.float32).numpy().reshape(B)
            run = np.ones(B, bool) if slot == 0 else status == 1  # idle problems leave k_lbfgs at once
            # ---- consume this slot's evaluation (eload: zeros past N)
            g = to_lanes(g_all.detach().cpu().to(torch.float32).numpy().reshape(B, N), E4)
            loss = cost.astype(np.float64)
            func_evals += run
            opt_cond = abs_max(g, np.ones(B, F32)) <= tol_grad
            if slot == 0:
                costs[k_out] = cost
                evals[:] = 1
                it[:] = 0
                stop = opt_cond.copy()
                count_reasons("opt_cond_start", stop)
                d = vload(d_mem)  # only read where n_iter > 0; zeros (never stored) otherwise
            else:
                evals += run
                d = vload(d_mem)
                r_eval = run & (evals >= max_eval)
                r_opt = run & ~r_eval & opt_cond
                r_small = run & ~r_eval & ~r_opt & (abs_max(d, t_st) <= tol_change)
                r_loss = run & ~r_eval & ~r_opt & ~r_small & (np.abs(loss - prev_loss) < tolerance_change)
                for name, msk in (("max_eval", r_eval), ("opt_cond", r_opt), ("small_step", r_small),
                                  ("loss_change", r_loss)):
                    count_reasons(name, msk)
                stop = r_eval | r_opt | r_small | r_loss
            body = run & ~stop
            # ---- the next iteration body, for the problems in `body`
            it += body
            n_iter += body
            first = body & (n_iter == 1)
            later = body & (n_iter > 1)
            d = np.where(first[:, None, None, None], g * F32(-1.0), d)  # scale(d, g, -1.0f)
            hdiag_st = np.where(first, one, hdiag_st)
            count = np.where(first, 0, count)
            head = np.where(first, 0, head)
            if later.any():
                y = g - vload(pg_mem)
                s = d * t_st[:, None, None, None]  # scale(s, d, st.t): last step's direction and length
                ys = dot(y, s)
                push = later & (ys > ys_min)
                count_reasons("skip_update", later & ~push)
                count_reasons("push", push)
                pushes += push
                if push.any():
                    pb, pos = rows[push], head[push]
                    hist[pb, pos, 0] = np.where(in_row[0], s[push], hist[pb, pos, 0])  # vstore
                    hist[pb, pos, 1] = np.where(in_row[0], y[push], hist[pb, pos, 1])
                    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
                        ro_mem[pb, pos] = one / ys[push]
                        hdiag_st = np.where(push, ys / np.where(push, dot(y, y), one), hdiag_st)
                    head = np.where(push, np.where(head + 1 == hs, 0, head + 1), head)
                    count = np.where(push, np.minimum(count + 1, hs), count)
                # two-loop recursion; entry i (0 = oldest) sits at ring position (head - count + i) mod hs
                cnt = np.where(later, count, 0)
                base = (head - cnt) % hs
                q = g * F32(-1.0)  # scale(q, g, -1.0f)
                for i in range(int(cnt.max()) - 1, -1, -1):  # newest -> oldest
                    act = i < cnt
                    pos = (base + i) % hs
                    s_i, y_i, ro_i = hist[rows, pos, 0], hist[rows, pos, 1], ro_mem[rows, pos]
                    a = dot(s_i, q) * ro_i
                    al_mem[act, i] = a[act]
                    q = np.where(act[:, None, None, None], axpy(q, -a, y_i), q)
                r = q * hdiag_st[:, None, None, None]  # scale(d, q, st.hdiag)
                for i in range(int(cnt.max())):  # oldest -> newest
                    act = i < cnt
                    pos = (base + i) % hs
                    s_i, y_i, ro_i = hist[rows, pos, 0], hist[rows, pos, 1], ro_mem[rows, pos]
                    be = dot(y_i, r) * ro_i
                    r = np.where(act[:, None, None, None], axpy(r, al_mem[:, i] - be, s_i), r)
                d = np.where(later[:, None, None, None], r, d)
            bm = body[:, None, None, None]
            pg_mem = np.where(bm & in_row, g, pg_mem)  # prev_flat_grad.copy_(flat_grad)
            prev_loss = np.where(body, loss, prev_loss)
            with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
                r1 = one / abs_sum(g)  # t = min(1., 1. / flat_grad.abs().sum()) * lr on the first iteration ever
            t = np.where(n_iter == 1, np.where(r1 < one, r1, one) * lr32, lr32).astype(F32)
            t_st = np.where(body, t, t_st)
            d_mem = np.where(bm & in_row, d, d_mem)
            gtd = dot(g, d)
            r_gtd = body & (gtd > -tol_change)
            count_reasons("gtd", r_gtd)
            move = body & ~r_gtd
            step = (u + t_st[:, None] * d.reshape(B, -1)[:, :N]).astype(F32)  # u += t*d, e < N only
            u = np.where(move[:, None], step, u)
            r_iter = move & (it == max_iter)
            count_reasons("max_iter", r_iter)
            stop_now = (run & stop) | r_gtd | r_iter
            status = np.where(run, np.where(stop_now, 0, 1), status)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    return {"u_last": torch.from_numpy(u), "costs": torch.from_numpy(costs), "n_iter": i32(n_iter),
            "func_evals": i32(func_evals), "pushes": i32(pushes), "reasons": reasons}
