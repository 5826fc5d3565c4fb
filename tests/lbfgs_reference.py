"""CPU restatement of the batched L-BFGS schedule of phnn_solve_lbfgs (TEST INFRASTRUCTURE).

lbfgs_schedule() runs B problems on the fixed slot schedule of the device solve: per outer step, max_iter slots, each
one batched evaluation of all B problems at their current iterates followed by the work of k_lbfgs for the problems
waiting on it (per-problem masks, a history ring buffer of (s, y) pairs).  The arithmetic is torch's own: every
per-problem operation is the tensor op torch/optim/lbfgs.py applies, on that problem's 1-D tensors, so the result
equals B separate torch.optim.LBFGS runs bit for bit (torch_lbfgs() below) when the evaluations agree.

evaluate(u (k, N) float32 CPU tensor, rows (k,) problem indices) -> (cost (k,) float32, grad (k, N) float32).
"""
from collections import Counter

import torch


def lbfgs_schedule(evaluate, u_init, lr, outer_steps, max_iter=20, max_eval=None, tolerance_grad=1e-7,
                   tolerance_change=1e-9, history_size=100):
    """-> dict(u_last (B,N), costs (outer_steps,B) orig_loss per step, n_iter (B), func_evals (B), reasons (Counter of
    how each step() ended, plus 'skip_update' for every history update dropped by ys <= 1e-10 and 'push' for every
    pair stored))"""
    reasons = Counter()
    if max_eval is None:
        max_eval = max_iter * 5 // 4
    u = u_init.detach().clone().to(torch.float32)
    B, N = u.shape
    hist = torch.zeros(B, history_size, 2, N)  # ring of (s, y) = (old_stps, old_dirs)
    ro = [[None] * history_size for _ in range(B)]
    count, head = [0] * B, [0] * B
    n_iter, func_evals = [0] * B, [0] * B
    d, t, H_diag = [None] * B, [None] * B, [1] * B
    prev_g, prev_loss = [None] * B, [None] * B
    it, evals, waiting = [0] * B, [0] * B, [False] * B
    costs = torch.empty(outer_steps, B)
    for k in range(outer_steps):
        for slot in range(max_iter):
            c, g_all = evaluate(u, list(range(B)))
            if slot == 0:
                costs[k] = c
            for b in range(B):
                if slot > 0 and not waiting[b]:
                    continue  # idle: this evaluation is ignored
                waiting[b] = False
                loss = float(c[b])
                flat_grad = g_all[b].clone()
                func_evals[b] += 1
                opt_cond = flat_grad.abs().max() <= tolerance_grad
                if slot == 0:
                    evals[b], it[b] = 1, 0
                    if opt_cond:
                        reasons["opt_cond_start"] += 1
                        continue
                else:
                    evals[b] += 1
                    why = ("max_eval" if evals[b] >= max_eval else "opt_cond" if opt_cond else
                           "small_step" if d[b].mul(t[b]).abs().max() <= tolerance_change else
                           "loss_change" if abs(loss - prev_loss[b]) < tolerance_change else None)
                    if why:
                        reasons[why] += 1
                        continue
                # ---- iteration body (torch/optim/lbfgs.py, step())
                it[b] += 1
                n_iter[b] += 1
                if n_iter[b] == 1:
                    d[b] = flat_grad.neg()
                    count[b], head[b] = 0, 0
                    H_diag[b] = 1
                else:
                    y = flat_grad.sub(prev_g[b])
                    s = d[b].mul(t[b])
                    ys = y.dot(s)
                    if ys > 1e-10:
                        hist[b, head[b], 0] = s
                        hist[b, head[b], 1] = y
                        ro[b][head[b]] = 1.0 / ys
                        head[b] = (head[b] + 1) % history_size
                        count[b] = min(count[b] + 1, history_size)
                        H_diag[b] = ys / y.dot(y)
                        reasons["push"] += 1
                    else:
                        reasons["skip_update"] += 1
                    cnt = count[b]
                    pos = [(head[b] - cnt + i) % history_size for i in range(cnt)]
                    al = [None] * cnt
                    q = flat_grad.neg()
                    for i in range(cnt - 1, -1, -1):
                        al[i] = hist[b, pos[i], 0].dot(q) * ro[b][pos[i]]
                        q.add_(hist[b, pos[i], 1], alpha=-al[i])
                    d[b] = r = torch.mul(q, H_diag[b])
                    for i in range(cnt):
                        be_i = hist[b, pos[i], 1].dot(r) * ro[b][pos[i]]
                        r.add_(hist[b, pos[i], 0], alpha=al[i] - be_i)
                prev_g[b] = flat_grad.clone()
                prev_loss[b] = loss
                t[b] = min(1.0, 1.0 / flat_grad.abs().sum()) * lr if n_iter[b] == 1 else lr
                gtd = flat_grad.dot(d[b])
                if gtd > -tolerance_change:
                    reasons["gtd"] += 1
                    continue
                u[b].add_(d[b], alpha=t[b])
                if it[b] != max_iter:
                    waiting[b] = True
                else:
                    reasons["max_iter"] += 1
    return {"u_last": u, "costs": costs, "n_iter": torch.tensor(n_iter, dtype=torch.int32),
            "func_evals": torch.tensor(func_evals, dtype=torch.int32), "reasons": reasons}


def torch_lbfgs(evaluate, u_init, lr, outer_steps, max_iter=20, max_eval=None, tolerance_grad=1e-7,
                tolerance_change=1e-9, history_size=100):
    """B separate torch.optim.LBFGS runs, problem b's closure = evaluate(u_b[None]).  Same return dict."""
    B, N = u_init.shape
    out_u, costs = torch.empty(B, N), torch.empty(outer_steps, B)
    n_iter, func_evals = [], []
    for b in range(B):
        x = u_init[b].detach().clone().to(torch.float32).requires_grad_(True)
        opt = torch.optim.LBFGS([x], lr=lr, max_iter=max_iter, max_eval=max_eval, tolerance_grad=tolerance_grad,
                                tolerance_change=tolerance_change, history_size=history_size)

        def closure():
            opt.zero_grad()
            c, g = evaluate(x.detach()[None], [b])
            x.grad = g[0].clone()
            return c[0].clone()

        for k in range(outer_steps):
            costs[k, b] = opt.step(closure)
        st = opt.state[x]
        out_u[b] = x.detach()
        n_iter.append(st.get("n_iter", 0))
        func_evals.append(st.get("func_evals", 0))
    return {"u_last": out_u, "costs": costs, "n_iter": torch.tensor(n_iter, dtype=torch.int32),
            "func_evals": torch.tensor(func_evals, dtype=torch.int32)}


def tanh_quadratic(B, N, seed=0, scale=1.0):
    """A smooth seeded test cost per problem: f(u) = sum_i a_i (u_i - c_i)^2 / 2 + w . tanh(u); float32 cost and
    gradient, evaluated row by row (no cross-problem reduction)."""
    g = torch.Generator().manual_seed(seed)
    a = (0.5 + 2.0 * torch.rand(B, N, generator=g)) * scale
    c = torch.randn(B, N, generator=g)
    w = torch.randn(B, N, generator=g)

    def evaluate(u, rows):
        cost = torch.empty(u.shape[0])
        grad = torch.empty_like(u)
        for j in range(u.shape[0]):
            b = int(rows[j])
            e = u[j] - c[b]
            th = torch.tanh(u[j])
            cost[j] = (a[b] * e * e).sum() * 0.5 + (w[b] * th).sum()
            grad[j] = a[b] * e + w[b] * (1 - th * th)
        return cost, grad

    return evaluate
