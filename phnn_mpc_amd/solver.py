"""Batched single-shooting solve: Adam on the control sequences of B independent MPC problems.

Host logic shared by both controller classes.  It restates the optimisation loops of the reference
  src/mpc_controller.py:164-209            (cold start zeros, Adam, returns the LAST iterate, clamped)
  src/mpc_controller_canonical.py:163-228  (optional warm start, Adam, returns the BEST clamped iterate; the cost
                                            of iterate k is measured before step k is applied, strict '<')
for B problems at once: Adam is element-wise, so B stacked problems of shape (H,m) behave exactly like B
separate torch.optim.Adam instances.  All arithmetic is delegated to an engine object (RolloutEngine on the
GPU): rollout_cost_grad (K1+K2) and adam_step (K3).
"""
import ctypes

import torch


def _need_reference(engine, x_ref):
    if x_ref is not None and not getattr(engine, "supports_reference", False):
        raise NotImplementedError(f"{type(engine).__name__} has no reference tracking (x_ref): RolloutEngine has")


def shooting_solve(engine, x0, u_init, cost, integrator, dt, lr, iters, track_best=False, u_min=None, u_max=None,
                   record_costs=True, x_ref=None, ref_offset=0):
    """x0 (B,n), u_init (B,H,m) on engine.device -> dict(u_last, costs[, best_u, best_cost]).

    u_last   : unclamped last iterate (B,H,m)
    costs    : (iters,B) cost of each iterate (measured before its Adam step), if record_costs
    best_u   : clamped best iterate (track_best)
    x_ref    : reference trajectory broadcastable to (B, rows, n), tracked from row ref_offset (int or device int32
               tensor) on (RolloutEngine.rollout_cost); None: the cost's x_target
    """
    _need_reference(engine, x_ref)
    rkw = {} if x_ref is None else {"x_ref": x_ref, "ref_offset": ref_offset}
    dev = x0.device
    u = u_init.detach().clone().contiguous()
    exp_avg = torch.zeros_like(u)
    exp_avg_sq = torch.zeros_like(u)
    B = u.shape[0]
    costs = torch.empty(iters, B, dtype=torch.float32, device=dev) if record_costs else None
    best_cost = best_u = None
    if track_best:
        best_cost = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
        best_u = torch.zeros_like(u)
    ws = {}
    for k in range(iters):
        c, g = engine.rollout_cost_grad(x0, u, cost, integrator, dt, workspace=ws, **rkw)
        if record_costs:
            costs[k].copy_(c)
        engine.adam_step(u, g, exp_avg, exp_avg_sq, lr, k + 1, cost=c if track_best else None, best_cost=best_cost,
                         best_u=best_u, u_min=u_min, u_max=u_max)
    out = {"u_last": u, "costs": costs}
    if track_best:
        out["best_u"], out["best_cost"] = best_u, best_cost
    return out


def _eager(engine, x0, u_init, cost, integrator, dt, lr, iters, track_best=False, u_min=None, u_max=None, record_costs=True,
           x_ref=None, ref_offset=0):
    """The solve without a captured graph: the library's own loop (phnn_solve: one call enqueues every launch) when the
    engine has one and the Adam-side bounds are the cost's (they are for both controller classes); else the Python loop.
    Same launches, same order: identical results.  x_ref / ref_offset: see shooting_solve."""
    _need_reference(engine, x_ref)
    rkw = {} if x_ref is None else {"x_ref": x_ref, "ref_offset": ref_offset}
    has_b = u_min is not None and u_max is not None
    same = bool(cost.has_u_bounds) == has_b and (not has_b or (float(cost.u_min) == float(ctypes.c_float(u_min).value)
                                                                and float(cost.u_max) == float(ctypes.c_float(u_max).value)))
    if hasattr(engine, "solve") and same:
        return engine.solve(x0, u_init, cost, integrator, dt, lr=lr, iters=iters, track_best=track_best, record_costs=record_costs,
                            **rkw)
    return shooting_solve(engine, x0, u_init, cost, integrator, dt, lr, iters, track_best=track_best, u_min=u_min, u_max=u_max,
                          record_costs=record_costs, **rkw)


def solver_for(engine, use_graph, previous=None):
    """-> callable(engine, x0, u_init, cost, ...) : shooting_solve, or a GraphedSolve bound to `engine` (reused from
    `previous` when it already is one for this engine)."""
    if not use_graph or engine.device.type != "cuda":
        return _eager
    if isinstance(previous, GraphedSolve) and previous.engine is engine:
        return previous
    return GraphedSolve(engine)


class GraphedSolve:
    """shooting_solve captured once as a HIP graph (all `iters` x (K1, K2, K3) launches plus the state resets) and
    replayed per call: one graph launch per MPC solve instead of 3 x iters kernel launches through Python.  Worth it
    where the solve is launch-bound -- the reference's own use, one plant (or a few) per call in a closed loop.

    The graph is tied to (B, H, m, iters, cost struct, integrator, dt, lr, flags); a call with another signature
    re-captures.  Inputs are copied into the graph's static buffers, results are returned as fresh tensors.
    Same kernels, same order, same arithmetic as shooting_solve: results are bit-identical.

    Reference tracking (x_ref, ref_offset): the graph reads the reference through the pointer it was captured with.
    That pointer is a static buffer of the graph, (1 | B, rows, n) as reference_view leaves it before broadcasting,
    and every call copies the caller's x_ref (and ref_offset, int or device int32 tensor) into it: a reference of
    another shape re-captures, one updated in place is seen by the next call.  The static buffer stays alive as long
    as this object holds the graph.
    """

    def __init__(self, engine):
        self.engine = engine
        self.key = None
        self.graph = None

    def _signature(self, x0, u_init, cost, integrator, dt, lr, iters, track_best, u_min, u_max, record_costs, ref=None):
        key = (tuple(x0.shape), tuple(u_init.shape), bytes(ctypes.string_at(ctypes.addressof(cost), ctypes.sizeof(cost))),
               integrator, float(dt), float(lr), int(iters), bool(track_best), u_min, u_max, bool(record_costs))
        return key if ref is None else key + (tuple(ref.shape),)

    def _compact_reference(self, x_ref, B, n):
        """x_ref -> the (1 | B, rows, 1 | n) tensor reference_view broadcasts from (what the static buffer holds)."""
        from .engine import reference_view
        t, bs, ts, rows = reference_view(x_ref, B, n, self.engine.device)
        t = t[:1] if bs == 0 else t
        t = t[:, :1] if ts == 0 else t
        return t

    def _capture(self, x0, u_init, cost, integrator, dt, lr, iters, track_best, u_min, u_max, record_costs, ref=None):
        eng, dev = self.engine, x0.device
        self.x0 = x0.detach().clone().contiguous()
        self.u_init = u_init.detach().clone().contiguous()
        self.u = torch.empty_like(self.u_init)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.u), torch.zeros_like(self.u)
        B = self.u.shape[0]
        self.costs = torch.empty(iters, B, dtype=torch.float32, device=dev) if record_costs else None
        self.best_cost = torch.empty(B, dtype=torch.float32, device=dev) if track_best else None
        self.best_u = torch.empty_like(self.u) if track_best else None
        self.ws = {}
        rkw = {}
        if ref is not None:
            self.x_ref = ref.clone()
            self.ref_offset = torch.zeros(1, dtype=torch.int32, device=dev)
            rkw = {"x_ref": self.x_ref, "ref_offset": self.ref_offset}

        def body():
            self.u.copy_(self.u_init)
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            if track_best:
                self.best_cost.fill_(float("inf"))
                self.best_u.zero_()
            for k in range(iters):
                c, g = eng.rollout_cost_grad(self.x0, self.u, cost, integrator, dt, workspace=self.ws, **rkw)
                if record_costs:
                    self.costs[k].copy_(c)
                eng.adam_step(self.u, g, self.exp_avg, self.exp_avg_sq, lr, k + 1, cost=c if track_best else None,
                              best_cost=self.best_cost, best_u=self.best_u, u_min=u_min, u_max=u_max)

        # one eager pass on a side stream first: allocates the workspace outside the capture
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            body()

    def __call__(self, engine, x0, u_init, cost, integrator, dt, lr, iters, track_best=False, u_min=None, u_max=None,
                 record_costs=True, x_ref=None, ref_offset=0):
        assert engine is self.engine
        _need_reference(engine, x_ref)
        ref = None if x_ref is None else self._compact_reference(x_ref, x0.shape[0], engine.n)
        key = self._signature(x0, u_init, cost, integrator, dt, lr, iters, track_best, u_min, u_max, record_costs, ref)
        if key != self.key:
            self.key = None
            self._capture(x0, u_init, cost, integrator, dt, lr, iters, track_best, u_min, u_max, record_costs, ref)
            self.key = key
        self.x0.copy_(x0)
        self.u_init.copy_(u_init)
        if ref is not None:
            self.x_ref.copy_(ref)
            if isinstance(ref_offset, torch.Tensor):
                self.ref_offset.copy_(ref_offset.reshape(-1)[:1])
            elif int(ref_offset) < 0:
                raise ValueError("ref_offset < 0")
            else:
                self.ref_offset.fill_(int(ref_offset))
        self.graph.replay()
        out = {"u_last": self.u.clone(), "costs": self.costs.clone() if record_costs else None}
        if track_best:
            out["best_u"], out["best_cost"] = self.best_u.clone(), self.best_cost.clone()
        return out


def lbfgs_solver_for(engine, use_graph, previous=None):
    """-> callable(**solve_lbfgs arguments) -> dict(u_last, costs, n_iter, func_evals): engine.solve_lbfgs, or a
    GraphedLBFGS bound to `engine` (reused from `previous` when it already is one for this engine)."""
    if not hasattr(engine, "solve_lbfgs"):
        raise NotImplementedError(f"{type(engine).__name__} has no batched L-BFGS solve (RolloutEngine has): use "
                                  "compute_control (one plant at a time)")
    if not use_graph or engine.device.type != "cuda":
        return engine.solve_lbfgs
    if isinstance(previous, GraphedLBFGS) and previous.engine is engine:
        return previous
    return GraphedLBFGS(engine)


class GraphedLBFGS:
    """engine.solve_lbfgs captured once as a HIP graph (the state reset plus every outer_steps x max_iter x (K1, K2,
    k_lbfgs) launch) and replayed per call.  Tied to (B, H, m, cost struct, integrator, dt and the L-BFGS options); a
    call with another signature re-captures.  Inputs are copied into the graph's static buffers, results are returned
    as fresh tensors; same launches in the same order as the eager call: identical results.  x_ref / ref_offset as in
    GraphedSolve (a static reference buffer; another shape re-captures)."""

    def __init__(self, engine):
        self.engine = engine
        self.key = None
        self.graph = None

    def _capture(self, x0, u_init, cost, kw, ref):
        eng, dev = self.engine, x0.device
        self.x0 = x0.detach().clone().contiguous()
        self.u_init = u_init.detach().clone().contiguous()
        self.ws = {}
        rkw = {}
        if ref is not None:
            self.x_ref = ref.clone()
            self.ref_offset = torch.zeros(1, dtype=torch.int32, device=dev)
            rkw = {"x_ref": self.x_ref, "ref_offset": self.ref_offset}
        # one eager pass on a side stream first: allocates the workspace outside the capture
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            eng.solve_lbfgs(self.x0, self.u_init, cost, workspace=self.ws, **kw, **rkw)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = eng.solve_lbfgs(self.x0, self.u_init, cost, workspace=self.ws, **kw, **rkw)

    def __call__(self, x0, u_init, cost, integrator="euler", dt=0.02, lr=1.0, outer_steps=1, max_iter=20, max_eval=None,
                 tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100, record_costs=True, workspace=None,
                 x_ref=None, ref_offset=0):
        kw = dict(integrator=integrator, dt=float(dt), lr=float(lr), outer_steps=int(outer_steps), max_iter=int(max_iter),
                  max_eval=max_eval, tolerance_grad=float(tolerance_grad), tolerance_change=float(tolerance_change),
                  history_size=int(history_size), record_costs=bool(record_costs))
        ref = None
        if x_ref is not None:
            ref = GraphedSolve._compact_reference(self, x_ref, x0.shape[0], self.engine.n)
        key = (tuple(x0.shape), tuple(u_init.shape), bytes(ctypes.string_at(ctypes.addressof(cost), ctypes.sizeof(cost))),
               tuple(sorted(kw.items())), None if ref is None else tuple(ref.shape))
        if key != self.key:
            self.key = None
            self._capture(x0, u_init, cost, kw, ref)
            self.key = key
        self.x0.copy_(x0)
        self.u_init.copy_(u_init)
        if ref is not None:
            self.x_ref.copy_(ref)
            if isinstance(ref_offset, torch.Tensor):
                self.ref_offset.copy_(ref_offset.reshape(-1)[:1])
            elif int(ref_offset) < 0:
                raise ValueError("ref_offset < 0")
            else:
                self.ref_offset.fill_(int(ref_offset))
        self.graph.replay()
        return {k: (None if v is None else v.clone()) for k, v in self.out.items()}
