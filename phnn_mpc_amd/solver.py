"""Batched single-shooting solve: Adam on the control sequences of B independent MPC problems.

Host logic shared by both controller classes.  It restates the optimisation loops of the reference
  src/mpc_controller.py:164-209            (cold start zeros, Adam, returns the LAST iterate, clamped)
  src/mpc_controller_canonical.py:163-228  (optional warm start, Adam, returns the BEST clamped iterate; the cost
                                            of iterate k is measured before step k is applied, strict '<')
for B problems at once: Adam is element-wise, so B stacked problems of shape (H,m) behave exactly like B
separate torch.optim.Adam instances.  All arithmetic is delegated to an engine object.  On a RolloutEngine the loop
is the library's (engine.solve: phnn_solve enqueues K1, K2, K3 of every iteration); shooting_solve is the same loop
in Python over rollout_cost_grad (K1+K2) and adam_step (K3), for engines that have only those, and the reference
engine.solve is pinned to bit for bit.  With use_graph either one (and engine.solve_lbfgs) is captured as a HIP
graph by the same class, Graphed.

mppi_solve is the gradient-free solver next to them (MPPI: sample K perturbations of the nominal, cost all of them in
one K1 launch, move the nominal to their softmin-weighted mean): the Python loop over engine.mppi_sample,
engine.rollout_cost and engine.mppi_update that engine.solve_mppi (phnn_solve_mppi) is pinned to bit for bit.
cem_solve is the cross-entropy solver of the same shape (a mean and a standard deviation per problem and element, both
refitted to the lowest-cost samples): the Python loop over engine.cem_sample, engine.rollout_cost and engine.cem_update
that engine.solve_cem (phnn_solve_cem) is pinned to bit for bit.
gn_solve is the curvature-based one: projected Gauss-Newton shooting on the rollout's linearisation with a parallel
backtracking line search, the Python loop over engine.rollout_linearize, engine.gn_direction, engine.gn_candidates,
engine.rollout_cost and engine.gn_select that engine.solve_gn (phnn_solve_gn) is pinned to bit for bit.
"""
import ctypes
import inspect

import numpy as np
import torch


def _need_reference(engine, x_ref):
    if x_ref is not None and not getattr(engine, "supports_reference", False):
        raise NotImplementedError(f"{type(engine).__name__} has no reference tracking (x_ref): RolloutEngine has")


def _need_terminal(engine, terminal):
    if terminal is not None and not hasattr(engine, "terminal_cost"):
        raise NotImplementedError(f"{type(engine).__name__} has no terminal cost (terminal): RolloutEngine has")


def _terminal_kw(terminal):
    """The `terminal` keyword of an engine call: passed only when there is a terminal weight, so that an engine written
    before the terminal cost existed is called exactly as it always was."""
    return {} if terminal is None else {"terminal": terminal}


def shooting_solve(engine, x0, u_init, cost, integrator, dt, lr, iters, track_best=False, u_min=None, u_max=None,
                   record_costs=True, x_ref=None, ref_offset=0, workspace=None, terminal=None):
    """x0 (B,n), u_init (B,H,m) on engine.device -> dict(u_last, costs[, best_u, best_cost]).

    u_last   : unclamped last iterate (B,H,m)
    costs    : (iters,B) cost of each iterate (measured before its Adam step), if record_costs
    best_u   : clamped best iterate (track_best)
    x_ref    : reference trajectory broadcastable to (B, rows, n), tracked from row ref_offset (int or device int32
               tensor) on (RolloutEngine.rollout_cost); None: the cost's x_target
    workspace: optional dict that keeps the engine's buffers alive across calls
    terminal : a terminal.TerminalCost, or None.  With one an iteration is K1 (engine.rollout_cost with the trajectory),
               engine.terminal_cost (the total cost, and row H of the cotangent), K2 (engine.rollout_vjp with that
               cotangent), K3: the sequence phnn_solve_term enqueues
    """
    _need_reference(engine, x_ref)
    _need_terminal(engine, terminal)
    rkw = {} if x_ref is None else {"x_ref": x_ref, "ref_offset": ref_offset}  # an engine without tracking takes neither
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
    ws = {} if workspace is None else workspace
    tb = None
    for k in range(iters):
        if terminal is None:
            c, g = engine.rollout_cost_grad(x0, u, cost, integrator, dt, workspace=ws, **rkw)
        else:
            c, traj = engine.rollout_cost(x0, u, cost, integrator, dt, want_traj=True, **rkw)
            tb = engine.terminal_cost(traj, cost, terminal, c, traj_bar=tb, want_traj_bar=True, **rkw)
            g = engine.rollout_vjp(x0, u, traj, cost, integrator, dt, traj_bar=tb, **rkw)[0]
        if record_costs:
            costs[k].copy_(c)
        engine.adam_step(u, g, exp_avg, exp_avg_sq, lr, k + 1, cost=c if track_best else None, best_cost=best_cost,
                         best_u=best_u, u_min=u_min, u_max=u_max)
    out = {"u_last": u, "costs": costs}
    if track_best:
        out["best_u"], out["best_cost"] = best_u, best_cost
    return out


def _eager(engine, x0, u_init, cost, integrator, dt, lr, iters, track_best=False, u_min=None, u_max=None, record_costs=True,
           x_ref=None, ref_offset=0, workspace=None, terminal=None):
    """The solve without a captured graph: the library's own loop (phnn_solve: one call enqueues every launch) when the
    engine has one and the Adam-side bounds are the cost's (they are for both controller classes); else the Python loop.
    Same launches, same order: identical results.  x_ref / ref_offset / workspace / terminal: see shooting_solve."""
    _need_reference(engine, x_ref)
    _need_terminal(engine, terminal)
    has_b = u_min is not None and u_max is not None
    same = bool(cost.has_u_bounds) == has_b and (not has_b or (float(cost.u_min) == float(ctypes.c_float(u_min).value)
                                                                and float(cost.u_max) == float(ctypes.c_float(u_max).value)))
    if hasattr(engine, "solve") and same:
        return engine.solve(x0, u_init, cost, integrator, dt, lr=lr, iters=iters, track_best=track_best, record_costs=record_costs,
                            workspace=workspace, x_ref=x_ref, ref_offset=ref_offset, **_terminal_kw(terminal))
    return shooting_solve(engine, x0, u_init, cost, integrator, dt, lr, iters, track_best=track_best, u_min=u_min, u_max=u_max,
                          record_costs=record_costs, x_ref=x_ref, ref_offset=ref_offset, workspace=workspace, terminal=terminal)


def _sampling_solve(engine, x0, u_init, cost, integrator, dt, iters, samples, sample, update, record_costs, workspace, x_ref,
                    ref_offset):
    """The loop under mppi_solve and cem_solve -> dict(u_last, costs, best_u, best_cost).  The mean u starts at
    clamp(u_init) (the cost's bounds); `iters` times: v, x0_rep = sample(u, i, ws) (samples perturbed copies per problem,
    sample 0 u itself), S = engine.rollout_cost of all B * samples rollouts, update(u, v, S, costs_row=, best_cost=,
    best_u=) moves u in place.  sample and update are the method's engine calls with its own arguments bound."""
    _need_reference(engine, x_ref)
    rkw = {}
    B = u_init.shape[0]
    if x_ref is not None:  # one reference per rollout: shared as it is, per-problem expanded once per solve
        rkw = {"x_ref": engine.mppi_reference(x_ref, B, samples), "ref_offset": ref_offset}
    u = u_init.detach().clone().contiguous()
    if cost.has_u_bounds:
        u = torch.clamp(u, float(cost.u_min), float(cost.u_max))
    dev = u.device
    costs = torch.empty(iters, B, dtype=torch.float32, device=dev) if record_costs else None
    best_cost = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
    best_u = torch.zeros_like(u)
    ws = {} if workspace is None else workspace
    for i in range(iters):
        v, x0_rep = sample(u, i, ws)
        s = engine.rollout_cost(x0_rep, v, cost, integrator, dt, **rkw)
        update(u, v, s, costs_row=costs[i] if record_costs else None, best_cost=best_cost, best_u=best_u)
    return {"u_last": u, "costs": costs, "best_u": best_u, "best_cost": best_cost}


def _noise_kw(noise):
    """The `noise` keyword of an engine call: passed only when there is a noise shape, so that an engine written before
    shaped noise existed is called exactly as it always was."""
    return {} if noise is None else {"noise": noise}


def mppi_solve(engine, x0, u_init, cost, integrator, dt, iters, samples, lam, sigma, seed, epoch=0, problem_offset=0,
               record_costs=True, workspace=None, x_ref=None, ref_offset=0, noise=None):
    """Sampling MPC (MPPI) on B independent problems: x0 (B,n), u_init (B,H,m) -> dict(u_last, costs, best_u, best_cost).

    The nominal u starts at clamp(u_init) (the cost's bounds); `iters` times: v = engine.mppi_sample (samples
    perturbed copies per problem, sample 0 the nominal itself), S = engine.rollout_cost of all B * samples rollouts,
    engine.mppi_update moves the nominal to sum_k w_k v_k / sum_k w_k with w_k = exp(-(S_k - min S) / lam).
    u_last   : the last nominal (B,H,m), in bounds
    costs    : (iters,B) cost of the nominal at every iteration (its sample 0), if record_costs
    best_u   : the best sample seen over all iterations (strict '<', lowest sample index on ties), best_cost its cost
    seed, epoch (int or device int32 tensor), problem_offset: the noise counter; problem b draws the noise of global
    problem problem_offset + b whatever batch it is solved in.  x_ref, ref_offset: as in shooting_solve.
    noise: None = white noise; a noise.Noise = time-correlated noise of that shape (engine.mppi_sample(noise=))."""
    return _sampling_solve(
        engine, x0, u_init, cost, integrator, dt, iters, samples,
        lambda u, i, ws: engine.mppi_sample(x0, u, cost, samples, sigma, seed, i, epoch=epoch, problem_offset=problem_offset,
                                            workspace=ws, **_noise_kw(noise)),
        lambda u, v, s, **out: engine.mppi_update(u, v, s, lam, cost, **out), record_costs, workspace, x_ref, ref_offset)


def cem_solve(engine, x0, u_init, cost, integrator, dt, iters, samples, elites, alpha, sigma, sigma_min, seed, epoch=0,
              problem_offset=0, record_costs=True, workspace=None, x_ref=None, ref_offset=0, noise=None):
    """Sampling MPC by the cross-entropy method on B independent problems: x0 (B,n), u_init (B,H,m) ->
    dict(u_last, sigma_last, costs, best_u, best_cost).

    The mean u starts at clamp(u_init) (the cost's bounds), the standard deviation sig at sigma (one value or one per
    control component) in every element; `iters` times: v = engine.cem_sample (samples perturbed copies per problem,
    sample 0 the mean itself), S = engine.rollout_cost of all B * samples rollouts, engine.cem_update refits u and sig
    to the `elites` samples of lowest finite cost with smoothing alpha, sig floored at sigma_min.
    u_last   : the last mean (B,H,m), in bounds;  sigma_last: the last standard deviation (B,H,m)
    costs, best_u, best_cost, seed, epoch, problem_offset, x_ref, ref_offset, noise: as in mppi_solve."""
    _need_reference(engine, x_ref)
    m = u_init.shape[2]
    s0 = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if s0.size not in (1, m):
        raise ValueError(f"sigma: one value or one per control component (m = {m}), got {sigma!r}")
    if not np.all((s0 >= 0) & np.isfinite(s0)):
        raise ValueError("sigma must be >= 0 and finite")
    sig = torch.tensor(np.broadcast_to(s0, (m,)).copy(), dtype=torch.float32, device=u_init.device).expand_as(u_init).contiguous()
    out = _sampling_solve(
        engine, x0, u_init, cost, integrator, dt, iters, samples,
        lambda u, i, ws: engine.cem_sample(x0, u, sig, cost, samples, seed, i, epoch=epoch, problem_offset=problem_offset,
                                           workspace=ws, **_noise_kw(noise)),
        lambda u, v, s, **out: engine.cem_update(u, sig, v, s, elites, alpha, sigma_min, cost, **out), record_costs, workspace,
        x_ref, ref_offset)
    return {"u_last": out.pop("u_last"), "sigma_last": sig, **out}


def _library_or(engine, name, loop):
    """-> the eager solve of a sampling method: the library's own loop (engine.<name>) where the engine has one, else the
    Python loop over its primitives (`loop`, called with the engine first).  Same launches, same order: identical results."""
    return getattr(engine, name) if hasattr(engine, name) else lambda *a, **k: loop(engine, *a, **k)


def _mppi_eager(engine, x0, u_init, cost, integrator, dt, iters, samples, lam, sigma, seed, epoch=0, problem_offset=0,
                record_costs=True, workspace=None, x_ref=None, ref_offset=0, noise=None):
    """The MPPI solve without a captured graph (_library_or); called as mppi_solve is."""
    return _library_or(engine, "solve_mppi", mppi_solve)(
        x0, u_init, cost, integrator, dt, iters=iters, samples=samples, lam=lam, sigma=sigma, seed=seed, epoch=epoch,
        problem_offset=problem_offset, record_costs=record_costs, workspace=workspace, x_ref=x_ref, ref_offset=ref_offset,
        **_noise_kw(noise))


def _cem_eager(engine, x0, u_init, cost, integrator, dt, iters, samples, elites, alpha, sigma, sigma_min, seed, epoch=0,
               problem_offset=0, record_costs=True, workspace=None, x_ref=None, ref_offset=0, noise=None):
    """The CEM solve without a captured graph (_library_or); called as cem_solve is."""
    return _library_or(engine, "solve_cem", cem_solve)(
        x0, u_init, cost, integrator, dt, iters=iters, samples=samples, elites=elites, alpha=alpha, sigma=sigma,
        sigma_min=sigma_min, seed=seed, epoch=epoch, problem_offset=problem_offset, record_costs=record_costs,
        workspace=workspace, x_ref=x_ref, ref_offset=ref_offset, **_noise_kw(noise))


def gn_solve(engine, x0, u_init, cost, integrator, dt, iters, line_steps=8, mu_init=1e-6, mu_min=1e-9, mu_max=1e6, mu_up=10.0,
             mu_down=0.1, record_costs=True, workspace=None, x_ref=None, ref_offset=0, box=False, terminal=None):
    """Projected Gauss-Newton shooting with Levenberg-Marquardt regularisation and a parallel backtracking line search on
    B independent problems: x0 (B,n), u_init (B,H,m) -> dict(u_last, cost, costs, mu, accepts, alpha_hist).

    The iterate u starts at clamp(u_init) (the cost's bounds) with cost and trajectory from engine.rollout_cost and
    mu = mu_init; `iters` times: engine.rollout_linearize at (u, traj), engine.gn_direction (the LQ step du on that
    model with the stage cost's gradients, Quu + mu I), engine.gn_candidates (clamp(u + 2^-j du), j < line_steps),
    engine.rollout_cost of all B * line_steps candidates, engine.gn_select (the best finite candidate replaces the
    iterate iff it is strictly cheaper; mu shrinks after an accepted iteration and grows after a rejected one).
    u_last    : the last iterate (B,H,m), in bounds;  cost: its cost (B) -- never higher than an earlier one
    costs     : (iters,B) cost of the iterate at the START of every iteration, if record_costs
    mu        : (B) float64, accepts: (B) int32 accepted iterations, alpha_hist: (iters,B) accepted step length or 0
    x_ref, ref_offset: as in shooting_solve (one reference per problem; the candidates of a problem share it).
    box       : the direction is the box-constrained LQ step (engine.gn_direction(..., box=True));
                the result gains nclamp_hist (iters,B) int32, the (t, component) pairs each direction held on a bound
    terminal  : a terminal.TerminalCost, or None.  With one engine.terminal_cost follows the set-up K1 and the candidates'
                K1 (group = line_steps rows per problem there) and the direction takes it (engine.gn_direction(...,
                terminal=)): the sequence phnn_solve_gn_term enqueues
    The Python loop that engine.solve_gn (phnn_solve_gn, phnn_solve_gn_ex, phnn_solve_gn_term) is pinned to bit for bit."""
    _need_reference(engine, x_ref)
    _need_terminal(engine, terminal)
    B, L = u_init.shape[0], int(line_steps)
    rkw_b, rkw_r = {}, {}
    if x_ref is not None:
        rkw_b = {"x_ref": x_ref, "ref_offset": ref_offset}
        rkw_r = {"x_ref": engine.mppi_reference(x_ref, B, L), "ref_offset": ref_offset}
    u = u_init.detach().clone().contiguous()
    if cost.has_u_bounds:
        u = torch.clamp(u, float(cost.u_min), float(cost.u_max))
    dev = u.device
    costs = torch.empty(iters, B, dtype=torch.float32, device=dev) if record_costs else None
    alpha = torch.empty(iters, B, dtype=torch.float32, device=dev) if record_costs else None
    mu = torch.full((B,), float(mu_init), dtype=torch.float64, device=dev)
    accepts = torch.zeros(B, dtype=torch.int32, device=dev)
    nclamp = torch.empty(iters, B, dtype=torch.int32, device=dev) if box else None
    bkw = {"box": True} if box else {}  # an engine without the box step is never handed the keyword
    c, traj = engine.rollout_cost(x0, u, cost, integrator, dt, want_traj=True, **rkw_b)
    if terminal is not None:
        engine.terminal_cost(traj, cost, terminal, c, **rkw_b)
    for it in range(iters):
        A, Bm, _ = engine.rollout_linearize(x0, u, cost, integrator, dt, traj=traj)
        d = engine.gn_direction(A, Bm, traj, u, cost, mu, **rkw_b, **bkw, **_terminal_kw(terminal))
        if box:
            nclamp[it].copy_(d["nclamp"])
        cand, x0_rep = engine.gn_candidates(x0, u, d["du"], cost, L)
        s, ctraj = engine.rollout_cost(x0_rep, cand, cost, integrator, dt, want_traj=True, **rkw_r)
        if terminal is not None:
            engine.terminal_cost(ctraj, cost, terminal, s, group=L, **rkw_r)
        engine.gn_select(u, traj, c, mu, accepts, cand, s, ctraj, d["status"], L, mu_min, mu_max, mu_up, mu_down,
                         costs_row=costs[it] if record_costs else None, alpha_row=alpha[it] if record_costs else None)
    out = {"u_last": u, "cost": c, "costs": costs, "mu": mu, "accepts": accepts, "alpha_hist": alpha}
    if box:
        out["nclamp_hist"] = nclamp
    return out


def _gn_eager(engine, x0, u_init, cost, integrator, dt, iters, line_steps=8, mu_init=1e-6, mu_min=1e-9, mu_max=1e6, mu_up=10.0,
              mu_down=0.1, record_costs=True, workspace=None, x_ref=None, ref_offset=0, box=False, terminal=None):
    """The Gauss-Newton solve without a captured graph (_library_or); called as gn_solve is."""
    _need_terminal(engine, terminal)
    bkw = {"box": True} if box else {}
    bkw.update(_terminal_kw(terminal))
    return _library_or(engine, "solve_gn", gn_solve)(
        x0, u_init, cost, integrator, dt, iters=iters, line_steps=line_steps, mu_init=mu_init, mu_min=mu_min, mu_max=mu_max,
        mu_up=mu_up, mu_down=mu_down, record_costs=record_costs, workspace=workspace, x_ref=x_ref, ref_offset=ref_offset, **bkw)


def capture(device, fn):
    """Runs fn() once on a side stream (whatever it allocates for later calls, it allocates outside the capture), then
    captures a second fn() as a HIP graph.  -> (graph, what the captured fn() returned).  Recording executes nothing:
    fn has run exactly once when this returns."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


class Graphed:
    """An eager solve callable `fn` (_eager, engine.solve_lbfgs) captured once as a HIP graph -- every launch of the
    solve and the library's state reset (memsets) -- and replayed per call: one graph launch per MPC solve instead of
    3 x iters kernel launches.  Worth it where the solve is launch-bound -- the reference's own use, one plant (or a
    few) per call in a closed loop.  Called exactly as fn is.

    The graph is tied to the shapes of x0 and u_init, the cost struct and every other argument of fn (integrator, dt,
    lr, iteration counts, flags); a call with another signature re-captures.  x0 and u_init are copied into the graph's
    static buffers, results are returned as fresh tensors.  The graph holds the very launches of fn in fn's order:
    results are bit-identical to fn's.

    Reference tracking (x_ref, ref_offset): the graph reads the reference through the pointer it was captured with.
    That pointer is a static buffer of the graph, (1 | B, rows, n) as reference_view leaves it before broadcasting,
    and every call copies the caller's x_ref (and ref_offset, int or device int32 tensor) into it: a reference of
    another shape re-captures, one updated in place is seen by the next call.  The static buffer stays alive as long
    as this object holds the graph.

    Terminal cost (terminal): a terminal.TerminalCost keys the graph by identity and its device tensor is what the graph
    reads: keep the object, another one re-captures.
    """

    def __init__(self, engine, fn):
        self.engine, self.fn = engine, fn
        self.params = inspect.signature(fn)
        self.key = None
        self.graph = None

    def _compact_reference(self, x_ref, B):
        """x_ref -> the (1 | B, rows, 1 | n) tensor reference_view broadcasts from (what the static buffer holds)."""
        from .engine import reference_view
        t, bs, ts, rows = reference_view(x_ref, B, self.engine.n, self.engine.device)
        t = t[:1] if bs == 0 else t
        t = t[:, :1] if ts == 0 else t
        return t

    def __call__(self, *args, **kwargs):
        a = self.params.bind(*args, **kwargs)
        a.apply_defaults()
        a = dict(a.arguments)  # what is left in it below are fn's options: part of the signature, passed on as given
        assert a.get("engine", self.engine) is self.engine
        x0, u_init, cost = a.pop("x0"), a.pop("u_init"), a.pop("cost")
        x_ref, ref_offset = a.pop("x_ref"), a.pop("ref_offset")
        del a["workspace"]  # the graph keeps its own
        if a.get("terminal") is not None:
            from .terminal import TerminalCost
            if not isinstance(a["terminal"], TerminalCost):  # an array neither hashes nor gives the graph a pointer that stays
                raise TypeError("a captured solve takes terminal= as a terminal.TerminalCost (it keys the graph by identity and "
                                f"holds the device tensor the graph reads), not a {type(a['terminal']).__name__}: wrap the "
                                "matrix once, TerminalCost(W), and keep the object")
        _need_reference(self.engine, x_ref)
        ref = None if x_ref is None else self._compact_reference(x_ref, x0.shape[0])
        key = (tuple(x0.shape), tuple(u_init.shape), bytes(ctypes.string_at(ctypes.addressof(cost), ctypes.sizeof(cost))),
               tuple(sorted(a.items())), None if ref is None else tuple(ref.shape))
        if key != self.key:
            self.key = None
            dev = self.engine.device
            self.x0 = x0.detach().clone().contiguous()
            self.u_init = u_init.detach().clone().contiguous()
            self.x_ref = None if ref is None else ref.clone()
            self.ref_offset = torch.zeros(1, dtype=torch.int32, device=dev) if ref is not None else 0
            ws = {}
            self.graph, self.out = capture(dev, lambda: self.fn(x0=self.x0, u_init=self.u_init, cost=cost, workspace=ws,
                                                                 x_ref=self.x_ref, ref_offset=self.ref_offset, **a))
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


class GraphedSolve(Graphed):
    """The Adam solve (_eager: engine.solve where the engine has it) as a graph; called as shooting_solve is."""

    def __init__(self, engine):
        super().__init__(engine, _eager)


class GraphedLBFGS(Graphed):
    """engine.solve_lbfgs as a graph: the state reset plus every outer_steps x max_iter x (K1, K2, k_lbfgs) launch."""

    def __init__(self, engine):
        super().__init__(engine, engine.solve_lbfgs)


class GraphedMPPI(Graphed):
    """The MPPI solve (_mppi_eager) as a graph: the clamp and resets plus every iters x (k_sample, K1, k_mppi_update)
    launch.  `epoch` is part of the graph's signature: an int re-captures when it changes, a device int32 tensor is read
    through its pointer at every replay (fill it in place between calls to draw fresh noise).  sigma must be hashable (a
    float or a tuple).  A per-problem x_ref lives in the graph's static buffer as given and its expansion to one row set
    per rollout is part of the replayed graph.  noise: None or a noise.Noise -- it keys the graph by identity and its
    device tensor is the graph's static buffer: keep the object, another one re-captures."""

    def __init__(self, engine):
        super().__init__(engine, _mppi_eager)


class GraphedCEM(Graphed):
    """The CEM solve (_cem_eager) as a graph: the clamp and resets plus every iters x (k_sample, K1, k_cem_update)
    launch.  `epoch`, sigma and x_ref behave as in GraphedMPPI."""

    def __init__(self, engine):
        super().__init__(engine, _cem_eager)


class GraphedGN(Graphed):
    """The Gauss-Newton solve (_gn_eager) as a graph: the clamp, the state reset and the set-up K1 plus every iters x
    (k_rollout_linearize, k_gn_direction, k_gn_candidates, K1, k_gn_select) launch.  x_ref behaves as in GraphedMPPI."""

    def __init__(self, engine):
        super().__init__(engine, _gn_eager)


def _graphed_or(eager, cls, engine, use_graph, previous):
    if not use_graph or engine.device.type != "cuda":
        return eager
    if type(previous) is cls and previous.engine is engine:
        return previous
    return cls(engine)


def solver_for(engine, use_graph, previous=None):
    """-> callable(engine, x0, u_init, cost, ...) as shooting_solve: _eager, or a GraphedSolve bound to `engine`
    (reused from `previous` when it already is one for this engine)."""
    return _graphed_or(_eager, GraphedSolve, engine, use_graph, previous)


def lbfgs_solver_for(engine, use_graph, previous=None):
    """-> callable(**solve_lbfgs arguments) -> dict(u_last, costs, n_iter, func_evals): engine.solve_lbfgs, or a
    GraphedLBFGS bound to `engine` (reused from `previous` when it already is one for this engine)."""
    if not hasattr(engine, "solve_lbfgs"):
        raise NotImplementedError(f"{type(engine).__name__} has no batched L-BFGS solve (RolloutEngine has): use "
                                  "compute_control (one plant at a time)")
    return _graphed_or(engine.solve_lbfgs, GraphedLBFGS, engine, use_graph, previous)


def mppi_solver_for(engine, use_graph, previous=None):
    """-> callable(engine, x0, u_init, cost, ...) as _mppi_eager: itself, or a GraphedMPPI bound to `engine` (reused from
    `previous` when it already is one for this engine)."""
    if not hasattr(engine, "mppi_sample"):
        raise NotImplementedError(f"{type(engine).__name__} has no MPPI kernels (RolloutEngine has)")
    return _graphed_or(_mppi_eager, GraphedMPPI, engine, use_graph, previous)


def cem_solver_for(engine, use_graph, previous=None):
    """-> callable(engine, x0, u_init, cost, ...) as _cem_eager: itself, or a GraphedCEM bound to `engine` (reused from
    `previous` when it already is one for this engine)."""
    if not hasattr(engine, "cem_sample"):
        raise NotImplementedError(f"{type(engine).__name__} has no CEM kernels (RolloutEngine has)")
    return _graphed_or(_cem_eager, GraphedCEM, engine, use_graph, previous)


def gn_solver_for(engine, use_graph, previous=None):
    """-> callable(engine, x0, u_init, cost, ...) as _gn_eager: itself, or a GraphedGN bound to `engine` (reused from
    `previous` when it already is one for this engine)."""
    if not hasattr(engine, "gn_direction"):
        raise NotImplementedError(f"{type(engine).__name__} has no Gauss-Newton kernels (RolloutEngine has)")
    return _graphed_or(_gn_eager, GraphedGN, engine, use_graph, previous)


# optimizer name of a sampling solve -> (its short name: engine.solve_<name>, controller.<name>_options(), solver_for)
SAMPLING = {"MPPI": ("mppi", mppi_solver_for), "CrossEntropy": ("cem", cem_solver_for)}
