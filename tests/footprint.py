"""Write-footprint harness: one arena, guarded regions, and the library's entry points called on pointers into it.

Every other test hands the library buffers torch allocated at exactly the needed size and looks only at the bytes it
expects to have been written; torch rounds every allocation up and places neighbours behind it, so a store a few floats
past an output, an under-reported workspace size, a read of workspace bytes the call did not write or a read one row
past an input passes all of them.  Here every input, output and workspace of a call is a *region* of ONE uint8 tensor
(the Arena) with a guard in front of it and behind it; the call gets pointers into the arena (the engine's own methods
allocate their outputs, so the C-ABI is called through eng.lib directly), and afterwards the guards are compared with
what was written into them.

Guard width: 64 KiB on each side of every region.  This is a condition, not a measurement: it is larger than any
single vector access (16 B), any tile the kernels store at once (16 rollouts x the widest row: 1 KiB per activation
vector, 17.5 KiB for the whole tape of one dynamics evaluation of a 128-wide model, which is one Euler stash step or one
RK4 stage slot), and any rounding of a workspace sub-region (256 B, 64 floats).  A defect of the kind looked for -- an
off-by-one bound, a tile too many, a region too few -- therefore lands in memory the test owns and cannot reach another
allocation.  If a kernel ever gets a larger stride, GUARD grows with it.  (One whole RK4 stash STEP of a 128-wide
model, four stage slots, is 70 KiB: a step too many would first cross 64 KiB of guard, where check() sees it.  The arena
therefore also keeps one further guard width of slack in front of its first and behind its last region.)

Placement: a region starts on a 256-byte boundary (what torch gives, and what the header promises for the workspace
sub-regions) plus its `skew`.  The skew of a tensor argument is 0 or what a row slice t[1:] of it gives -- the bytes of
one row, 8 or 12 for (B, n) states with n = 2, 3, 4 * H * m for controls (52 for H * m = 13).  A row slice keeps every
alignment the kernels rely on (rows of n = 4 states stay 16-byte aligned; the 16-byte row paths of MPPI / CEM are chosen
by the host from the pointers it is given), so nothing is misaligned that a kernel accesses with a 16-byte vector.
Workspaces are never skewed.

The second half of the module describes each entry point as an Op: its buffers (name, dtype, shape, role, initial
contents), the C calls on arena pointers, and the same operation through the RolloutEngine method on fresh tensors.
tests/test_gpu_footprint.py runs the properties F1 .. F6 over them; tests/test_footprint_model.py checks the arena
itself on CPU tensors.
"""
import ctypes as C

import numpy as np

GUARD = 64 * 1024
ALIGN = 256

IN, OUT, INOUT, WS = "in", "out", "inout", "ws"


def _up(x, a=ALIGN):
    return (x + a - 1) // a * a


class Region:
    """One buffer of a call.  role: IN (read only), OUT (written, contents on entry ignored), INOUT (documented
    in-place state: loaded like an input, compared like an output), WS (workspace)."""

    def __init__(self, name, nbytes, role, skew=0):
        assert role in (IN, OUT, INOUT, WS) and nbytes >= 0 and 0 <= skew < ALIGN
        assert not (role == WS and skew), "workspaces are never skewed"
        self.name, self.nbytes, self.role, self.skew = name, int(nbytes), role, int(skew)


def layout(regions, guard=GUARD):
    """-> ({name: (start, nbytes)}, total bytes): region i starts at a 256-byte boundary + skew, with at least `guard`
    bytes that belong to no region in front of it and behind it (the guards of two neighbours do not overlap), and one
    more guard width of slack at either end of the arena."""
    at, cur = {}, guard  # leading slack
    for r in regions:
        assert r.name not in at, r.name
        start = _up(cur + guard) + r.skew
        at[r.name] = (start, r.nbytes)
        cur = start + r.nbytes + guard
    return at, _up(cur + guard)  # trailing slack


class Arena:
    def __init__(self, torch, device, regions, guard=GUARD):
        self.torch, self.regions, self.guard = torch, list(regions), guard
        self.at, self.total = layout(self.regions, guard)
        # the arena's own base is put on a 256-byte boundary whatever the allocator gives (the CPU allocator gives 64)
        self._raw = torch.zeros(self.total + ALIGN, dtype=torch.uint8, device=device)
        lead = -self._raw.data_ptr() % ALIGN
        self.buf = self._raw[lead: lead + self.total]
        assert self.buf.data_ptr() % ALIGN == 0
        self._gbyte = {}  # (name, side) -> byte the guard was filled with

    # -------------------------------------------------------------- geometry
    def guards(self, name):
        """-> ((front start, front end), (back start, back end)) of region `name`: exactly `guard` bytes each."""
        s, n = self.at[name]
        return (s - self.guard, s), (s + n, s + n + self.guard)

    def interior(self, name):
        s, n = self.at[name]
        return self.buf[s: s + n]

    def view(self, name, dtype, shape):
        return self.interior(name).view(dtype).view(*shape)

    def ptr(self, name):
        return C.c_void_p(self.buf.data_ptr() + self.at[name][0])

    # -------------------------------------------------------------- contents
    def fill(self, byte, input_guard_byte=None):
        """Writes `byte` to every byte of the arena that is not the interior of an IN / INOUT region: all guards, the
        gaps between them, and the interiors of outputs and workspaces.  input_guard_byte: another byte for the guards
        around the IN regions (the read fence)."""
        cur = 0
        for r in self.regions:
            s, n = self.at[r.name]
            keep = r.role in (IN, INOUT)
            self.buf[cur: s if keep else s + n].fill_(byte)
            cur = s + n
        self.buf[cur:].fill_(byte)
        for r in self.regions:
            gb = input_guard_byte if (r.role == IN and input_guard_byte is not None) else byte
            for side, (a, b) in zip(("front", "back"), self.guards(r.name)):
                self._gbyte[(r.name, side)] = gb
                if gb != byte:
                    self.buf[a:b].fill_(gb)

    def load(self, name, tensor):
        """Copies a tensor's bytes into the interior of region `name`."""
        t = self.torch.as_tensor(tensor).contiguous()
        src = t.reshape(-1).view(self.torch.uint8)
        dst = self.interior(name)
        assert src.numel() == dst.numel(), (name, src.numel(), dst.numel())
        dst.copy_(src)

    def check(self):
        """-> [(region, 'front' | 'back', offset of the first changed byte within that guard)], empty when every guard
        still holds what fill() wrote.  The comparison runs on the arena's device; only the verdict is copied."""
        torch = self.torch
        keys, flags = [], []
        for r in self.regions:
            for side, (a, b) in zip(("front", "back"), self.guards(r.name)):
                keys.append((r.name, side, a, b))
                flags.append((self.buf[a:b] != self._gbyte[(r.name, side)]).any())
        if not keys:
            return []
        verdict = torch.stack(flags).cpu().tolist()
        hits = []
        for (name, side, a, b), bad in zip(keys, verdict):
            if bad:
                ne = (self.buf[a:b] != self._gbyte[(name, side)]).to(torch.uint8)
                hits.append((name, side, int(ne.argmax())))
        return hits

    def written(self, name, byte):
        """-> (first, last + 1) byte offsets within region `name` that differ from `byte`, or None when none does."""
        ne = (self.interior(name) != byte).nonzero()
        if ne.numel() == 0:
            return None
        return int(ne[0]), int(ne[-1]) + 1


# ===================================================================================================== operations
class Buf:
    """A buffer of an operation.  init: numpy array loaded before the call (IN, INOUT, and the accumulating outputs the
    test initialises itself); skew: may be placed at the row-slice offset (tensor arguments; never workspaces)."""

    def __init__(self, name, dtype, shape, role, init=None, skew=True):
        self.name, self.dtype, self.shape, self.role, self.init = name, np.dtype(dtype), tuple(int(d) for d in shape), role, init
        self.can_skew = skew and role != WS
        if init is not None:
            assert init.dtype == self.dtype and init.shape == self.shape, (name, init.dtype, init.shape, self.shape)

    @property
    def nbytes(self):
        return int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize

    @property
    def row_skew(self):
        """Byte offset of t[1:] against t, modulo the region alignment: what a row slice through the engine produces."""
        row = int(np.prod(self.shape[1:], dtype=np.int64)) * self.dtype.itemsize
        return row % ALIGN if self.can_skew else 0


def _torch_dtype(torch, dt):
    return {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8}[np.dtype(dt).name]


class Op:
    """One entry point (or a chain of them sharing buffers) as a footprint case.  Subclasses fill self.bufs, and give
    call(eng, p) -- the C calls, p[name] a c_void_p into the arena or None for a buffer the case leaves out -- and
    engine(eng) -> {buffer name: tensor} of the same operation through the RolloutEngine on fresh tensors (only the
    buffers that path produces)."""

    name = "op"

    def __init__(self):
        self.bufs = []

    def add(self, *a, **k):
        self.bufs.append(Buf(*a, **k))

    def regions(self, skew):
        return [Region(b.name, b.nbytes, b.role, b.row_skew if skew else 0) for b in self.bufs]

    def outputs(self):
        return [b for b in self.bufs if b.role in (OUT, INOUT)]

    def input(self, name):
        return next(b.init for b in self.bufs if b.name == name)

    def call(self, eng, p):
        raise NotImplementedError

    def engine(self, eng):
        return {}


def check_rc(eng, rc):
    from phnn_mpc_amd.engine import _check
    _check(eng.lib, eng.h, rc)


def run(torch, eng, op, fill, input_guard_byte=None, skew=False):
    """One execution of `op` in a fresh arena filled with `fill`.  -> (guard hits, {output name: uint8 copy of its
    bytes}, arena)."""
    arena = Arena(torch, eng.device, op.regions(skew))
    arena.fill(fill, input_guard_byte)
    for b in op.bufs:
        if b.init is not None:
            arena.load(b.name, torch.from_numpy(np.ascontiguousarray(b.init)))
    before = {b.name: arena.interior(b.name).clone() for b in op.bufs if b.role == IN}
    p = {b.name: arena.ptr(b.name) for b in op.bufs}
    op.call(eng, p)
    torch.cuda.synchronize(eng.device)
    hits = arena.check()
    for name, was in before.items():  # a kernel must not write its inputs
        ne = (arena.interior(name) != was)
        if bool(ne.any()):
            hits.append((name, "interior", int(ne.to(torch.uint8).argmax())))
    outs = {b.name: arena.interior(b.name).clone() for b in op.outputs()}
    return hits, outs, arena


def as_bytes(torch, t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same_bytes(torch, a, b):
    return a.numel() == b.numel() and bool(torch.equal(a, b))


# ----------------------------------------------------------------------------------------------------- rollouts
class RollOp(Op):
    """K1 then K2 on shared buffers: phnn_rollout_fwd -> phnn_rollout_grad (kind 'grad'), their _ref twins ('ref'), or
    phnn_rollout_fwd -> phnn_rollout_vjp with trajectory and cost cotangents ('vjp').  stash: the K1 -> K2 workspace is
    given (exactly phnn_workspace_bytes) or NULL.  optional: grad_x0 is given, else NULL -- and then a second K1 runs with
    traj = NULL into cost_nt."""

    def __init__(self, eng, cost, x0, U, integ, dt, kind="grad", stash=True, optional=True, rng=None):
        super().__init__()
        B, H, m = U.shape
        n = x0.shape[1]
        self.name = f"roll_{kind} B{B} H{H} integ{integ} stash={int(stash)} opt={int(optional)}"
        self.cost, self.integ, self.dt, self.kind, self.B, self.H, self.stash, self.optional = cost, integ, dt, kind, B, H, stash, optional
        f = np.float32
        self.add("x0", f, (B, n), IN, x0)
        self.add("u", f, (B, H, m), IN, U)
        self.rows = 0
        if kind == "ref":
            self.rows = H + 3  # per-problem reference, longer than the horizon: offset 2 leaves the last row clamped
            self.add("x_ref", f, (B, self.rows, n), IN, (0.1 * rng.normal(size=(B, self.rows, n))).astype(f))
        if kind == "vjp":
            self.add("traj_bar", f, (B, H + 1, n), IN, rng.normal(size=(B, H + 1, n)).astype(f))
            self.add("cost_bar", f, (B,), IN, rng.normal(size=B).astype(f))
        self.add("cost", f, (B,), OUT)
        self.add("traj", f, (B, H + 1, n), OUT)
        self.add("grad_u", f, (B, H, m), OUT)
        if optional:
            self.add("grad_x0", f, (B, n), OUT)
        else:
            self.add("cost_nt", f, (B,), OUT)
        if stash:
            nb = eng.workspace_bytes(B, H, integ)
            assert nb > 0
            self.add("stash", np.uint8, (nb,), WS)

    def _ref(self, p):
        from phnn_mpc_amd import _capi
        r = _capi.Reference()
        n = self.bufs[0].shape[1]
        r.x_ref, r.batch_stride, r.time_stride, r.rows, r.offset_host = p["x_ref"].value, self.rows * n, n, self.rows, 2
        return r

    def call(self, eng, p):
        lib, h, st = eng.lib, eng.h, eng._stream()
        B, H, c, integ, dt = self.B, self.H, C.byref(self.cost), self.integ, float(self.dt)
        ws = p.get("stash")
        if self.kind == "ref":
            r = self._ref(p)
            check_rc(eng, lib.phnn_rollout_fwd_ref(h, p["x0"], p["u"], B, H, c, C.byref(r), integ, dt, p["cost"], p["traj"], ws, st))
            check_rc(eng, lib.phnn_rollout_grad_ref(h, p["x0"], p["u"], B, H, c, C.byref(r), integ, dt, p["traj"], ws,
                                                    p["grad_u"], p.get("grad_x0"), st))
            if not self.optional:
                check_rc(eng, lib.phnn_rollout_fwd_ref(h, p["x0"], p["u"], B, H, c, C.byref(r), integ, dt, p["cost_nt"], None, None, st))
            return
        check_rc(eng, lib.phnn_rollout_fwd(h, p["x0"], p["u"], B, H, c, integ, dt, p["cost"], p["traj"], ws, st))
        if self.kind == "vjp":
            check_rc(eng, lib.phnn_rollout_vjp(h, p["x0"], p["u"], B, H, c, integ, dt, p["traj"], ws, p["traj_bar"], p["cost_bar"],
                                               p["grad_u"], p.get("grad_x0"), st))
        else:
            check_rc(eng, lib.phnn_rollout_grad(h, p["x0"], p["u"], B, H, c, integ, dt, p["traj"], ws, p["grad_u"], p.get("grad_x0"), st))
        if not self.optional:
            check_rc(eng, lib.phnn_rollout_fwd(h, p["x0"], p["u"], B, H, c, integ, dt, p["cost_nt"], None, None, st))

    def engine(self, eng):
        x0, U = self.input("x0"), self.input("u")
        kw = dict(x_ref=self.input("x_ref"), ref_offset=2) if self.kind == "ref" else {}
        name = {0: "euler", 1: "rk4"}[self.integ]
        c, traj = eng.rollout_cost(x0, U, self.cost, name, self.dt, want_traj=True, **kw)
        out = {"cost": c, "traj": traj}
        if not self.optional:
            out["cost_nt"] = eng.rollout_cost(x0, U, self.cost, name, self.dt, **kw)
        if self.kind == "vjp":
            if not self.stash:  # the engine's rollout_vjp passes no stash
                gu, gx = eng.rollout_vjp(x0, U, traj, self.cost, name, self.dt, traj_bar=self.input("traj_bar"),
                                         cost_bar=self.input("cost_bar"))
                out["grad_u"], out["grad_x0"] = gu, gx
        else:
            keep = eng.use_stash
            eng.use_stash = self.stash
            try:
                _, gu, gx = eng.rollout_cost_grad(x0, U, self.cost, name, self.dt, want_grad_x0=True, **kw)
            finally:
                eng.use_stash = keep
            out["grad_u"], out["grad_x0"] = gu, gx
        if not self.optional:
            out.pop("grad_x0", None)
        return out


class PointOp(Op):
    """phnn_model_forward (H given or NULL) and phnn_model_vjp on the same points."""

    def __init__(self, x, u, lam, with_H=True):
        super().__init__()
        B, n = x.shape
        m = u.shape[1]
        self.name, self.B, self.with_H = f"point B{B} H={int(with_H)}", B, with_H
        f = np.float32
        self.add("x", f, (B, n), IN, x)
        self.add("u", f, (B, m), IN, u)
        self.add("lam", f, (B, n), IN, lam)
        self.add("dx", f, (B, n), OUT)
        if with_H:
            self.add("H", f, (B,), OUT)
        self.add("xbar", f, (B, n), OUT)
        self.add("ubar", f, (B, m), OUT)

    def call(self, eng, p):
        st = eng._stream()
        check_rc(eng, eng.lib.phnn_model_forward(eng.h, p["x"], p["u"], self.B, p["dx"], p.get("H"), st))
        check_rc(eng, eng.lib.phnn_model_vjp(eng.h, p["x"], p["u"], p["lam"], self.B, p["xbar"], p["ubar"], st))

    def engine(self, eng):
        dx, H = eng.forward(self.input("x"), self.input("u"))
        xb, ub = eng.vjp(self.input("x"), self.input("u"), self.input("lam"))
        out = {"dx": dx, "xbar": xb, "ubar": ub}
        if self.with_H:
            out["H"] = H
        return out


class TrainOp(Op):
    """The training side.  mode 'plain': phnn_rollout_trajectory (dx given or NULL) alone.  'records': that, then
    phnn_rollout_wgrad recomputing the forward pass.  'tapes': phnn_rollout_trajectory_ws into the weight-gradient
    workspace, then phnn_rollout_wgrad with PHNN_WGRAD_TAPES.  accumulate: grad_theta is added to -- an accumulating
    entry, so the test initialises it itself (its contents on entry are data, not scratch)."""

    def __init__(self, eng, x0, U, integ, dt, rng, mode="records", optional=True, accumulate=False):
        super().__init__()
        B, H, m = U.shape
        n = x0.shape[1]
        self.name = f"train_{mode} B{B} H{H} integ{integ} opt={int(optional)} acc={int(accumulate)}"
        self.B, self.H, self.integ, self.dt, self.mode, self.optional, self.accumulate = B, H, integ, dt, mode, optional, accumulate
        f = np.float32
        self.add("x0", f, (B, n), IN, x0)
        self.add("u", f, (B, H, m), IN, U)
        self.add("traj", f, (B, H + 1, n), OUT)
        if optional:
            self.add("dX", f, (B, H, n), OUT)
        if mode != "plain":
            self.add("traj_bar", f, (B, H + 1, n), IN, rng.normal(size=(B, H + 1, n)).astype(f))
            self.add("dx_bar", f, (B, H, n), IN, rng.normal(size=(B, H, n)).astype(f))
            P = eng.blob.size
            self.add("grad_theta", f, (P,), INOUT if accumulate else OUT, rng.normal(size=P).astype(f) if accumulate else None)
            if optional:
                self.add("grad_u", f, (B, H, m), OUT)
                self.add("grad_x0", f, (B, n), OUT)
            nb = int(eng.lib.phnn_wgrad_workspace_bytes(eng.h, B, H, integ))
            assert nb > 0
            self.add("wws", np.uint8, (nb,), WS)

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        lib, h, st = eng.lib, eng.h, eng._stream()
        B, H, integ, dt = self.B, self.H, self.integ, float(self.dt)
        if self.mode == "tapes":
            check_rc(eng, lib.phnn_rollout_trajectory_ws(h, p["x0"], p["u"], B, H, integ, dt, p["traj"], p.get("dX"), p["wws"], st))
        else:
            check_rc(eng, lib.phnn_rollout_trajectory(h, p["x0"], p["u"], B, H, integ, dt, p["traj"], p.get("dX"), st))
        if self.mode == "plain":
            return
        flags = (_capi.WGRAD_ACCUMULATE if self.accumulate else 0) | (_capi.WGRAD_TAPES if self.mode == "tapes" else 0)
        check_rc(eng, lib.phnn_rollout_wgrad(h, p["x0"], p["u"], B, H, integ, dt, p["traj"], p["traj_bar"], p["dx_bar"], p["wws"],
                                             p["grad_theta"], flags, p.get("grad_u"), p.get("grad_x0"), st))

    def engine(self, eng):
        import torch
        x0, U = self.input("x0"), self.input("u")
        name = {0: "euler", 1: "rk4"}[self.integ]
        traj, dX = eng.rollout_trajectory(x0, U, name, self.dt, want_dx=True, tapes=self.mode == "tapes")
        out = {"traj": traj}
        if self.optional:
            out["dX"] = dX
        if self.mode != "plain":
            gt = torch.tensor(self.input("grad_theta"), device=eng.device) if self.accumulate else None
            g, gu, gx = eng.rollout_wgrad(x0, U, traj, name, self.dt, traj_bar=self.input("traj_bar"), dx_bar=self.input("dx_bar"),
                                          grad_theta=gt, accumulate=self.accumulate,
                                          tape_token=eng.tape_token if self.mode == "tapes" else None)
            out["grad_theta"] = g
            if self.optional:
                out["grad_u"], out["grad_x0"] = gu, gx
        return out


class PointWgradOp(Op):
    """phnn_model_wgrad (Hbar given or NULL; accumulate: grad_theta initialised by the test, see TrainOp)."""

    def __init__(self, eng, x, u, lam, Hbar, rng, accumulate=False):
        super().__init__()
        N, n = x.shape
        m = u.shape[1]
        self.name, self.N, self.accumulate = f"point_wgrad N{N} Hbar={int(Hbar is not None)} acc={int(accumulate)}", N, accumulate
        f = np.float32
        self.add("x", f, (N, n), IN, x)
        self.add("u", f, (N, m), IN, u)
        self.add("lam", f, (N, n), IN, lam)
        if Hbar is not None:
            self.add("Hbar", f, (N,), IN, Hbar)
        P = eng.blob.size
        self.add("grad_theta", f, (P,), INOUT if accumulate else OUT, rng.normal(size=P).astype(f) if accumulate else None)
        self.add("xbar", f, (N, n), OUT)
        self.add("ubar", f, (N, m), OUT)
        nb = int(eng.lib.phnn_wgrad_workspace_bytes(eng.h, N, 0, 0))
        assert nb > 0
        self.add("wws", np.uint8, (nb,), WS)

    def call(self, eng, p):
        check_rc(eng, eng.lib.phnn_model_wgrad(eng.h, p["x"], p["u"], p["lam"], p.get("Hbar"), self.N, p["wws"], p["grad_theta"],
                                               int(self.accumulate), p["xbar"], p["ubar"], eng._stream()))

    def engine(self, eng):
        import torch
        names = [b.name for b in self.bufs]
        gt = torch.tensor(self.input("grad_theta"), device=eng.device) if self.accumulate else None
        g, xb, ub = eng.model_wgrad(self.input("x"), self.input("u"), self.input("lam"),
                                    self.input("Hbar") if "Hbar" in names else None, grad_theta=gt, accumulate=self.accumulate)
        return {"grad_theta": g, "xbar": xb, "ubar": ub}


# ----------------------------------------------------------------------------------------------------- solves
class AdamOp(Op):
    """phnn_adam_step with best-iterate tracking.  best_cost and best_u accumulate (strict '<' against the value on
    entry), so the test initialises them: half the problems improve, half do not."""

    def __init__(self, B, H, m, rng, u_min, u_max):
        super().__init__()
        f = np.float32
        self.name, self.B, self.per, self.u_min, self.u_max = f"adam B{B} H{H} m{m}", B, H * m, u_min, u_max
        sh = (B, H, m)
        self.add("u", f, sh, INOUT, rng.uniform(-3, 3, size=sh).astype(f))
        self.add("grad", f, sh, IN, rng.normal(size=sh).astype(f))
        self.add("m", f, sh, INOUT, (0.1 * rng.normal(size=sh)).astype(f))
        self.add("v", f, sh, INOUT, (0.1 * rng.uniform(size=sh)).astype(f))
        cost = rng.uniform(1, 2, size=B).astype(f)
        self.add("cost", f, (B,), IN, cost)
        self.add("best_cost", f, (B,), INOUT, np.where(np.arange(B) % 2 == 0, cost + 1, cost - 1).astype(f))
        self.add("best_u", f, sh, INOUT, rng.normal(size=sh).astype(f))

    def call(self, eng, p):
        check_rc(eng, eng.lib.phnn_adam_step(eng.h, p["u"], p["grad"], p["m"], p["v"], self.B * self.per, 0.015, 0.9, 0.999, 1e-8, 3,
                                             p["cost"], p["best_cost"], p["best_u"], self.per, self.u_min, self.u_max, 1,
                                             eng._stream()))

    def engine(self, eng):
        import torch
        t = {k: torch.tensor(self.input(k), device=eng.device) for k in ("u", "grad", "m", "v", "cost", "best_cost", "best_u")}
        eng.adam_step(t["u"], t["grad"], t["m"], t["v"], 0.015, 3, cost=t["cost"], best_cost=t["best_cost"], best_u=t["best_u"],
                      u_min=self.u_min, u_max=self.u_max)
        return {k: t[k] for k in ("u", "m", "v", "best_cost", "best_u")}


class SolveOp(Op):
    """phnn_solve (Adam, track_best on), 2 iterations."""
    ITERS = 2

    def __init__(self, eng, cost, x0, U, integ, dt, stash=True):
        super().__init__()
        B, H, m = U.shape
        n = x0.shape[1]
        self.name = f"solve B{B} H{H} m{m} integ{integ} stash={int(stash)}"
        self.cost, self.integ, self.dt, self.B, self.H, self.stash = cost, integ, dt, B, H, stash
        f = np.float32
        self.add("x0", f, (B, n), IN, x0)
        self.add("u", f, (B, H, m), INOUT, U)
        for k in ("m", "v", "grad"):
            self.add(k, f, (B, H, m), OUT)
        self.add("cost", f, (B,), OUT)
        self.add("traj", f, (B, H + 1, n), OUT)
        self.add("costs", f, (self.ITERS, B), OUT)
        self.add("best_cost", f, (B,), OUT)
        self.add("best_u", f, (B, H, m), OUT)
        if stash:
            self.add("stash", np.uint8, (eng.workspace_bytes(B, H, integ),), WS)

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        opt = _capi.SolveOptions(self.ITERS, 0.015, 0.9, 0.999, 1e-8, 1)
        check_rc(eng, eng.lib.phnn_solve(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), self.integ, float(self.dt),
                                         C.byref(opt), p["m"], p["v"], p["grad"], p["cost"], p["traj"], p.get("stash"), p["costs"],
                                         p["best_cost"], p["best_u"], eng._stream()))

    def engine(self, eng):
        keep = eng.use_stash
        eng.use_stash = self.stash
        try:
            ws = {}
            r = eng.solve(self.input("x0"), self.input("u"), self.cost, {0: "euler", 1: "rk4"}[self.integ], self.dt, lr=0.015,
                          iters=self.ITERS, track_best=True, workspace=ws)
        finally:
            eng.use_stash = keep
        return {"u": r["u_last"], "costs": r["costs"], "best_cost": r["best_cost"], "best_u": r["best_u"], "m": ws["m"], "v": ws["v"],
                "grad": ws["grad_u"], "cost": ws["cost"], "traj": ws["traj"]}


class LbfgsOp(Op):
    """phnn_solve_lbfgs, history 3, max_iter 4, one outer step; the optimizer state lives in a workspace of exactly
    phnn_lbfgs_workspace_bytes."""
    HIST, MAX_ITER = 3, 4

    def __init__(self, eng, cost, x0, U, integ, dt):
        super().__init__()
        B, H, m = U.shape
        n = x0.shape[1]
        self.name = f"lbfgs B{B} H{H} m{m} integ{integ}"
        self.cost, self.integ, self.dt, self.B, self.H = cost, integ, dt, B, H
        f = np.float32
        self.add("x0", f, (B, n), IN, x0)
        self.add("u", f, (B, H, m), INOUT, U)
        self.add("grad", f, (B, H, m), OUT)
        self.add("cost", f, (B,), OUT)
        self.add("traj", f, (B, H + 1, n), OUT)
        self.add("costs", f, (1, B), OUT)
        self.add("n_iter", np.int32, (B,), OUT)
        self.add("func_evals", np.int32, (B,), OUT)
        self.add("stash", np.uint8, (eng.workspace_bytes(B, H, integ),), WS)
        self.nws = eng.lbfgs_workspace_bytes(B, H, self.HIST)
        assert self.nws > 0
        self.add("lws", np.uint8, (self.nws,), WS)

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        opt = _capi.LbfgsOptions()
        opt.outer_steps, opt.max_iter, opt.max_eval, opt.history_size = 1, self.MAX_ITER, 0, self.HIST
        opt.lr, opt.tolerance_grad, opt.tolerance_change = 1.0, 1e-7, 1e-9
        check_rc(eng, eng.lib.phnn_solve_lbfgs(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), None, self.integ,
                                               float(self.dt), C.byref(opt), p["grad"], p["cost"], p["traj"], p["stash"], p["lws"],
                                               self.nws, p["costs"], p["n_iter"], p["func_evals"], eng._stream()))

    def engine(self, eng):
        ws = {}
        r = eng.solve_lbfgs(self.input("x0"), self.input("u"), self.cost, {0: "euler", 1: "rk4"}[self.integ], self.dt, lr=1.0,
                            outer_steps=1, max_iter=self.MAX_ITER, history_size=self.HIST, workspace=ws)
        return {"u": r["u_last"], "costs": r["costs"], "n_iter": r["n_iter"], "func_evals": r["func_evals"], "grad": ws["grad_u"],
                "cost": ws["cost"], "traj": ws["traj"]}


K_SAMPLES, ELITES, SOLVE_ITERS = 6, 2, 2
SEED = 0x1234_5678_9ABC_DEF0


class SampleOp(Op):
    """phnn_mppi_sample / phnn_cem_sample (which: 'mppi' | 'cem'); x0_rep given or NULL."""

    def __init__(self, which, cost, x0, U, rng, with_x0rep=True):
        super().__init__()
        B, H, m = U.shape
        n = x0.shape[1]
        self.name = f"{which}_sample B{B} H{H} m{m} x0rep={int(with_x0rep)}"
        self.which, self.cost, self.B, self.H, self.m, self.with_x0rep = which, cost, B, H, m, with_x0rep
        f = np.float32
        self.add("x0", f, (B, n), IN, x0)
        self.add("u", f, (B, H, m), IN, U)
        if which == "cem":
            self.add("sig", f, (B, H, m), IN, rng.uniform(0.1, 1.0, size=(B, H, m)).astype(f))
        self.add("v", f, (B * K_SAMPLES, H, m), OUT)
        if with_x0rep:
            self.add("x0_rep", f, (B * K_SAMPLES, n), OUT)
        self.sigma = [0.5, 0.25, 1.0, 0.75][:m]

    def call(self, eng, p):
        if self.which == "mppi":
            opt, _ = eng._mppi_options(0, K_SAMPLES, 1.0, self.sigma, SEED, 3, 5)
            check_rc(eng, eng.lib.phnn_mppi_sample(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), C.byref(opt), 1, p["v"],
                                                   p.get("x0_rep"), eng._stream()))
        else:
            opt, _ = eng._cem_options(0, K_SAMPLES, 1, 0.0, 0.0, 0.0, SEED, 3, 5)
            check_rc(eng, eng.lib.phnn_cem_sample(eng.h, p["x0"], p["u"], p["sig"], self.B, self.H, C.byref(self.cost), C.byref(opt), 1,
                                                  p["v"], p.get("x0_rep"), eng._stream()))

    def engine(self, eng):
        import torch
        if self.which == "mppi":
            v, xr = eng.mppi_sample(self.input("x0"), self.input("u"), self.cost, K_SAMPLES, self.sigma, SEED, 1, epoch=3, problem_offset=5)
        else:
            sig = torch.tensor(self.input("sig"), device=eng.device)
            v, xr = eng.cem_sample(self.input("x0"), self.input("u"), sig, self.cost, K_SAMPLES, SEED, 1, epoch=3, problem_offset=5)
        return {"v": v, "x0_rep": xr} if self.with_x0rep else {"v": v}


class UpdateOp(Op):
    """phnn_mppi_update / phnn_cem_update.  best_cost and best_u accumulate across iterations (strict '<' against the value
    on entry, exactly as Adam's), so the test initialises them: problems alternate between a best that every sample beats
    and one that none does.  One problem has only non-finite sample costs (its state is kept)."""

    def __init__(self, which, cost, B, H, m, rng):
        super().__init__()
        f = np.float32
        self.name = f"{which}_update B{B} H{H} m{m}"
        self.which, self.cost, self.B, self.H, self.m = which, cost, B, H, m
        sh = (B, H, m)
        self.add("u", f, sh, INOUT, rng.uniform(-1, 1, size=sh).astype(f))
        if which == "cem":
            self.add("sig", f, sh, INOUT, rng.uniform(0.1, 1.0, size=sh).astype(f))
        self.add("v", f, (B * K_SAMPLES, H, m), IN, rng.uniform(-1.5, 2.0, size=(B * K_SAMPLES, H, m)).astype(f))
        s = rng.uniform(1, 3, size=(B, K_SAMPLES)).astype(f)
        s[:, 1] = np.inf
        if B > 2:
            s[2] = np.nan
        self.add("s", f, (B * K_SAMPLES,), IN, s.reshape(-1))
        self.add("costs_row", f, (B,), OUT)
        self.add("best_cost", f, (B,), INOUT, np.where(np.arange(B) % 2 == 0, 10.0, 0.5).astype(f))
        self.add("best_u", f, sh, INOUT, rng.normal(size=sh).astype(f))

    def call(self, eng, p):
        if self.which == "mppi":
            opt, _ = eng._mppi_options(0, K_SAMPLES, 0.7, 0.0, 0, 0, 0)
            check_rc(eng, eng.lib.phnn_mppi_update(eng.h, p["u"], p["v"], p["s"], self.B, self.H, C.byref(self.cost), C.byref(opt),
                                                   p["costs_row"], p["best_cost"], p["best_u"], eng._stream()))
        else:
            opt, _ = eng._cem_options(0, K_SAMPLES, ELITES, 0.25, 0.0, 0.05, 0, 0, 0)
            check_rc(eng, eng.lib.phnn_cem_update(eng.h, p["u"], p["sig"], p["v"], p["s"], self.B, self.H, C.byref(self.cost),
                                                  C.byref(opt), p["costs_row"], p["best_cost"], p["best_u"], eng._stream()))

    def engine(self, eng):
        import torch
        names = [b.name for b in self.bufs if b.init is not None]
        t = {k: torch.tensor(self.input(k), device=eng.device) for k in names}
        t["costs_row"] = torch.empty(self.B, dtype=torch.float32, device=eng.device)
        if self.which == "mppi":
            eng.mppi_update(t["u"], t["v"], t["s"], 0.7, self.cost, costs_row=t["costs_row"], best_cost=t["best_cost"], best_u=t["best_u"])
        else:
            eng.cem_update(t["u"], t["sig"], t["v"], t["s"], ELITES, 0.25, 0.05, self.cost, costs_row=t["costs_row"],
                           best_cost=t["best_cost"], best_u=t["best_u"])
        return {b.name: t[b.name] for b in self.outputs()}


class SampleSolveOp(Op):
    """phnn_solve_mppi / phnn_solve_cem, K = 6 samples, E = 2 elites, 2 iterations, in a workspace of exactly
    phnn_mppi_workspace_bytes / phnn_cem_workspace_bytes."""

    def __init__(self, which, eng, cost, x0, U, integ, dt, iters=SOLVE_ITERS):
        super().__init__()
        B, H, m = U.shape
        n = x0.shape[1]
        self.name, self.iters = f"solve_{which} B{B} H{H} m{m} integ{integ} iters{iters}", iters
        self.which, self.cost, self.integ, self.dt, self.B, self.H, self.m = which, cost, integ, dt, B, H, m
        f = np.float32
        self.add("x0", f, (B, n), IN, x0)
        self.add("u", f, (B, H, m), INOUT, U)
        self.add("costs", f, (iters, B), OUT)
        self.add("best_cost", f, (B,), OUT)
        self.add("best_u", f, (B, H, m), OUT)
        if which == "cem":
            self.add("sigma_out", f, (B, H, m), OUT)
            self.nws = eng.cem_workspace_bytes(B, H, K_SAMPLES)
        else:
            self.nws = eng.mppi_workspace_bytes(B, H, K_SAMPLES)
        assert self.nws > 0
        self.add("ws", np.uint8, (self.nws,), WS)
        self.sigma = [0.5, 0.25, 1.0, 0.75][:m]

    def call(self, eng, p):
        if self.which == "mppi":
            opt, _ = eng._mppi_options(self.iters, K_SAMPLES, 0.7, self.sigma, SEED, 3, 5)
            check_rc(eng, eng.lib.phnn_solve_mppi(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), None, self.integ,
                                                  float(self.dt), C.byref(opt), p["ws"], self.nws, p["costs"], p["best_cost"],
                                                  p["best_u"], eng._stream()))
        else:
            opt, _ = eng._cem_options(self.iters, K_SAMPLES, ELITES, 0.25, self.sigma, 0.05, SEED, 3, 5)
            check_rc(eng, eng.lib.phnn_solve_cem(eng.h, p["x0"], p["u"], self.B, self.H, C.byref(self.cost), None, self.integ,
                                                 float(self.dt), C.byref(opt), p["ws"], self.nws, p["costs"], p["best_cost"],
                                                 p["best_u"], p["sigma_out"], eng._stream()))

    def engine(self, eng):
        name = {0: "euler", 1: "rk4"}[self.integ]
        kw = dict(iters=self.iters, samples=K_SAMPLES, sigma=self.sigma, seed=SEED, epoch=3, problem_offset=5)
        if self.which == "mppi":
            r = eng.solve_mppi(self.input("x0"), self.input("u"), self.cost, name, self.dt, lam=0.7, **kw)
        else:
            r = eng.solve_cem(self.input("x0"), self.input("u"), self.cost, name, self.dt, elites=ELITES, alpha=0.25, sigma_min=0.05, **kw)
        out = {"u": r["u_last"], "costs": r["costs"], "best_cost": r["best_cost"], "best_u": r["best_u"]}
        if self.which == "cem":
            out["sigma_out"] = r["sigma_last"]
        return out


# ----------------------------------------------------------------------------------------------------- loop kernels
class PlantOp(Op):
    """phnn_plant_step with state_f32, done_step and both logs at step `step` of T.  done_step accumulates (set the first
    time a plant terminates, initialise to -1), so the test initialises it; the logs receive one row per step, so the
    other rows keep the fill and only row step + 1 / step is compared through the whole-buffer bytes of two equal fills --
    the logs are therefore initialised by the test as well (zeros)."""

    def __init__(self, B, T, step, rng):
        super().__init__()
        self.name, self.B, self.T, self.step = f"plant B{B} T{T} step{step}", B, T, step
        st = rng.uniform(-0.4, 0.4, size=(B, 4))
        st[::5, 0] = 10.5  # beyond x_limit: terminates at this step
        done = np.full(B, -1, np.int32)
        done[::10] = 0  # terminated earlier: kept
        self.H = 3
        self.add("state", np.float64, (B, 4), INOUT, st)
        self.add("action", np.float32, (B, self.H), IN, rng.uniform(-2.5, 2.5, size=(B, self.H)).astype(np.float32))
        self.add("state_f32", np.float32, (B, 4), OUT)
        self.add("done_step", np.int32, (B,), INOUT, done)
        self.add("log_states", np.float64, (T + 1, B, 4), INOUT, np.zeros((T + 1, B, 4)))
        self.add("log_controls", np.float32, (T, B), INOUT, np.zeros((T, B), np.float32))

    def call(self, eng, p):
        from phnn_mpc_amd import _capi
        pl = _capi.Plant.default()
        check_rc(eng, eng.lib.phnn_plant_step(eng.h, C.byref(pl), p["state"], p["action"], self.H, self.B, 1, -1.5, 2.0, p["state_f32"],
                                              p["done_step"], None, self.step, p["log_states"], p["log_controls"], eng._stream()))

    def engine(self, eng):
        import torch
        from phnn_mpc_amd import _capi
        t = {b.name: torch.tensor(b.init, device=eng.device) for b in self.bufs if b.init is not None}
        t["state_f32"] = torch.empty(self.B, 4, dtype=torch.float32, device=eng.device)
        eng.plant_step(_capi.Plant.default(), t["state"], t["action"], self.H, u_min=-1.5, u_max=2.0, state_f32=t["state_f32"],
                       done_step=t["done_step"], step=self.step, log_states=t["log_states"], log_controls=t["log_controls"])
        return {b.name: t[b.name] for b in self.outputs()}


class ShiftOp(Op):
    """phnn_shift_controls with a device step counter (an in-place int32, advanced by one)."""

    def __init__(self, B, H, m, rng):
        super().__init__()
        self.name, self.B, self.H, self.m = f"shift B{B} H{H} m{m}", B, H, m
        self.add("src", np.float32, (B, H, m), IN, rng.normal(size=(B, H, m)).astype(np.float32))
        self.add("dst", np.float32, (B, H, m), OUT)
        self.add("step", np.int32, (1,), INOUT, np.array([7], np.int32))

    def call(self, eng, p):
        check_rc(eng, eng.lib.phnn_shift_controls(eng.h, p["src"], p["dst"], self.B, self.H, self.m, p["step"], eng._stream()))

    def engine(self, eng):
        import torch
        src = torch.tensor(self.input("src"), device=eng.device)
        dst, step = torch.empty_like(src), torch.tensor([7], dtype=torch.int32, device=eng.device)
        eng.shift_controls(src, dst, step_dev=step)
        return {"dst": dst, "step": step}


class PackOp(Op):
    """phnn_update_weights_dev from a blob in the arena; the blob region must stay unwritten (it is an IN region: F1 and
    its own bytes).  The packed image is read back by the test through phnn_read_image."""

    def __init__(self, blob):
        super().__init__()
        self.name = "pack"
        self.add("blob", np.float32, blob.shape, IN, blob)

    def call(self, eng, p):
        check_rc(eng, eng.lib.phnn_update_weights_dev(eng.h, p["blob"], self.bufs[0].shape[0], eng._stream()))
