"""RolloutEngine: the thin Python face of the C-ABI (include/phnn_mpc.h) on torch device tensors.

torch is plumbing here (device memory, streams); all arithmetic happens in the gfx950 kernels of
csrc/libphnn_mpc.so.  There is no fallback: without the library or without a GPU, construction raises.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi, weights


class PhnnError(RuntimeError):
    pass


def _check(lib, handle, rc):
    if rc != 0:
        msg = lib.phnn_last_error(handle)
        msg = msg.decode() if msg else ""
        if msg.startswith("Unknown integrator"):
            raise ValueError(msg)  # the reference raises ValueError (src/integrators.py:172,226)
        raise PhnnError(f"phnn_mpc error {rc}: {msg}")


def reference_view(x_ref, B, n, device=None):
    """Strides of a reference trajectory for phnn_reference.

    x_ref: anything broadcastable to (B, rows, n) -- (n,) a setpoint, (rows, n) one trajectory shared by the batch,
    (1 | B, rows, n); a last dimension of 1 broadcasts over the state.  -> (t, batch_stride, time_stride, rows): a
    float32 tensor on `device` (None: x_ref's own) whose element [b, row, i] sits at t.data_ptr() + 4 * (b * batch_stride +
    row * time_stride + i).  A problem or row dimension that is broadcast (size 1, or stride 0 from expand) gets stride 0
    and is not materialised; the data are copied only to make them float32 on `device` or to make the last dimension
    contiguous (then only the distinct elements are copied)."""
    t = torch.as_tensor(x_ref, dtype=torch.float32, device=device)
    shape = tuple(t.shape)
    if not 1 <= t.dim() <= 3:
        raise ValueError(f"x_ref must have 1 to 3 dimensions (n,), (rows, n) or (B, rows, n), got shape {shape}")
    while t.dim() < 3:
        t = t.unsqueeze(0)
    if t.shape[0] not in (1, B) or t.shape[2] not in (1, n) or t.shape[1] < 1 or t.shape[1] >= 2 ** 31:
        raise ValueError(f"x_ref of shape {shape} does not broadcast to (B={B}, rows, n={n})")
    t = t.expand(t.shape[0], t.shape[1], n)
    if n > 1 and t.stride(2) != 1:
        src = t[:1] if t.stride(0) == 0 else t
        src = src[:, :1] if src.stride(1) == 0 else src
        t = src.contiguous().expand(t.shape)
    rows = int(t.shape[1])
    bs = 0 if t.shape[0] == 1 else int(t.stride(0))
    ts = 0 if rows == 1 else int(t.stride(1))
    return t, bs, ts, rows


class RolloutEngine:
    """One dynamics model resident on one GPU.

    state_dict: the reference's state_dict (torch tensors or numpy arrays), or a checkpoint wrapping it.
    """

    supports_reference = True  # rollout_cost / rollout_cost_grad / solve track x_ref (phnn_reference)

    def __init__(self, state_dict, device="cuda:0", kind=None, activation="tanh", matmul=None, force_matmul=False,
                 max_waves=None, split="auto"):
        """matmul: 'default' | 'f32' | 'bf16x3' | 'f16x2' (None: the PHNN_MATMUL environment variable, else
        'default').  The environment is read HERE, on the Python side, as a default only; the C-ABI takes the
        explicit phnn_options.  f16x2 on a model narrower than 128 needs force_matmul=True (known to exceed the
        stated tolerance there).  max_waves (None: PHNN_MAX_WAVES, else 8): waves per workgroup cap.
        split: 'auto' | 'never' | 'always' -- the small-batch kernels that put four waves on every 16-rollout tile
        (bitwise the same results; automatic while the batch has at most two tiles per CU)."""
        self.lib = _capi.load_library()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise PhnnError("RolloutEngine needs a GPU device (cuda:N); there is no CPU path")
        if not torch.cuda.is_available():
            raise PhnnError("no GPU visible to torch; the rollout engine has no CPU fallback")
        self.activation = activation
        self.desc, self.blob = weights.pack_state_dict(state_dict, kind=kind, activation=activation)
        self.n, self.m, self.kind = self.desc.n, self.desc.m, self.desc.kind
        self.layout = weights.blob_layout(state_dict, kind=self.kind)  # [(state_dict key, offset, shape)] of the blob
        self._wg_ws = None
        self._tape_gen, self._tape_token = 0, None  # tapes kept by the last rollout_trajectory(tapes=True), if still valid
        self.use_tapes = os.environ.get("PHNN_NO_TAPES", "0") != "1"
        if matmul is None:
            matmul = os.environ.get("PHNN_MATMUL", "default")
            force_matmul = force_matmul or "PHNN_MATMUL" in os.environ  # an explicit environment override is a force
        if matmul not in _capi.MATMUL_MODES:
            raise ValueError(f"matmul must be one of {sorted(_capi.MATMUL_MODES)}, got {matmul!r}")
        if max_waves is None:
            max_waves = int(os.environ.get("PHNN_MAX_WAVES", "0"))
        self.options = _capi.Options()
        self.options.matmul_mode = _capi.MATMUL_MODES[matmul]
        self.options.force_matmul = int(bool(force_matmul))
        self.options.max_waves = int(max_waves)
        if split not in _capi.SPLIT_MODES:
            raise ValueError(f"split must be one of {sorted(_capi.SPLIT_MODES)}, got {split!r}")
        self.options.split_tiles = _capi.SPLIT_MODES[split]
        # K1 -> K2 activation stash (Euler): on unless PHNN_NO_STASH=1; capped so a huge batch falls back to
        # the recompute kernels instead of allocating more than max_stash_bytes of HBM
        self.use_stash = os.environ.get("PHNN_NO_STASH", "0") != "1"
        self.max_stash_bytes = int(float(os.environ.get("PHNN_MAX_STASH_GB", "96")) * (1 << 30))
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        h = C.c_void_p()
        rc = self.lib.phnn_create_ex(C.byref(self.desc), self.blob.ctypes.data_as(C.POINTER(C.c_float)),
                                     self.blob.size, idx, C.byref(self.options), C.byref(h))
        _check(self.lib, None, rc)
        self.h = h

    def update_weights(self, state_dict):
        """Re-pack and re-upload the weights of the same architecture (after an optimizer step / load_state_dict)."""
        desc, blob = weights.pack_state_dict(state_dict, kind=self.kind, activation=self.activation)
        if blob.size != self.blob.size:
            raise PhnnError("update_weights: the state_dict describes another architecture")
        self.blob = blob
        self._tape_token = None  # tapes of the old weights
        rc = self.lib.phnn_update_weights(self.h, blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, self._stream())
        _check(self.lib, self.h, rc)

    def update_weights_dev(self, blob_dev):
        """The same from a float32 blob on the engine's device (weights.pack_state_dict order, e.g. torch.cat of the
        module's parameters and buffers): padded and packed by one small kernel in stream order -- no device-to-host copy,
        host packing or upload (phnn_update_weights_dev)."""
        if blob_dev.device != self.device or blob_dev.dtype != torch.float32 or not blob_dev.is_contiguous():
            raise PhnnError("update_weights_dev: a contiguous float32 tensor on the engine's device is required")
        if blob_dev.numel() != self.blob.size:
            raise PhnnError("update_weights_dev: the blob describes another architecture")
        self._tape_token = None  # tapes of the old weights
        rc = self.lib.phnn_update_weights_dev(self.h, blob_dev.data_ptr(), blob_dev.numel(), self._stream())
        _check(self.lib, self.h, rc)

    def read_image(self):
        """The packed weight image as the kernels stage it (tests: host-packed vs device-packed)."""
        n = C.c_size_t()
        _check(self.lib, self.h, self.lib.phnn_read_image(self.h, None, 0, C.byref(n), None))
        out = np.empty(n.value, np.float32)
        rc = self.lib.phnn_read_image(self.h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, None, self._stream())
        _check(self.lib, self.h, rc)
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.phnn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _t(self, a, shape=None):
        t = torch.as_tensor(a, dtype=torch.float32, device=self.device)
        if shape is not None:
            if t.numel() == 0:  # an empty batch: -1 is ambiguous for reshape
                shape = tuple(0 if d == -1 else d for d in shape)
            t = t.reshape(shape)
        return t.contiguous()

    def _controls(self, u, B):
        """(B,H,m) view of the controls; H is read from a 3-D input so that B = 0 keeps its horizon."""
        u = self._t(u)
        H = u.shape[1] if u.dim() == 3 else (u.numel() // max(B * self.m, 1))
        return u.reshape(B, H, self.m), H

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def _reference(self, x_ref, ref_offset, B):
        """-> (phnn_reference, tensors to keep alive until the launches are enqueued), or (None, None) without x_ref.
        ref_offset: int >= 0 or a device int32 tensor (its first element is read by every launch; a captured graph
        follows it)."""
        if x_ref is None:
            return None, None
        t, bs, ts, rows = reference_view(x_ref, B, self.n, self.device)
        r = _capi.Reference()
        r.x_ref = t.data_ptr() if t.numel() else None
        r.batch_stride, r.time_stride, r.rows = bs, ts, rows
        if isinstance(ref_offset, torch.Tensor):
            if ref_offset.dtype != torch.int32 or ref_offset.device != self.device or ref_offset.numel() < 1:
                raise ValueError("ref_offset: an int or an int32 tensor on the engine's device")
            r.offset_dev = ref_offset.data_ptr()
        else:
            r.offset_host = int(ref_offset)
        return r, (t, ref_offset)

    def _terminal(self, terminal, B, group=1):
        """-> (phnn_terminal, tensors to keep alive until the launches are enqueued), or (None, None) without one.
        terminal: a terminal.TerminalCost, or an (n,n) / (B,n,n) array or tensor (wrapped in one)."""
        if terminal is None:
            return None, None
        from .terminal import TerminalCost
        if not isinstance(terminal, TerminalCost):
            terminal = TerminalCost(terminal)
        terminal.check(B, self.n)
        W = terminal.tensor(self.device)
        t = _capi.Terminal()
        t.W_dev = W.data_ptr()
        t.batch_stride = self.n * self.n if terminal.per_problem else 0
        t.group = int(group)
        return t, (W, terminal)

    def _roll_call(self, name, ref, x0, u, B, H, cost, *rest):
        """lib.<name>(h, x0, u, B, H, cost, *rest, stream); with a phnn_reference its twin <name>_ref, which takes the
        reference right after the cost."""
        fn = getattr(self.lib, name if ref is None else name + "_ref")
        mid = () if ref is None else (C.byref(ref),)
        _check(self.lib, self.h, fn(self.h, self._p(x0), self._p(u), B, H, C.byref(cost), *mid, *rest, self._stream()))

    def _roll_workspace(self, ws, B, H, integ):
        """The K1 / K2 buffers of a (B, H, integrator) problem in the dict `ws` (None: a fresh one): stash (None above
        max_stash_bytes or without use_stash: K2 recomputes), traj, cost, grad_u, grad_x0.  rollout_cost_grad, solve and
        solve_lbfgs share them, and add their own state next to them; another problem size starts the dict afresh."""
        ws = {} if ws is None else ws
        key = (B, H, integ)
        if ws.get("key") != key:
            ws.clear()
            ws["key"] = key
            nbytes = self.workspace_bytes(B, H, integ) if self.use_stash else 0
            ws["stash"] = (torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                           if 0 < nbytes <= self.max_stash_bytes else None)
            f = dict(dtype=torch.float32, device=self.device)
            ws["traj"], ws["cost"] = torch.empty(B, H + 1, self.n, **f), torch.empty(B, **f)
            ws["grad_u"], ws["grad_x0"] = torch.empty(B, H, self.m, **f), torch.empty(B, self.n, **f)
        return ws

    def _integ(self, integrator):
        if isinstance(integrator, str):
            if integrator not in _capi.INTEGRATORS:
                raise ValueError(f"Unknown integrator: {integrator}")
            return _capi.INTEGRATORS[integrator]
        return int(integrator)

    # ------------------------------------------------------------------ model(x,u), VJP
    def forward(self, x, u):
        x = self._t(x, (-1, self.n))
        u = self._t(u, (-1, self.m))
        B = x.shape[0]
        dx = torch.empty_like(x)
        H = torch.empty(B, dtype=torch.float32, device=self.device)
        _check(self.lib, self.h, self.lib.phnn_model_forward(self.h, self._p(x), self._p(u), B, self._p(dx), self._p(H),
                                                             self._stream()))
        return dx, H

    def vjp(self, x, u, lam):
        x = self._t(x, (-1, self.n))
        u = self._t(u, (-1, self.m))
        lam = self._t(lam, (-1, self.n))
        B = x.shape[0]
        xb = torch.empty_like(x)
        ub = torch.empty(B, self.m, dtype=torch.float32, device=self.device)
        _check(self.lib, self.h, self.lib.phnn_model_vjp(self.h, self._p(x), self._p(u), self._p(lam), B, self._p(xb),
                                                         self._p(ub), self._stream()))
        return xb, ub

    # ------------------------------------------------------------------ rollouts
    def rollout_cost(self, x0, u, cost, integrator="euler", dt=0.02, want_traj=False, traj_out=None, x_ref=None,
                     ref_offset=0):
        """K1.  x0 (B,n), u (B,H,m) -> cost (B) [, traj (B,H+1,n)].  x_ref: a reference trajectory broadcastable to
        (B, rows, n); step t of problem b is then costed about row min(ref_offset + t, rows - 1) of its reference
        instead of cost.x_target (reference_view, phnn_reference)."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        c = torch.empty(B, dtype=torch.float32, device=self.device)
        traj = traj_out
        if traj is None and want_traj:
            traj = torch.empty(B, H + 1, self.n, dtype=torch.float32, device=self.device)
        ref, _keep = self._reference(x_ref, ref_offset, B)
        self._roll_call("phnn_rollout_fwd", ref, x0, u, B, H, cost, self._integ(integrator), float(dt), self._p(c),
                        self._p(traj), None)
        return (c, traj) if (want_traj or traj_out is not None) else c

    def workspace_bytes(self, B, H, integrator="euler"):
        return int(self.lib.phnn_workspace_bytes(self.h, int(B), int(H), self._integ(integrator)))

    def rollout_cost_grad(self, x0, u, cost, integrator="euler", dt=0.02, want_grad_x0=False, workspace=None,
                          after_forward=None, x_ref=None, ref_offset=0):
        """K1 + K2.  -> (cost (B), grad_u (B,H,m)[, grad_x0 (B,n)]).  `workspace`: optional dict reused across
        calls to avoid re-allocating the trajectory / outputs.  `after_forward(cost)` is called once K1 is enqueued
        and before K2 is: the costs are final then, so a collective on them overlaps the adjoint kernel.
        x_ref, ref_offset: reference tracking as in rollout_cost."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        integ = self._integ(integrator)
        ws = self._roll_workspace(workspace, B, H, integ)
        stash = self._p(ws["stash"])
        ref, _keep = self._reference(x_ref, ref_offset, B)
        self._roll_call("phnn_rollout_fwd", ref, x0, u, B, H, cost, integ, float(dt), self._p(ws["cost"]),
                        self._p(ws["traj"]), stash)
        if after_forward is not None:
            after_forward(ws["cost"])
        self._roll_call("phnn_rollout_grad", ref, x0, u, B, H, cost, integ, float(dt), self._p(ws["traj"]), stash,
                        self._p(ws["grad_u"]), self._p(ws["grad_x0"]) if want_grad_x0 else None)
        if want_grad_x0:
            return ws["cost"], ws["grad_u"], ws["grad_x0"]
        return ws["cost"], ws["grad_u"]

    def rollout_vjp(self, x0, u, traj, cost, integrator="euler", dt=0.02, traj_bar=None, cost_bar=None, x_ref=None,
                    ref_offset=0):
        """General reverse pass: cotangents on the trajectory (B,H+1,n) and/or the cost (B) -> (grad_u, grad_x0).
        x_ref, ref_offset: reference tracking as in rollout_cost (phnn_rollout_vjp_ref)."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        traj = self._t(traj, (B, H + 1, self.n))
        tb = self._t(traj_bar, (B, H + 1, self.n)) if traj_bar is not None else None
        cb = self._t(cost_bar, (B,)) if cost_bar is not None else None
        gu = torch.empty(B, H, self.m, dtype=torch.float32, device=self.device)
        gx = torch.empty(B, self.n, dtype=torch.float32, device=self.device)
        ref, _keep = self._reference(x_ref, ref_offset, B)
        self._roll_call("phnn_rollout_vjp", ref, x0, u, B, H, cost, self._integ(integrator), float(dt), self._p(traj), None,
                        self._p(tb), self._p(cb), self._p(gu), self._p(gx))
        return gu, gx

    # ------------------------------------------------------------------ terminal cost and its LQR weight
    def terminal_cost(self, traj, cost, terminal, cost_b, traj_bar=None, want_traj_bar=False, x_ref=None, ref_offset=0,
                      group=1):
        """k_terminal_cost behind a K1 launch: cost_b (B) += e_H^T W e_H in place, with e_H = traj[:, H] - the cost's
        x_target or the reference row min(ref_offset + H, rows - 1).  terminal: a terminal.TerminalCost (or its W);
        row i uses the W of problem i // group.  traj_bar (B,H+1,n): row H receives the gradient of the term, the rows
        before it are not touched (want_traj_bar: a zeroed one is made here).  -> traj_bar or None."""
        traj = self._t(traj)
        B, H = traj.shape[0], traj.shape[1] - 1
        traj = traj.reshape(B, H + 1, self.n)
        self._assert_device_f32(cost_b, traj_bar)
        assert cost_b.numel() == B and (traj_bar is None or traj_bar.numel() == traj.numel())
        if traj_bar is None and want_traj_bar:
            traj_bar = torch.zeros_like(traj)
        g = max(int(group), 1)  # a group < 1 is the library's to refuse
        term, _keep_t = self._terminal(terminal, (B + g - 1) // g, group)
        ref, _keep = self._reference(x_ref, ref_offset, B)
        rc = self.lib.phnn_terminal_cost(self.h, self._p(traj), B, H, C.byref(cost), None if ref is None else C.byref(ref),
                                         None if term is None else C.byref(term), self._p(cost_b), self._p(traj_bar),
                                         self._stream())
        _check(self.lib, self.h, rc)
        return traj_bar

    def dare(self, A, Bm, cost, max_iters=None, tol=None, mu=0.0):
        """k_dare: the Riccati step of tvlqr iterated on the constant A (B,n,n), Bm (B,n,m) from P_0 = Q + Q^T until
        max|P_k - P_{k-1}| <= tol * max|P_k| -> dict(P (B,n,n) float64, K (B,m,n) float64 the gain of the last step,
        W (B,n,n) float32 = 0.5 (P - (Q + Q^T)) the terminal weight, iters (B) int32, status (B) int32: 0 converged,
        1 failed (P, K, W NaN), 2 max_iters reached (the last iterate)).  max_iters / tol None: terminal.DARE_MAX_ITERS /
        terminal.DARE_TOL."""
        from .terminal import DARE_MAX_ITERS, DARE_TOL
        A = self._t(A)
        B = A.shape[0]
        A = A.reshape(B, self.n, self.n)
        Bm = self._t(Bm, (B, self.n, self.m))
        d = dict(dtype=torch.float64, device=self.device)
        P, K = torch.empty(B, self.n, self.n, **d), torch.empty(B, self.m, self.n, **d)
        W = torch.empty(B, self.n, self.n, dtype=torch.float32, device=self.device)
        iters = torch.empty(B, dtype=torch.int32, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        opt = _capi.DareOptions()
        opt.max_iters = int(DARE_MAX_ITERS if max_iters is None else max_iters)
        opt.tol, opt.mu = float(DARE_TOL if tol is None else tol), float(mu)
        rc = self.lib.phnn_dare(self.h, self._p(A), self._p(Bm), B, C.byref(cost), C.byref(opt), self._p(P), self._p(K),
                                self._p(W), self._p(iters), self._p(status), self._stream())
        _check(self.lib, self.h, rc)
        return dict(P=P, K=K, W=W, iters=iters, status=status)

    # ------------------------------------------------------------------ linearisation, TV-LQR gains
    def jacobian(self, x, u):
        """Point Jacobians of the dynamics: x (B,n), u (B,m) -> A (B,n,n) = df/dx, Bm (B,n,m) = df/du, one launch.
        Row i equals vjp(x, u, e_i) bit for bit."""
        x = self._t(x, (-1, self.n))
        u = self._t(u, (-1, self.m))
        B = x.shape[0]
        A = torch.empty(B, self.n, self.n, dtype=torch.float32, device=self.device)
        Bm = torch.empty(B, self.n, self.m, dtype=torch.float32, device=self.device)
        _check(self.lib, self.h, self.lib.phnn_model_jacobian(self.h, self._p(x), self._p(u), B, self._p(A), self._p(Bm),
                                                              self._stream()))
        return A, Bm

    def rollout_linearize(self, x0, u, cost, integrator="euler", dt=0.02, traj=None):
        """The local model of a rollout: A (B,H,n,n) = d x_{t+1} / d x_t and Bm (B,H,n,m) = d x_{t+1} / d u_t (unclamped
        u; a column is 0 where the cost's bounds clamp that control) of the integrator step at (traj[b,t], u[b,t]).
        traj (B,H+1,n): the states K1 wrote for (x0, u); None runs K1 here.  cost None: no clamp (needs traj).
        -> (A, Bm, traj)."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        integ = self._integ(integrator)
        if traj is None:
            if cost is None:
                raise ValueError("rollout_linearize: without a cost the trajectory must be given")
            _, traj = self.rollout_cost(x0, u, cost, integ, dt, want_traj=True)
        else:
            traj = self._t(traj, (B, H + 1, self.n))
        A = torch.empty(B, H, self.n, self.n, dtype=torch.float32, device=self.device)
        Bm = torch.empty(B, H, self.n, self.m, dtype=torch.float32, device=self.device)
        rc = self.lib.phnn_rollout_linearize(self.h, self._p(u), B, H, C.byref(cost) if cost is not None else None, integ,
                                             float(dt), self._p(traj), self._p(A), self._p(Bm), self._stream())
        _check(self.lib, self.h, rc)
        return A, Bm, traj

    def tvlqr(self, A, Bm, cost, mu=0.0, want_P=False):
        """LQ backward pass on (A (B,H,n,n), Bm (B,H,n,m)) with the cost's Q and R, float64: -> dict(K (B,H,m,n) with
        delta u_t = K_t delta x_t, P0 (B,n,n) the cost-to-go at t = 0, P (B,H+1,n,n) or None, status (B) int32: 0, or
        t + 1 where the recursion failed at step t (K_s, P_s for s <= t are NaN then))."""
        A = self._t(A)
        B, H = A.shape[0], A.shape[1]
        A = A.reshape(B, H, self.n, self.n)
        Bm = self._t(Bm, (B, H, self.n, self.m))
        d = dict(dtype=torch.float64, device=self.device)
        K, P0 = torch.empty(B, H, self.m, self.n, **d), torch.empty(B, self.n, self.n, **d)
        P = torch.empty(B, H + 1, self.n, self.n, **d) if want_P else None
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        opt = _capi.TvlqrOptions()
        opt.mu = float(mu)
        rc = self.lib.phnn_tvlqr(self.h, self._p(A), self._p(Bm), B, H, C.byref(cost), C.byref(opt), self._p(K), self._p(P0),
                                 self._p(P), self._p(status), self._stream())
        _check(self.lib, self.h, rc)
        return dict(K=K, P0=P0, P=P, status=status)

    # ------------------------------------------------------------------ training side: parameter gradients (row f4)
    @property
    def has_wgrad(self):
        """True when the handle has weight-gradient kernels (pHNN and canonical pHNN variants)."""
        return self.lib.phnn_wgrad_workspace_bytes(self.h, 16, 1, 0) > 0

    def _wgrad_workspace(self, B, H, integ):
        need = int(self.lib.phnn_wgrad_workspace_bytes(self.h, int(B), int(H), int(integ)))
        if need == 0 and B > 0:
            raise PhnnError("this model variant has no weight-gradient kernels (pHNN and canonical pHNN have them)")
        if self._wg_ws is None or self._wg_ws.numel() < need:
            self._wg_ws = torch.empty(max(need, 1), dtype=torch.uint8, device=self.device)
            self._tape_token = None  # a new buffer: whatever tapes the old one held are gone
        return self._wg_ws

    @property
    def wgrad_workspace(self):
        """The uint8 buffer records, slab and tapes share (None before the first weight-gradient call).  The kernels
        write every byte they later read, so its earlier contents never matter (tests fill it to show that)."""
        return self._wg_ws

    def rollout_trajectory(self, x0, u, integrator="euler", dt=0.02, want_dx=False, tapes=False):
        """Training rollout (no clamp, no cost): x0 (B,n), u (B,H,m) -> traj (B,H+1,n) [, dX (B,H,n) = f(x_t,u_t)].
        tapes=True (models with weight-gradient kernels): K1 also keeps the tapes of every dynamics evaluation in the
        weight-gradient workspace; `self.tape_token` then identifies them, and rollout_wgrad(..., tape_token=that)
        uses them as long as nothing else has touched the workspace or the weights since."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        integ = self._integ(integrator)
        traj = torch.empty(B, H + 1, self.n, dtype=torch.float32, device=self.device)
        dX = torch.empty(B, H, self.n, dtype=torch.float32, device=self.device) if want_dx else None
        ws = None
        if tapes and self.use_tapes and B > 0 and self.has_wgrad:
            ws = self._wgrad_workspace(B, H, integ)
            self._tape_gen += 1
            self._tape_token = (self._tape_gen, B, H, integ, float(dt))
        rc = self.lib.phnn_rollout_trajectory_ws(self.h, self._p(x0), self._p(u), B, H, integ, float(dt), self._p(traj),
                                                 self._p(dX), self._p(ws), self._stream())
        _check(self.lib, self.h, rc)
        return (traj, dX) if want_dx else traj

    @property
    def tape_token(self):
        """Token of the tapes the weight-gradient workspace currently holds (None: none / invalidated)."""
        return self._tape_token

    def rollout_wgrad(self, x0, u, traj, integrator="euler", dt=0.02, traj_bar=None, dx_bar=None, grad_theta=None,
                      accumulate=False, tape_token=None):
        """Reverse pass of a training rollout: cotangents on the trajectory (B,H+1,n) and on the per-step derivatives
        (B,H,n) -> (grad_theta (P,) in weight-blob layout, grad_u (B,H,m), grad_x0 (B,n)).  tape_token: the token
        rollout_trajectory(tapes=True) left for this very rollout; used only if the tapes are still the current ones
        (otherwise the adjoint recomputes the forward pass, same results to rounding)."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        integ = self._integ(integrator)
        traj = self._t(traj, (B, H + 1, self.n))
        tb = self._t(traj_bar, (B, H + 1, self.n)) if traj_bar is not None else None
        db = self._t(dx_bar, (B, H, self.n)) if dx_bar is not None else None
        if grad_theta is None:
            grad_theta = torch.empty(self.blob.size, dtype=torch.float32, device=self.device)
            accumulate = False
        gu = torch.empty(B, H, self.m, dtype=torch.float32, device=self.device)
        gx = torch.empty(B, self.n, dtype=torch.float32, device=self.device)
        ws = self._wgrad_workspace(B, H, integ)
        use_tapes = (tape_token is not None and tape_token == self._tape_token
                     and tape_token[1:] == (B, H, integ, float(dt)))
        if not use_tapes:
            # records and slab of THIS shape start at offset 0 of the shared workspace and may reach into the tape region
            # of whatever (smaller / other-shaped) rollout left its tapes there: those tapes are no longer trustworthy
            self._tape_token = None
        flags = (_capi.WGRAD_ACCUMULATE if accumulate else 0) | (_capi.WGRAD_TAPES if use_tapes else 0)
        rc = self.lib.phnn_rollout_wgrad(self.h, self._p(x0), self._p(u), B, H, integ, float(dt), self._p(traj),
                                         self._p(tb), self._p(db), self._p(ws), self._p(grad_theta), flags,
                                         self._p(gu), self._p(gx), self._stream())
        _check(self.lib, self.h, rc)
        return grad_theta, gu, gx

    def model_wgrad(self, x, u, lam, Hbar=None, grad_theta=None, accumulate=False):
        """Single evaluations: -> (grad_theta (P,) of sum lam.f + Hbar H, xbar (N,n), ubar (N,m))."""
        x = self._t(x, (-1, self.n))
        u = self._t(u, (-1, self.m))
        lam = self._t(lam, (-1, self.n))
        N = x.shape[0]
        hb = self._t(Hbar, (N,)) if Hbar is not None else None
        if grad_theta is None:
            grad_theta = torch.empty(self.blob.size, dtype=torch.float32, device=self.device)
            accumulate = False
        xb = torch.empty_like(x)
        ub = torch.empty(N, self.m, dtype=torch.float32, device=self.device)
        ws = self._wgrad_workspace(N, 0, 0)
        self._tape_token = None  # point-mode records may reach into the tape region of a rollout-sized workspace
        rc = self.lib.phnn_model_wgrad(self.h, self._p(x), self._p(u), self._p(lam), self._p(hb), N, self._p(ws),
                                       self._p(grad_theta), int(accumulate), self._p(xb), self._p(ub), self._stream())
        _check(self.lib, self.h, rc)
        return grad_theta, xb, ub

    def mass_cotangents(self, B, H=0, integrator="euler"):
        """(q (P,2), Mbar (P,2,2)) of the evaluation points of the LAST rollout_wgrad(B, H, integrator) / model_wgrad(B
        points, H = 0) call, read from the records in the weight-gradient workspace -- canonical models with a
        MassMatrixNetwork: the cotangent of M(q) at every evaluation (phnn_wgrad_record_info).  P = 16 * records: points
        beyond the batch carry zero cotangents."""
        rf, so, ss = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self.lib, self.h, self.lib.phnn_wgrad_record_info(self.h, C.byref(rf), C.byref(so), C.byref(ss)))
        tiles = (int(B) + 15) // 16
        n_rec = tiles if H <= 0 else tiles * int(H) * (4 if self._integ(integrator) == 1 else 1)
        rec = self._wg_ws.view(torch.float32)[: n_rec * rf.value].view(n_rec, rf.value)
        sm = rec[:, so.value:].reshape(n_rec * 16, ss.value)
        return sm[:, 24:26], sm[:, 20:24].reshape(-1, 2, 2)

    def named_grads(self, grad_theta):
        """{state_dict key: tensor view of the parameter's shape} of a gradient blob."""
        return weights.unpack_grad_blob(None, grad_theta, layout=self.layout)

    # ------------------------------------------------------------------ Adam on the controls (K3)
    def adam_step(self, u, grad, exp_avg, exp_avg_sq, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, cost=None,
                  best_cost=None, best_u=None, u_min=None, u_max=None):
        """In-place torch.optim.Adam step on u (B,H,m) (+ optional best-iterate tracking)."""
        for t in (u, grad, exp_avg, exp_avg_sq):
            assert t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device
        per = u[0].numel() if u.dim() > 1 else 1
        has_b = u_min is not None and u_max is not None
        rc = self.lib.phnn_adam_step(self.h, self._p(u), self._p(grad), self._p(exp_avg), self._p(exp_avg_sq),
                                     u.numel(), float(lr), float(beta1), float(beta2), float(eps), int(step),
                                     self._p(cost), self._p(best_cost), self._p(best_u), per,
                                     float(u_min) if has_b else 0.0, float(u_max) if has_b else 0.0, int(has_b),
                                     self._stream())
        _check(self.lib, self.h, rc)

    # ------------------------------------------------------------------ the whole shooting solve (K1, K2, K3 x iters)
    def solve(self, x0, u_init, cost, integrator="euler", dt=0.02, lr=0.015, iters=30, track_best=False, record_costs=True,
              beta1=0.9, beta2=0.999, eps=1e-8, workspace=None, x_ref=None, ref_offset=0, terminal=None):
        """phnn_solve: Adam on the control sequences of B independent problems, the loops of
        src/mpc_controller.py:164-209 / src/mpc_controller_canonical.py:163-228, as ONE library call that enqueues the
        K1 / K2 / K3 launches of every iteration (no Python between them).  -> dict as solver.shooting_solve, same
        results bit for bit.  workspace: optional dict reused across calls (K1 / K2 buffers and Adam's moments).
        x_ref, ref_offset: every problem tracks its own reference (rollout_cost; phnn_solve_ref).
        terminal: a terminal.TerminalCost (or its W): phnn_solve_term -- every K1 is followed by k_terminal_cost, K2 reads
        its cotangent, and costs / best_cost are total costs.  None: the calls and bits of before."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u_init, H = self._controls(u_init, B)
        integ = self._integ(integrator)
        ws = self._roll_workspace(workspace, B, H, integ)
        f = dict(dtype=torch.float32, device=self.device)
        if "m" not in ws:  # Adam's moments; phnn_solve zeroes them
            ws["m"], ws["v"] = torch.empty(B, H, self.m, **f), torch.empty(B, H, self.m, **f)
        u = u_init.detach().clone().contiguous()
        costs = torch.empty(int(iters), B, **f) if record_costs else None
        best_cost = torch.empty(B, **f) if track_best else None
        best_u = torch.empty(B, H, self.m, **f) if track_best else None
        if track_best and int(iters) == 0:  # phnn_solve returns before its state reset: shooting_solve's initial values
            best_cost.fill_(float("inf"))
            best_u.zero_()
        opt = _capi.SolveOptions(int(iters), float(lr), float(beta1), float(beta2), float(eps), int(bool(track_best)))
        ref, _keep = self._reference(x_ref, ref_offset, B)
        term, _keep_t = self._terminal(terminal, B)
        if term is not None:
            if "traj_bar" not in ws:  # the cotangent K2 reads; phnn_solve_term zeroes it
                ws["traj_bar"] = torch.empty(B, H + 1, self.n, **f)
            rc = self.lib.phnn_solve_term(self.h, self._p(x0), self._p(u), B, H, C.byref(cost),
                                          None if ref is None else C.byref(ref), C.byref(term), integ, float(dt),
                                          C.byref(opt), self._p(ws["m"]), self._p(ws["v"]), self._p(ws["grad_u"]),
                                          self._p(ws["cost"]), self._p(ws["traj"]), self._p(ws["stash"]), self._p(costs),
                                          self._p(best_cost), self._p(best_u), self._p(ws["traj_bar"]), self._stream())
            _check(self.lib, self.h, rc)
        else:
            self._roll_call("phnn_solve", ref, x0, u, B, H, cost, integ, float(dt), C.byref(opt), self._p(ws["m"]),
                            self._p(ws["v"]), self._p(ws["grad_u"]), self._p(ws["cost"]), self._p(ws["traj"]),
                            self._p(ws["stash"]), self._p(costs), self._p(best_cost), self._p(best_u))
        out = {"u_last": u, "costs": costs}
        if track_best:
            out["best_u"], out["best_cost"] = best_u, best_cost
        return out

    # ------------------------------------------------------------------ batched L-BFGS solve (K1, K2, k_lbfgs)
    def lbfgs_workspace_bytes(self, B, H, history_size=100):
        return int(self.lib.phnn_lbfgs_workspace_bytes(self.h, int(B), int(H), int(history_size)))

    def solve_lbfgs(self, x0, u_init, cost, integrator="euler", dt=0.02, lr=1.0, outer_steps=1, max_iter=20, max_eval=None,
                    tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100, record_costs=True, workspace=None,
                    x_ref=None, ref_offset=0, terminal=None):
        """phnn_solve_lbfgs: B independent torch.optim.LBFGS(lr, max_iter, max_eval, tolerance_grad, tolerance_change,
        history_size) optimizers, each created fresh and stepped outer_steps times on its problem's K1 cost and K2
        gradient (src/mpc_controller.py:169-170,196-197), as ONE library call: outer_steps x max_iter x (K1, K2,
        k_lbfgs) launches.  -> dict(u_last (B,H,m) unclamped last iterate, costs (outer_steps,B) orig_loss of every
        step() or None, n_iter (B) int32 state['n_iter'], func_evals (B) int32 state['func_evals']).
        workspace: optional dict reused across calls (K1 / K2 buffers and the optimizer state).  x_ref, ref_offset:
        every problem tracks its own reference (rollout_cost).  terminal: refused (the L-BFGS solve has no terminal term)."""
        from .terminal import refuse
        refuse(terminal, "the L-BFGS solve")
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u_init, H = self._controls(u_init, B)
        integ = self._integ(integrator)
        ws = self._roll_workspace(workspace, B, H, integ)
        if ws.get("lbfgs_history") != int(history_size):
            ws["lbfgs_history"] = int(history_size)
            ws["lbfgs_state"] = torch.empty(max(self.lbfgs_workspace_bytes(B, H, history_size), 1), dtype=torch.uint8,
                                            device=self.device)
        u = u_init.detach().clone().contiguous()
        costs = torch.empty(int(outer_steps), B, dtype=torch.float32, device=self.device) if record_costs else None
        n_iter = torch.empty(B, dtype=torch.int32, device=self.device)
        func_evals = torch.empty(B, dtype=torch.int32, device=self.device)
        opt = _capi.LbfgsOptions()
        opt.outer_steps, opt.max_iter = int(outer_steps), int(max_iter)
        opt.max_eval = 0 if max_eval is None else int(max_eval)
        opt.history_size = int(history_size)
        opt.lr, opt.tolerance_grad, opt.tolerance_change = float(lr), float(tolerance_grad), float(tolerance_change)
        if max_eval is not None and int(max_eval) < 1:
            raise ValueError("max_eval must be >= 1 (None: torch's default max_iter * 5 // 4)")
        ref, _keep = self._reference(x_ref, ref_offset, B)
        rc = self.lib.phnn_solve_lbfgs(self.h, self._p(x0), self._p(u), B, H, C.byref(cost),
                                       None if ref is None else C.byref(ref), integ, float(dt), C.byref(opt),
                                       self._p(ws["grad_u"]), self._p(ws["cost"]), self._p(ws["traj"]),
                                       self._p(ws["stash"]), self._p(ws["lbfgs_state"]), ws["lbfgs_state"].numel(),
                                       self._p(costs), self._p(n_iter), self._p(func_evals), self._stream())
        _check(self.lib, self.h, rc)
        return {"u_last": u, "costs": costs, "n_iter": n_iter, "func_evals": func_evals}

    # ------------------------------------------------------------------ batched sampling solves, MPPI and CEM (k_sample, K1, k_mppi_update / k_cem_update)
    def mppi_workspace_bytes(self, B, H, samples):
        return int(self.lib.phnn_mppi_workspace_bytes(self.h, int(B), int(H), int(samples)))

    def cem_workspace_bytes(self, B, H, samples):
        return int(self.lib.phnn_cem_workspace_bytes(self.h, int(B), int(H), int(samples)))

    def _sampling_options(self, opt, sigma_field, iters, samples, sigma, seed, epoch, problem_offset):
        """Fills what phnn_mppi_options and phnn_cem_options share -> (opt, what to keep alive).  sigma (into the struct's
        sigma_field): one value or one per control component; epoch: int or a device int32 tensor (its first element is
        read by every launch; a captured graph follows it)."""
        opt.iters, opt.samples = int(iters), int(samples)
        sig = np.asarray(sigma, dtype=np.float64).reshape(-1)
        if sig.size == 1:
            sig = np.repeat(sig, self.m)
        if sig.shape != (self.m,):
            raise ValueError(f"sigma: one value or one per control component (m = {self.m}), got {sigma!r}")
        for i in range(self.m):
            sigma_field[i] = float(sig[i])
        if not 0 <= int(seed) < 2 ** 64:
            raise ValueError("seed must fit 64 bits")
        opt.seed, opt.problem_offset = int(seed), int(problem_offset)
        if isinstance(epoch, torch.Tensor):
            if epoch.dtype != torch.int32 or epoch.device != self.device or epoch.numel() < 1:
                raise ValueError("epoch: an int or an int32 tensor on the engine's device")
            opt.epoch_dev = epoch.data_ptr()
        else:
            opt.epoch_host = int(epoch)
        return opt, epoch

    def _mppi_options(self, iters, samples, lam, sigma, seed, epoch, problem_offset):
        """-> (phnn_mppi_options, what to keep alive); sigma and the counter fields as in _sampling_options."""
        opt = _capi.MppiOptions()
        setattr(opt, "lambda", float(lam))
        return self._sampling_options(opt, opt.sigma, iters, samples, sigma, seed, epoch, problem_offset)

    def _cem_options(self, iters, samples, elites, alpha, sigma, sigma_min, seed, epoch, problem_offset):
        """-> (phnn_cem_options, what to keep alive).  sigma: the initial standard deviation."""
        opt = _capi.CemOptions()
        opt.elites, opt.alpha, opt.sigma_min = int(elites), float(alpha), float(sigma_min)
        return self._sampling_options(opt, opt.sigma_init, iters, samples, sigma, seed, epoch, problem_offset)

    def _sampling_buffers(self, ws, meth, B, H, samples):
        """The sample tensor (B*K, H, m), replicated x0 (B*K, n), K1 cost vector (B*K) and, for CEM, the sigma state
        (B, H, m) of a sampling problem, as views ws[meth + "_v" | "_x0" | "_s" | "_sig"] of one
        phnn_<meth>_workspace_bytes buffer ws[meth] kept in the dict `ws` (the layout phnn_solve_<meth> uses)."""
        key = (B, H, int(samples))
        if ws.get(meth + "_key") != key:
            ws[meth + "_key"] = key
            nbytes = getattr(self, meth + "_workspace_bytes")(B, H, samples)  # 0: arguments the library call itself will refuse
            buf = ws[meth] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            nb = B if nbytes else 0
            R = nb * int(samples)
            regions = [("_v", (R, H, self.m)), ("_x0", (R, self.n)), ("_s", (R,))] + [("_sig", (nb, H, self.m))] * (meth == "cem")
            off = 0
            for name, shape in regions:  # each region 256-byte aligned
                end = off + 4 * int(np.prod(shape))
                ws[meth + name] = buf[off:end].view(torch.float32).view(shape)
                off = (end + 255) & ~255
        return ws

    def _mppi_buffers(self, ws, B, H, samples):
        return self._sampling_buffers(ws, "mppi", B, H, samples)

    def _cem_buffers(self, ws, B, H, samples):
        return self._sampling_buffers(ws, "cem", B, H, samples)

    def mppi_reference(self, x_ref, B, samples):
        """The reference as the B * samples rollouts of a sampling solve see it: one shared by all problems goes straight
        through (batch stride 0); a per-problem one is expanded on the device to one row set per rollout (rollout
        b * samples + k tracks problem b's), samples times its bytes."""
        if x_ref is None:
            return None
        t, bs, ts, _rows = reference_view(x_ref, B, self.n, self.device)
        if bs == 0:
            return t[:1]
        return (t[:, :1] if ts == 0 else t).repeat_interleave(int(samples), dim=0)

    def _assert_device_f32(self, *tensors):
        for t in tensors:
            assert t is None or (t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device)

    def _noise_shape(self, noise):
        """noise (noise.Noise, or an (H, P) array wrapped here) -> (phnn_noise_shape on this device, what to keep alive)."""
        from .noise import Noise
        noise = noise if isinstance(noise, Noise) else Noise(noise.detach().cpu().numpy() if isinstance(noise, torch.Tensor) else noise)
        return noise.struct(self.device), noise

    def _sample(self, meth, opt, x0, u, sig, cost, iteration, workspace, noise=None):
        """phnn_<meth>_sample (noise None) or phnn_<meth>_sample_shaped; sig: the method's extra input tensors (CEM's
        standard deviation)."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        self._assert_device_f32(*sig)
        assert all(t.numel() == u.numel() for t in sig)
        ws = self._sampling_buffers({} if workspace is None else workspace, meth, B, H, opt.samples)
        head = (self.h, self._p(x0), self._p(u), *map(self._p, sig), B, H, C.byref(cost), C.byref(opt), int(iteration))
        tail = (self._p(ws[meth + "_v"]), self._p(ws[meth + "_x0"]), self._stream())
        if noise is None:
            rc = getattr(self.lib, f"phnn_{meth}_sample")(*head, *tail)
        else:
            shape, _keep = self._noise_shape(noise)
            rc = getattr(self.lib, f"phnn_{meth}_sample_shaped")(*head, C.byref(shape), *tail)
        _check(self.lib, self.h, rc)
        return ws[meth + "_v"], ws[meth + "_x0"]

    def mppi_sample(self, x0, u, cost, samples, sigma, seed, iteration, epoch=0, problem_offset=0, workspace=None, noise=None):
        """k_sample with MPPI's sigma.  x0 (B,n), nominal u (B,H,m) -> (v (B*samples,H,m), x0 replicated (B*samples,n)):
        sample b * samples + k is clamp(u_b + sigma o z), z standard normal from the Philox counter (seed, epoch, iteration,
        problem_offset + b, k) and zero for k = 0.  The outputs are views of `workspace` (a dict reused across calls).
        noise: None = white; a noise.Noise (or an (H, P) array) = k_shaped_sample, z[t, c] = sum_s L[t, s] eps[s, c]."""
        opt, _keep = self._mppi_options(0, samples, 1.0, sigma, seed, epoch, problem_offset)
        return self._sample("mppi", opt, x0, u, (), cost, iteration, workspace, noise)

    def cem_sample(self, x0, u, sig, cost, samples, seed, iteration, epoch=0, problem_offset=0, workspace=None, noise=None):
        """k_sample with CEM's sigma: as mppi_sample with a standard deviation sig (B,H,m) per problem and element,
        sample b * samples + k = clamp(u_b + sig_b o z).  noise: as in mppi_sample."""
        opt, _keep = self._cem_options(0, samples, 1, 0.0, 0.0, 0.0, seed, epoch, problem_offset)
        return self._sample("cem", opt, x0, u, (sig,), cost, iteration, workspace, noise)

    def _update(self, meth, options, u, sig, v, s, cost, costs_row, best_cost, best_u):
        """phnn_<meth>_update; options(samples) -> the method's options struct, sig as in _sample."""
        self._assert_device_f32(u, *sig, v, s, costs_row, best_cost, best_u)
        B, H = u.shape[0], u.shape[1]
        samples = s.numel() // max(B, 1)
        assert v.numel() == B * samples * H * self.m and s.numel() == B * samples and all(t.numel() == u.numel() for t in sig)
        opt, _keep = options(samples)
        rc = getattr(self.lib, f"phnn_{meth}_update")(self.h, self._p(u), *map(self._p, sig), self._p(v), self._p(s), B, H,
                                                      C.byref(cost), C.byref(opt), self._p(costs_row), self._p(best_cost),
                                                      self._p(best_u), self._stream())
        _check(self.lib, self.h, rc)

    def mppi_update(self, u, v, s, lam, cost, costs_row=None, best_cost=None, best_u=None):
        """k_mppi_update, in place on the nominal u (B,H,m): u_b = clamp(sum_k w_k v_{b,k} / sum_k w_k) with
        w_k = exp(-(s_{b,k} - min_k s_b) / lam) over the samples v (B*K,H,m) of costs s (B*K); the clamp is the cost's.  costs_row (B) receives
        s_{b,0}; best_cost (B) / best_u (B,H,m) the lowest-cost sample seen so far (strict '<', lowest k on ties)."""
        self._update("mppi", lambda K: self._mppi_options(0, K, lam, 0.0, 0, 0, 0), u, (), v, s, cost, costs_row, best_cost, best_u)

    def cem_update(self, u, sig, v, s, elites, alpha, sigma_min, cost, costs_row=None, best_cost=None, best_u=None):
        """k_cem_update, in place on the mean u and the standard deviation sig (B,H,m): both refitted to the `elites`
        samples of lowest finite cost (cost, then sample index) among v (B*K,H,m) with costs s (B*K):
        u = clamp(alpha u + (1 - alpha) mean), sig = max(sigma_min, sqrt(alpha sig^2 + (1 - alpha) var)); the clamp is
        the cost's.  costs_row (B) receives s_{b,0}; best_cost (B) / best_u (B,H,m) the lowest-cost sample seen so far."""
        self._update("cem", lambda K: self._cem_options(0, K, elites, alpha, 0.0, sigma_min, 0, 0, 0), u, (sig,), v, s, cost,
                     costs_row, best_cost, best_u)

    def _solve_sampling(self, meth, opt, x0, u_init, cost, integrator, dt, record_costs, workspace, x_ref, ref_offset,
                        expanded_ref, noise=None):
        """phnn_solve_<meth> (noise None) or phnn_solve_<meth>_shaped -> dict(u_last, [sigma_last (CEM),] costs, best_u,
        best_cost)."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u_init, H = self._controls(u_init, B)
        integ = self._integ(integrator)
        ws = self._sampling_buffers(self._roll_workspace(workspace, B, H, integ), meth, B, H, opt.samples)
        f = dict(dtype=torch.float32, device=self.device)
        u = u_init.detach().clone().contiguous()
        costs = torch.empty(max(opt.iters, 0), B, **f) if record_costs else None
        best_cost, best_u = torch.empty(B, **f), torch.empty(B, H, self.m, **f)
        sig = (torch.empty(B, H, self.m, **f),) if meth == "cem" else ()
        ref, _keep_ref = self._reference(x_ref if expanded_ref else self.mppi_reference(x_ref, B, opt.samples), ref_offset,
                                         B * opt.samples)
        head = (self.h, self._p(x0), self._p(u), B, H, C.byref(cost), None if ref is None else C.byref(ref), integ, float(dt),
                C.byref(opt))
        tail = (self._p(ws[meth]), ws[meth].numel(), self._p(costs), self._p(best_cost), self._p(best_u), *map(self._p, sig),
                self._stream())
        if noise is None:
            rc = getattr(self.lib, "phnn_solve_" + meth)(*head, *tail)
        else:
            shape, _keep_noise = self._noise_shape(noise)
            rc = getattr(self.lib, f"phnn_solve_{meth}_shaped")(*head, C.byref(shape), *tail)
        _check(self.lib, self.h, rc)
        return {"u_last": u, **({"sigma_last": sig[0]} if sig else {}), "costs": costs, "best_u": best_u, "best_cost": best_cost}

    def solve_mppi(self, x0, u_init, cost, integrator="euler", dt=0.02, iters=4, samples=64, lam=1.0, sigma=1.0, seed=0,
                   epoch=0, problem_offset=0, record_costs=True, workspace=None, x_ref=None, ref_offset=0, expanded_ref=False,
                   noise=None, terminal=None):
        """phnn_solve_mppi: sampling MPC (MPPI) on B independent problems as ONE library call: the nominal is clamped,
        then iters x (k_sample, K1 over B * samples rollouts, k_mppi_update); no gradient is taken anywhere.
        -> dict(u_last (B,H,m) last nominal (in bounds), costs (iters,B) the nominal's cost at every iteration or None,
        best_u (B,H,m) / best_cost (B) the best sample over all iterations), same results bit for bit as
        solver.mppi_solve.  sigma: noise standard deviation, one value or one per control component; lam: softmin
        temperature in units of the cost; seed, epoch (int or device int32 tensor), problem_offset: the noise counter
        (problem b's noise depends on problem_offset + b, not on the batch).  x_ref, ref_offset: as in rollout_cost; a
        per-problem reference is expanded to one row set per rollout (mppi_reference: samples times its bytes) once per
        call, unless expanded_ref says x_ref already is what mppi_reference returned (a closed loop expands it once).
        noise: None = white noise; a noise.Noise (or an (H, P) array) = time-correlated noise (phnn_solve_mppi_shaped:
        k_shaped_sample in k_sample's place, everything else as it is); a captured graph reads its device tensor in place.
        terminal: refused (the sampling solves have no terminal term)."""
        from .terminal import refuse
        refuse(terminal, "the MPPI solve")
        opt, _keep = self._mppi_options(iters, samples, lam, sigma, seed, epoch, problem_offset)
        return self._solve_sampling("mppi", opt, x0, u_init, cost, integrator, dt, record_costs, workspace, x_ref, ref_offset,
                                    expanded_ref, noise)

    def solve_cem(self, x0, u_init, cost, integrator="euler", dt=0.02, iters=4, samples=64, elites=8, alpha=0.25, sigma=1.0,
                  sigma_min=0.05, seed=0, epoch=0, problem_offset=0, record_costs=True, workspace=None, x_ref=None,
                  ref_offset=0, expanded_ref=False, noise=None, terminal=None):
        """phnn_solve_cem: sampling MPC by the cross-entropy method on B independent problems as ONE library call: the
        mean is clamped and the standard deviation set to sigma, then iters x (k_sample, K1 over B * samples
        rollouts, k_cem_update); no gradient is taken anywhere.  -> dict(u_last (B,H,m) last mean (in bounds), sigma_last
        (B,H,m) last standard deviation, costs (iters,B) the mean's cost at every iteration or None, best_u (B,H,m) /
        best_cost (B) the best sample over all iterations), same results bit for bit as solver.cem_solve.  elites: how
        many of the lowest-cost samples mean and standard deviation are refitted to; alpha: smoothing in [0, 1);
        sigma: initial standard deviation, one value or one per control component; sigma_min: its floor.  seed, epoch,
        problem_offset, x_ref, ref_offset, expanded_ref, noise (phnn_solve_cem_shaped): as in solve_mppi.  terminal: refused."""
        from .terminal import refuse
        refuse(terminal, "the cross-entropy solve")
        opt, _keep = self._cem_options(iters, samples, elites, alpha, sigma, sigma_min, seed, epoch, problem_offset)
        return self._solve_sampling("cem", opt, x0, u_init, cost, integrator, dt, record_costs, workspace, x_ref, ref_offset,
                                    expanded_ref, noise)

    # ------------------------------------------------------------------ batched Gauss-Newton solve
    def gn_workspace_bytes(self, B, H, line_steps):
        return int(self.lib.phnn_gn_workspace_bytes(self.h, int(B), int(H), int(line_steps)))

    @staticmethod
    def _gn_options(iters, line_steps, mu_init, mu_min, mu_max, mu_up, mu_down):
        opt = _capi.GnOptions()
        opt.iters, opt.line_steps = int(iters), int(line_steps)
        opt.mu_init, opt.mu_min, opt.mu_max = float(mu_init), float(mu_min), float(mu_max)
        opt.mu_up, opt.mu_down = float(mu_up), float(mu_down)
        return opt

    def _mu(self, mu, B):
        """(B,) float64 on the device from a tensor of that shape or one value."""
        if isinstance(mu, torch.Tensor):
            return mu.to(device=self.device, dtype=torch.float64).reshape(B).contiguous()
        return torch.full((B,), float(mu), dtype=torch.float64, device=self.device)

    def gn_direction(self, A, Bm, traj, u, cost, mu, x_ref=None, ref_offset=0, box=False, terminal=None):
        """k_gn_direction: the Gauss-Newton step of every problem on its local model.  A (B,H,n,n), Bm (B,H,n,m) from
        rollout_linearize, traj (B,H+1,n), u (B,H,m), mu (B) float64 or one value; x_ref / ref_offset: problem b's
        reference as in rollout_cost.  -> dict(du (B,H,m) float32, dV (B) float64 -- the cost's slope along du is -dV,
        the predicted change at the full step -dV/2 --, status (B) int32 as tvlqr's).  A failed problem has du = 0 and
        dV = NaN.  box: k_gn_direction_box, the step with the cost's control bounds inside the LQ problem (DESIGN.md
        section 19); the dict gains nclamp (B) int32, the (t, component) pairs held on a bound.  terminal: a
        terminal.TerminalCost (or its W): the backward sweep starts from the stage terms at H plus the terminal weight's
        (phnn_gn_direction_term)."""
        A = self._t(A)
        B, H = A.shape[0], A.shape[1]
        A = A.reshape(B, H, self.n, self.n)
        Bm, traj, u = self._t(Bm, (B, H, self.n, self.m)), self._t(traj, (B, H + 1, self.n)), self._t(u, (B, H, self.m))
        mu = self._mu(mu, B)
        du = torch.empty(B, H, self.m, dtype=torch.float32, device=self.device)
        dV = torch.empty(B, dtype=torch.float64, device=self.device)
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        scratch = torch.empty(B * H * (self.m * self.n + self.m), dtype=torch.float64, device=self.device)
        ref, _keep = self._reference(x_ref, ref_offset, B)
        head = (self.h, self._p(A), self._p(Bm), self._p(traj), self._p(u), B, H, C.byref(cost),
                None if ref is None else C.byref(ref), self._p(mu), self._p(du), self._p(dV), self._p(status))
        term, _keep_t = self._terminal(terminal, B)
        if term is not None:
            nclamp = torch.empty(B, dtype=torch.int32, device=self.device) if box else None
            rc = self.lib.phnn_gn_direction_term(*head[:9], C.byref(term), *head[9:], _capi.PHNN_GN_BOX if box else 0,
                                                 self._p(nclamp), self._p(scratch), self._stream())
            _check(self.lib, self.h, rc)
            out = dict(du=du, dV=dV, status=status)
            if box:
                out["nclamp"] = nclamp
            return out
        if box:
            nclamp = torch.empty(B, dtype=torch.int32, device=self.device)
            rc = self.lib.phnn_gn_direction_box(*head, self._p(nclamp), self._p(scratch), self._stream())
            _check(self.lib, self.h, rc)
            return dict(du=du, dV=dV, status=status, nclamp=nclamp)
        rc = self.lib.phnn_gn_direction(*head, self._p(scratch), self._stream())
        _check(self.lib, self.h, rc)
        return dict(du=du, dV=dV, status=status)

    def gn_candidates(self, x0, u, du, cost, line_steps):
        """k_gn_candidates: -> (cand (B*L,H,m), x0 replicated (B*L,n)); row b*L + j = clamp(u_b + 2^-j du_b), the clamp
        the cost's."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u, H = self._controls(u, B)
        du = self._t(du, (B, H, self.m))
        L = int(line_steps)
        rows = B * L if 1 <= L <= 32 else 0  # the library call refuses another L
        cand = torch.empty(rows, H, self.m, dtype=torch.float32, device=self.device)
        x0_rep = torch.empty(rows, self.n, dtype=torch.float32, device=self.device)
        rc = self.lib.phnn_gn_candidates(self.h, self._p(x0), self._p(u), self._p(du), B, H, C.byref(cost), L, self._p(cand),
                                         self._p(x0_rep), self._stream())
        _check(self.lib, self.h, rc)
        return cand, x0_rep

    def gn_select(self, u, traj, cost_b, mu, accepts, cand, cand_cost, cand_traj, status, line_steps, mu_min, mu_max, mu_up,
                  mu_down, costs_row=None, alpha_row=None):
        """k_gn_select, in place on u (B,H,m), traj (B,H+1,n), cost_b (B), mu (B) float64 and accepts (B) int32: problem
        b takes its lowest-cost finite candidate (lowest j on ties) iff status_b == 0 and that cost is < cost_b; mu
        shrinks by mu_down (floor mu_min) then, else grows by mu_up (cap mu_max).  costs_row (B) receives cost_b as it
        was, alpha_row (B) the accepted step length or 0."""
        self._assert_device_f32(u, traj, cost_b, cand, cand_cost, cand_traj, costs_row, alpha_row)
        assert mu.dtype == torch.float64 and accepts.dtype == torch.int32 and status.dtype == torch.int32
        assert all(t.is_contiguous() and t.device == self.device for t in (mu, accepts, status))
        B, H = u.shape[0], u.shape[1]
        L = int(line_steps)
        assert cand.numel() == B * L * H * self.m and cand_cost.numel() == B * L and cand_traj.numel() == B * L * (H + 1) * self.n
        opt = self._gn_options(0, L, 0.0, mu_min, mu_max, mu_up, mu_down)
        rc = self.lib.phnn_gn_select(self.h, self._p(u), self._p(traj), self._p(cost_b), self._p(mu), self._p(accepts),
                                     self._p(cand), self._p(cand_cost), self._p(cand_traj), self._p(status), B, H,
                                     C.byref(opt), self._p(costs_row), self._p(alpha_row), self._stream())
        _check(self.lib, self.h, rc)

    def solve_gn(self, x0, u_init, cost, integrator="euler", dt=0.02, iters=10, line_steps=8, mu_init=1e-6, mu_min=1e-9,
                 mu_max=1e6, mu_up=10.0, mu_down=0.1, record_costs=True, workspace=None, x_ref=None, ref_offset=0,
                 expanded_ref=False, box=False, terminal=None):
        """phnn_solve_gn: projected Gauss-Newton shooting on B independent problems as ONE library call: the iterate is
        clamped and costed, then iters x (k_rollout_linearize, k_gn_direction, k_gn_candidates, K1 over B * line_steps
        candidates, k_gn_select).  -> dict(u_last (B,H,m) in bounds, cost (B) its cost, costs (iters,B) the cost at the
        start of every iteration or None, mu (B) float64, accepts (B) int32, alpha_hist (iters,B) the accepted step
        lengths, 0 where rejected, or None), same results bit for bit as solver.gn_solve.  The cost of a problem never
        rises.  x_ref, ref_offset, expanded_ref: as in solve_mppi, with line_steps rollouts per problem.  The workspace
        (a dict reused across calls) keeps the device buffer of phnn_gn_workspace_bytes.  box: phnn_solve_gn_ex with
        PHNN_GN_BOX -- the direction is k_gn_direction_box -- and the dict gains nclamp_hist (iters,B) int32.
        terminal: a terminal.TerminalCost (or its W): phnn_solve_gn_term -- k_terminal_cost behind the set-up K1 and the
        candidates' K1, the direction started from the terminal weight; every cost is a total cost.  None: the calls and
        bits of before."""
        x0 = self._t(x0, (-1, self.n))
        B = x0.shape[0]
        u_init, H = self._controls(u_init, B)
        integ = self._integ(integrator)
        opt = self._gn_options(iters, line_steps, mu_init, mu_min, mu_max, mu_up, mu_down)
        ws = {} if workspace is None else workspace
        key = (B, H, opt.line_steps)
        if ws.get("gn_key") != key:
            ws["gn_key"] = key
            ws["gn"] = torch.empty(max(self.gn_workspace_bytes(B, H, opt.line_steps), 256), dtype=torch.uint8, device=self.device)
        f = dict(dtype=torch.float32, device=self.device)
        u = u_init.detach().clone().contiguous()
        rows = max(opt.iters, 0)
        costs = torch.empty(rows, B, **f) if record_costs else None
        alpha = torch.empty(rows, B, **f) if record_costs else None
        cost_b = torch.empty(B, **f)
        mu = torch.empty(B, dtype=torch.float64, device=self.device)
        accepts = torch.empty(B, dtype=torch.int32, device=self.device)
        ref, _keep = self._reference(x_ref if expanded_ref else self.mppi_reference(x_ref, B, opt.line_steps), ref_offset,
                                     B * max(opt.line_steps, 1))
        head = (self.h, self._p(x0), self._p(u), B, H, C.byref(cost), None if ref is None else C.byref(ref), integ, float(dt),
                C.byref(opt), self._p(ws["gn"]), ws["gn"].numel(), self._p(cost_b), self._p(costs), self._p(mu),
                self._p(accepts), self._p(alpha))
        out = {"u_last": u, "cost": cost_b, "costs": costs, "mu": mu, "accepts": accepts, "alpha_hist": alpha}
        term, _keep_t = self._terminal(terminal, B)
        if term is not None:
            if box:
                out["nclamp_hist"] = torch.empty(rows, B, dtype=torch.int32, device=self.device)
            rc = self.lib.phnn_solve_gn_term(*head[:7], C.byref(term), *head[7:], _capi.PHNN_GN_BOX if box else 0,
                                             self._p(out.get("nclamp_hist")), self._stream())
        elif box:
            out["nclamp_hist"] = torch.empty(rows, B, dtype=torch.int32, device=self.device)
            rc = self.lib.phnn_solve_gn_ex(*head, _capi.PHNN_GN_BOX, self._p(out["nclamp_hist"]), self._stream())
        else:
            rc = self.lib.phnn_solve_gn(*head, self._stream())
        _check(self.lib, self.h, rc)
        return out

    # ------------------------------------------------------------------ what the three filters share
    def _filter_log(self, struct_cls, log):
        """log: None or dict(log_xhat (T+1,B,n) float32, log_dhat (T+1,B,m) float32 -- a _capi.DekfLog's only --, log_nis
        (T,B) float64, step_dev int32 tensor or step int) -> a struct_cls (_capi.EkfLog / _capi.DekfLog) or None."""
        if log is None:
            return None
        lg = struct_cls()
        for key, field in (("log_xhat", "log_xhat_dev"), ("log_dhat", "log_dhat_dev"), ("log_nis", "log_nis_dev"),
                           ("step_dev", "step_dev")):
            if log.get(key) is not None and hasattr(lg, field):
                setattr(lg, field, log[key].data_ptr())
        lg.step_host = int(log.get("step", -1))
        return lg

    def _ekf_outputs(self, B, nis, innov, status):
        d = dict(dtype=torch.float64, device=self.device)
        nis = torch.empty(B, **d) if nis is True else (None if nis is False else nis)
        innov = torch.empty(B, self.n, **d) if innov is True else (None if innov is False else innov)
        status = torch.empty(B, dtype=torch.int32, device=self.device) if status is None else status
        return nis, innov, status

    def _filter_update(self, symbol, log_cls, xpred, jac, y, P, nz, extra, opt, xhat, nis, innov, status, log, xpred_stride,
                       y_stride):
        """The body of ekf_update and dekf_update.  jac: the Jacobians the library takes after xpred, (A,) or (A, Bm); P
        (B,nz,nz) float64; extra: the float32 state it takes after xhat, () or (dhat,).  -> (xhat, nis, innov, status)."""
        self._assert_device_f32(xpred, *jac, y, *extra)
        assert P.dtype == torch.float64 and P.is_contiguous() and P.device == self.device
        B = P.shape[0]
        assert P.numel() == B * nz * nz and jac[0].numel() == B * self.n * self.n
        if xhat is None:
            xhat = torch.empty(B, self.n, dtype=torch.float32, device=self.device)
        self._assert_device_f32(xhat)
        nis, innov, status = self._ekf_outputs(B, nis, innov, status)
        lg = self._filter_log(log_cls, log)
        rc = getattr(self.lib, symbol)(self.h, self._p(xpred), self.n if xpred_stride is None else int(xpred_stride),
                                       *map(self._p, jac), self._p(y), self.n if y_stride is None else int(y_stride), B,
                                       C.byref(opt), self._p(P), self._p(xhat), *map(self._p, extra), self._p(nis),
                                       self._p(innov), self._p(status), None if lg is None else C.byref(lg), self._stream())
        _check(self.lib, self.h, rc)
        return xhat, nis, innov, status

    def _filter_step(self, symbol, ws_name, ws_bytes, log_cls, state, u, u_stride, y, cost, integrator, dt, opt, nis, innov,
                     status, log, workspace, y_stride):
        """The body of ekf_step, dekf_step and ukf_step.  state: the filter's tensors by the names of the result, in the
        order the library takes them -- float32 (B,.) ones, then the float64 covariance; ws_name: the key of the device
        buffer of ws_bytes(B) bytes in the workspace dict.  -> dict(**state, nis, innov, status)."""
        *x, P = state.values()
        self._assert_device_f32(*x, u, y)
        assert P.dtype == torch.float64 and P.is_contiguous() and P.device == self.device
        B = x[0].shape[0]
        ws = {} if workspace is None else workspace
        if ws.get(ws_name + "_key") != B:
            ws[ws_name + "_key"] = B
            ws[ws_name] = torch.empty(max(ws_bytes(B), 256), dtype=torch.uint8, device=self.device)
        nis, innov, status = self._ekf_outputs(B, nis, innov, status)
        lg = self._filter_log(log_cls, log)
        rc = getattr(self.lib, symbol)(self.h, *map(self._p, x), self._p(P), self._p(u), int(u_stride), self._p(y),
                                       self.n if y_stride is None else int(y_stride), B,
                                       C.byref(cost) if cost is not None else None, self._integ(integrator), float(dt),
                                       C.byref(opt), self._p(nis), self._p(innov), self._p(status),
                                       None if lg is None else C.byref(lg), self._p(ws[ws_name]), self._stream())
        _check(self.lib, self.h, rc)
        return dict(state, nis=nis, innov=innov, status=status)

    # ------------------------------------------------------------------ extended Kalman filter
    def ekf_workspace_bytes(self, B):
        return int(self.lib.phnn_ekf_workspace_bytes(self.h, int(B)))

    def ekf_update(self, xpred, A, y, P, opt, xhat=None, nis=True, innov=True, status=None, log=None, xpred_stride=None,
                   y_stride=None):
        """k_ekf_update on its own: the covariance propagation through A and the measurement update of the components
        in opt (_capi.EkfOptions).  xpred: float32, problem b's prediction at xpred.view(-1)[b * xpred_stride + i] (default
        stride n: a (B,n) tensor); A (B,n,n) float32; y float32 with y_stride likewise (only measured components are
        read); P (B,n,n) float64, updated IN PLACE.  nis / innov: True = allocate, False = skip, or a float64 tensor (B) /
        (B,n) to write.  -> dict(xhat (B,n) float32, P, nis, innov, status (B) int32: 0 updated or nothing measured, 1
        dropped measurement, 2 failure with NaN outputs)."""
        xhat, nis, innov, status = self._filter_update("phnn_ekf_update", _capi.EkfLog, xpred, (A,), y, P, self.n, (), opt,
                                                       xhat, nis, innov, status, log, xpred_stride, y_stride)
        return dict(xhat=xhat, P=P, nis=nis, innov=innov, status=status)

    def ekf_step(self, xhat, P, u, u_stride, y, cost, integrator, dt, opt, nis=True, innov=False, status=None, log=None,
                 workspace=None, y_stride=None):
        """phnn_ekf_step: one filter step through the learned model as ONE library call -- k_ekf_controls, K1 with H = 1
        from xhat, the linearisation of that step, k_ekf_update -- IN PLACE on xhat (B,n) float32 and P (B,n,n) float64.
        u: float32, problem b's applied control at u.view(-1)[b * u_stride + k]; cost: its bounds clamp the control as
        K1 and the plant do (None: no clamp); y, opt, nis, innov, status, log: as in ekf_update.  workspace: a dict
        reused across calls (keeps the device buffer of ekf_workspace_bytes).  -> dict(xhat, P, nis, innov, status)."""
        return self._filter_step("phnn_ekf_step", "ekf", self.ekf_workspace_bytes, _capi.EkfLog, dict(xhat=xhat, P=P), u,
                                 u_stride, y, cost, integrator, dt, opt, nis, innov, status, log, workspace, y_stride)

    # ------------------------------------------------------------------ tracking the plan between solves
    def feedback_workspace_bytes(self, B, H):
        return int(self.lib.phnn_feedback_workspace_bytes(self.h, int(B), int(H)))

    def feedback_plan(self, x0, u, cost, integrator="euler", dt=0.02, mu=0.0, workspace=None, traj=None, K=None, status=None):
        """phnn_feedback_plan: the nominal trajectory and the TV-LQR gains of a plan as ONE library call -- K1 from x0 with
        trajectories, the linearisation of that rollout, the LQ backward pass.  x0 (B,n), u (B,H,m) float32 on the
        engine's device, read in place; cost: the controller's (Q, R, bounds).  workspace: a dict reused across calls
        (keeps the device buffer of feedback_workspace_bytes and, unless given, the outputs).  -> dict(traj (B,H+1,n)
        float32, K (B,H,m,n) float64, status (B) int32: phnn_tvlqr's).  The backward pass starts from the stage cost
        (P_H = Q + Q^T) also when the solve that made the plan had a terminal weight: the gains track the plan, they
        do not re-optimise it."""
        self._assert_device_f32(x0, u)
        B, H = u.shape[0], u.shape[1]  # u is (B,H,m)
        ws = {} if workspace is None else workspace
        if ws.get("fb_key") != (B, H):
            ws["fb_key"] = (B, H)
            ws["fb"] = torch.empty(max(self.feedback_workspace_bytes(B, H), 256), dtype=torch.uint8, device=self.device)
            ws["fb_traj"] = torch.empty(B, H + 1, self.n, dtype=torch.float32, device=self.device)
            ws["fb_K"] = torch.empty(B, H, self.m, self.n, dtype=torch.float64, device=self.device)
            ws["fb_status"] = torch.empty(B, dtype=torch.int32, device=self.device)
        traj = ws["fb_traj"] if traj is None else traj
        K = ws["fb_K"] if K is None else K
        status = ws["fb_status"] if status is None else status
        assert traj.dtype == torch.float32 and K.dtype == torch.float64 and status.dtype == torch.int32
        opt = _capi.TvlqrOptions()
        opt.mu = float(mu)
        rc = self.lib.phnn_feedback_plan(self.h, self._p(x0), self._p(u), B, H, C.byref(cost), self._integ(integrator), float(dt),
                                         C.byref(opt), self._p(ws["fb"]), ws["fb"].numel(), self._p(traj), self._p(K),
                                         self._p(status), self._stream())
        _check(self.lib, self.h, rc)
        return dict(traj=traj, K=K, status=status)

    def feedback_control(self, x, u, traj, K, cost, solve_every, step=0, step_dev=None, u_out=None, status=True, dev=True,
                         log_status=None, log_dev=None):
        """phnn_feedback_control: u_out = clamp(clamp(u[:, j]) + K[:, j] (x - traj[:, j])) with j = step % solve_every,
        one launch.  x (B,n), u (B,H,m), traj (B,H+1,n) float32, K (B,H,m,n) float64 on the engine's device; cost: its
        bounds only (None: no clamp); step: an int, or step_dev an int32 device tensor (a captured launch follows it).
        status / dev: True = allocate, False = skip, or an int32 (B) / float64 (B) tensor to write; log_status (T,B) int32
        and log_dev (T,B) float64 receive row `step`.  -> dict(u (B,m) float32, status: 0 feedback, 1 gains not finite, 2
        deviation not finite (1, 2: the plan's control), dev: max |x - traj[:, j]| or NaN for status 2)."""
        self._assert_device_f32(x, u, traj)
        assert K.dtype == torch.float64 and K.is_contiguous() and K.device == self.device
        B, H = K.shape[0], K.shape[1]
        if u_out is None:
            u_out = torch.empty(B, self.m, dtype=torch.float32, device=self.device)
        self._assert_device_f32(u_out)
        status = torch.empty(B, dtype=torch.int32, device=self.device) if status is True else (None if status is False else status)
        dev = torch.empty(B, dtype=torch.float64, device=self.device) if dev is True else (None if dev is False else dev)
        rc = self.lib.phnn_feedback_control(self.h, self._p(x), self._p(u), self._p(traj), self._p(K), B, H,
                                            C.byref(cost) if cost is not None else None, int(solve_every), self._p(step_dev),
                                            -1 if step_dev is not None else int(step), self._p(u_out), self._p(status),
                                            self._p(dev), self._p(log_status), self._p(log_dev), self._stream())
        _check(self.lib, self.h, rc)
        return dict(u=u_out, status=status, dev=dev)

    # ------------------------------------------------------------------ disturbance-augmented filter
    def dekf_workspace_bytes(self, B):
        return int(self.lib.phnn_dekf_workspace_bytes(self.h, int(B)))

    def dekf_update(self, xpred, A, Bm, y, Pz, dhat, opt, xhat=None, nis=True, innov=True, status=None, log=None,
                    xpred_stride=None, y_stride=None):
        """k_dekf_update on its own: ekf_update on the augmented state z = (x, d) with the Jacobian [[A, Bm], [0, I]] and
        the options of _capi.DekfOptions.  xpred, y, strides, nis, innov, status: as in ekf_update; A (B,n,n) and Bm
        (B,n,m) float32; Pz (B,n+m,n+m) float64 and dhat (B,m) float32 are updated IN PLACE.  -> dict(xhat (B,n) float32,
        dhat, P (= Pz), nis, innov (B,n), status (B) int32)."""
        B = Pz.shape[0]
        assert Bm.numel() == B * self.n * self.m and dhat.numel() == B * self.m
        xhat, nis, innov, status = self._filter_update("phnn_dekf_update", _capi.DekfLog, xpred, (A, Bm), y, Pz,
                                                       self.n + self.m, (dhat,), opt, xhat, nis, innov, status, log,
                                                       xpred_stride, y_stride)
        return dict(xhat=xhat, dhat=dhat, P=Pz, nis=nis, innov=innov, status=status)

    def dekf_step(self, xhat, dhat, Pz, u, u_stride, y, cost, integrator, dt, opt, nis=True, innov=False, status=None, log=None,
                  workspace=None, y_stride=None):
        """phnn_dekf_step: one step of the disturbance-augmented filter as ONE library call -- k_dekf_controls (the row
        c(u) + dhat), K1 with H = 1 from xhat without bounds, the linearisation of that step without bounds,
        k_dekf_update -- IN PLACE on xhat (B,n) float32, dhat (B,m) float32 and Pz (B,n+m,n+m) float64.  u: float32,
        problem b's applied command at u.view(-1)[b * u_stride + k]; cost: its bounds clamp the command (None: no clamp);
        the rest as in ekf_step.  -> dict(xhat, dhat, P, nis, innov, status)."""
        return self._filter_step("phnn_dekf_step", "dekf", self.dekf_workspace_bytes, _capi.DekfLog,
                                 dict(xhat=xhat, dhat=dhat, P=Pz), u, u_stride, y, cost, integrator, dt, opt, nis, innov, status,
                                 log, workspace, y_stride)

    def dist_compensate(self, v, v_stride, dhat, cost, u_cmd=None, status=None):
        """phnn_dist_compensate: u_cmd (B,m) = c(c(v) - dhat), c the clamp to the cost's bounds (None: none); v: float32,
        problem b's command at v.view(-1)[b * v_stride + k]; dhat (B,m) float32.  A component whose dhat is not finite
        keeps c(v), and status (B) int32 (True = allocate, None = skip, or a tensor) is 1 for that problem.
        -> (u_cmd, status)."""
        self._assert_device_f32(v, dhat, u_cmd)
        B = dhat.numel() // self.m
        if u_cmd is None:
            u_cmd = torch.empty(B, self.m, dtype=torch.float32, device=self.device)
        if status is True:
            status = torch.empty(B, dtype=torch.int32, device=self.device)
        rc = self.lib.phnn_dist_compensate(self.h, self._p(v), int(v_stride), self._p(dhat), B,
                                           C.byref(cost) if cost is not None else None, self._p(u_cmd), self._p(status),
                                           self._stream())
        _check(self.lib, self.h, rc)
        return u_cmd, status

    # ------------------------------------------------------------------ unscented Kalman filter
    def ukf_workspace_bytes(self, B):
        return int(self.lib.phnn_ukf_workspace_bytes(self.h, int(B)))

    def ukf_sigma(self, xhat, P, opt, u=None, u_stride=None, chi=None, ctrl=None):
        """k_ukf_sigma on its own: the S = 2 n + 1 sigma points of (xhat (B,n) float32, P (B,n,n) float64, lower triangle
        read) with the spread opt.gamma (_capi.UkfOptions) -> (chi (B,S,n) float32, ctrl).  With u (float32, problem b's
        control at u.view(-1)[b * u_stride + k], default stride m) the control rows ctrl (B,S,1,m) are written too, else
        ctrl is None.  A problem whose P is not positive definite or whose xhat is not finite has NaN sigma points."""
        self._assert_device_f32(xhat, u, chi, ctrl)
        assert P.dtype == torch.float64 and P.is_contiguous() and P.device == self.device
        B, S = xhat.shape[0], 2 * self.n + 1
        assert xhat.numel() == B * self.n and P.numel() == B * self.n * self.n
        if chi is None:
            chi = torch.empty(B, S, self.n, dtype=torch.float32, device=self.device)
        if ctrl is None and u is not None:
            ctrl = torch.empty(B, S, 1, self.m, dtype=torch.float32, device=self.device)
        assert chi.numel() == B * S * self.n and (ctrl is None or ctrl.numel() == B * S * self.m)
        rc = self.lib.phnn_ukf_sigma(self.h, self._p(xhat), self._p(P), self._p(u), self.m if u_stride is None else int(u_stride),
                                     B, C.byref(opt), self._p(chi), self._p(ctrl), self._stream())
        _check(self.lib, self.h, rc)
        return chi, ctrl

    def ukf_moments(self, Y, B, opt, Y_stride=None, xm=None, Pm=None, eye=True):
        """k_ukf_moments on its own: the weighted mean and covariance of the images of B problems' sigma points with the
        weights opt.wm0, opt.wc0, opt.wi.  Y: float32, image k of problem b at Y.view(-1)[(b * S + k) * Y_stride + i]
        (default stride n: a (B,S,n) tensor).  eye: True = allocate, False = skip, or a (B,n,n) float32 tensor.
        -> dict(xm (B,n) float32, Pm (B,n,n) float64, eye (B,n,n) float32 identity or None)."""
        self._assert_device_f32(Y, xm)
        n = self.n
        if xm is None:
            xm = torch.empty(B, n, dtype=torch.float32, device=self.device)
        if Pm is None:
            Pm = torch.empty(B, n, n, dtype=torch.float64, device=self.device)
        eye = torch.empty(B, n, n, dtype=torch.float32, device=self.device) if eye is True else (None if eye is False else eye)
        self._assert_device_f32(eye)
        assert Pm.dtype == torch.float64 and Pm.is_contiguous() and Pm.device == self.device
        assert xm.numel() == B * n and Pm.numel() == B * n * n and (eye is None or eye.numel() == B * n * n)
        rc = self.lib.phnn_ukf_moments(self.h, self._p(Y), n if Y_stride is None else int(Y_stride), int(B), C.byref(opt),
                                       self._p(xm), self._p(Pm), self._p(eye), self._stream())
        _check(self.lib, self.h, rc)
        return dict(xm=xm, Pm=Pm, eye=eye)

    def ukf_step(self, xhat, P, u, u_stride, y, cost, integrator, dt, opt, nis=True, innov=False, status=None, log=None,
                 workspace=None, y_stride=None):
        """phnn_ukf_step: one step of the unscented filter as ONE library call -- k_ukf_sigma, K1 with H = 1 on the
        B * (2 n + 1) sigma points, k_ukf_moments, k_ekf_update with the identity -- IN PLACE on xhat (B,n) float32 and P
        (B,n,n) float64.  The arguments are ekf_step's, opt a _capi.UkfOptions.  -> dict(xhat, P, nis, innov, status)."""
        return self._filter_step("phnn_ukf_step", "ukf", self.ukf_workspace_bytes, _capi.EkfLog, dict(xhat=xhat, P=P), u,
                                 u_stride, y, cost, integrator, dt, opt, nis, innov, status, log, workspace, y_stride)

    # ------------------------------------------------------------------ the plant, on the device
    def plant_step(self, plant, state, action, action_stride, u_min=None, u_max=None, state_f32=None, done_step=None,
                   step=0, step_dev=None, log_states=None, log_controls=None, ex=None, metrics=None):
        """One float64 Euler step of the reference cart-pole for B plants, in place on `state` (B,4) float64.
        action: float32 tensor, plant b takes action.view(-1)[b * action_stride].  See include/phnn_mpc.h.
        ex (_capi.PlantEx) / metrics (_capi.PlantMetrics): phnn_plant_step_ex -- per-plant parameters, disturbances,
        freeze at termination, running metrics; the structs hold device pointers, the caller keeps the tensors alive."""
        assert state.dtype == torch.float64 and state.is_contiguous() and state.device == self.device
        assert action.dtype == torch.float32 and action.is_contiguous() and action.device == self.device
        B = state.shape[0]
        has_b = u_min is not None and u_max is not None
        rest = (self._p(state), self._p(action), int(action_stride), B, int(has_b), float(u_min) if has_b else 0.0,
                float(u_max) if has_b else 0.0, self._p(state_f32), self._p(done_step), self._p(step_dev), int(step),
                self._p(log_states), self._p(log_controls), self._stream())
        if ex is None and metrics is None:
            rc = self.lib.phnn_plant_step(self.h, C.byref(plant), *rest)
        else:
            rc = self.lib.phnn_plant_step_ex(self.h, C.byref(plant), C.byref(ex) if ex is not None else None,
                                             C.byref(metrics) if metrics is not None else None, *rest)
        _check(self.lib, self.h, rc)

    def shift_controls(self, src, dst, step_dev=None):
        """dst[b,t] = src[b,t+1], dst[b,H-1] = 0 (warm start of the next solve); advances *step_dev if given."""
        B, H, m = src.shape
        rc = self.lib.phnn_shift_controls(self.h, self._p(src), self._p(dst), B, H, m, self._p(step_dev), self._stream())
        _check(self.lib, self.h, rc)

    def advance_step(self, step_dev):
        rc = self.lib.phnn_shift_controls(self.h, None, None, 0, 1, 1, self._p(step_dev), self._stream())
        _check(self.lib, self.h, rc)

    @property
    def variant(self):
        """e.g. 'phnn<n=4,hid=128,fixedG,f16x2>'"""
        return self.lib.phnn_variant_name(self.h).decode()

    @property
    def matmul_mode(self):
        v = self.variant
        return "f16x2" if "f16x2" in v else ("bf16x3" if "bf16x3" in v else "f32")

    def kernel_info(self, B, integrator="euler"):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.lib.phnn_kernel_info(self.h, self._integ(integrator), C.byref(a), C.byref(b), C.byref(c), int(B))
        return {"rollouts_per_workgroup": a.value, "lds_bytes": b.value, "workgroups": c.value}


def as_numpy(t):
    return t.detach().cpu().numpy().astype(np.float64)
