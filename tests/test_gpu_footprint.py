"""The write footprint of every entry point, with guarded buffers (tests/footprint.py): each call gets pointers into
one arena in which every input, output and workspace has 64 KiB of guard on both sides, and workspaces of EXACTLY the
size the library reports.

Properties, asserted for every case and measured and reported before the test asserts:
  F1  guards: after the call and a synchronise no guard byte has changed, around inputs, outputs and workspaces alike,
      and no input byte either.
  F2  dirty = clean: outputs and documented in-place states are bit-identical whether outputs, workspaces and guards
      were filled with 0xFF (NaN to every float view) or with 0x00 before the call.  The accumulating entries are
      initialised by the test, because their contents on entry are data: grad_theta with accumulate = 1; best_cost /
      best_u of phnn_adam_step, phnn_mppi_update and phnn_cem_update (strict '<' against the value on entry); done_step
      (set once, from -1); the logs of phnn_plant_step (one row per call, the other rows must stay).
  F3  = the ordinary call: bit-identical to the same operation through the RolloutEngine method on fresh tensors (which
      other tests anchor to the float64 oracle).
  F4  read fence: with the guards around the INPUTS filled 0xFF instead of 0x00, outputs are bit-identical: a read past
      an input that reaches a result turns it into NaN.  What this cannot see: a stray read whose value is discarded
      (a load for an invalid lane that is masked afterwards, a prefetch), or one that lands in the input's own interior.
  F5  sizes: every *_workspace_bytes is positive for valid arguments, 0 for invalid ones and non-decreasing in B, H,
      samples and history; the calls succeed with exactly that many bytes (F1); the regions the Python side carves
      (_mppi_buffers, _cem_buffers, the record view of mass_cotangents) and the tape offset lie inside the reported
      size, do not overlap and are where the library writes -- located through their known contents.
  F6  row-sliced views: every tensor argument placed at the offset a row slice t[1:] gives (8 / 12 bytes for n = 2 / 3
      states, 4 H m for controls: 52 at H m = 13) yields the bits of the 256-byte aligned placement.

Cases: the smallest shapes at which each store path differs -- B in {1, 17, 37} (a partial tile, a full tile plus one,
two full tiles plus a ragged tile of 5), H in {1, 6}, Euler and RK4, stash given and NULL, optional outputs given and
NULL, split-tile and whole-tile kernels; the solves at B in {1, 19} and (H, m) in {(4, 1), (13, 1), (5, 2), (5, 3)}
(every N mod 4), K = 6, E = 2, 2 iterations.
"""
import ctypes as C
import time

import numpy as np
import pytest

import footprint as fp
import variant_census as vc

pytestmark = pytest.mark.gpu

# one census spec per store path
SPECS = {
    "phnn<n=4,hid=128,fixedG,f16x2>": "whole-tile and split-tile, wgrad",
    "phnn<n=2,hid=64,Gnet>": "element state stores, wgrad",
    "canonical<m=3,hid=128,f16x2>": "m > 1 control and gradient rows, wgrad",
    "odefunc<n=3,hid=128,f16x2>": "24-bit tape, n = 3",
    "odefunc<n=4,hid=128,relu>": "float32 z-tape",
}
ENGINES = [(sid, split) for sid in SPECS for split in (("never", "always") if vc.CENSUS[sid]["split"] else ("auto",))]
BATCHES, HORIZONS = (1, 17, 37), (1, 6)
# m -> the model the solves run on
SOLVE_MODEL = {1: "phnn<n=4,hid=128,fixedG,f16x2>", 2: "phnn<n=4,m=2,hid=128,fixedG,f16x2>", 3: "canonical<m=3,hid=128,f16x2>"}
SOLVE_SHAPES = [(4, 1), (13, 1), (5, 2), (5, 3)]
SOLVE_BATCHES = (1, 19)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


_engines = {}


def engine(sid, split="auto"):
    if (sid, split) not in _engines:
        from phnn_mpc_amd.engine import RolloutEngine
        s = vc.CENSUS[sid]
        eng = RolloutEngine(vc.build_state_dict(sid, s), "cuda:0", split=split, **vc.engine_kwargs(s))
        assert eng.variant == sid
        _engines[(sid, split)] = eng
    return _engines[(sid, split)]


def rng_of(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


class Report:
    """Collects the properties of every case of one test; prints a summary, then asserts."""

    def __init__(self, what):
        self.what, self.n, self.bad, self.t0 = what, {}, [], time.perf_counter()

    def note(self, prop, ok, msg):
        self.n[prop] = self.n.get(prop, 0) + 1
        if not ok:
            self.bad.append(f"{prop} {msg}")

    def finish(self):
        print(f"\n{self.what}: " + ", ".join(f"{k} x{v}" for k, v in sorted(self.n.items())) +
              f"; {len(self.bad)} failed; {time.perf_counter() - self.t0:.2f} s")
        for b in self.bad[:40]:
            print("   ", b)
        assert not self.bad, (self.what, self.bad[:40])


def _diff(torch, a, b, dtype):
    """First differing element of two byte tensors, for the message."""
    k = int((a != b).to(torch.uint8).argmax()) if a.numel() == b.numel() and a.numel() else -1
    return f"first differing byte {k} of {a.numel()}"


def footprint(rep, torch, eng, op, f3=True):
    """F1, F2, F3, F4, F6 of one operation.  `op` may be None: its constructor found a size of 0 (see make()).
    F3 -- the only execution on buffers without guards, which the engine sizes by the library's own size functions -- runs
    only when the guarded executions were clean: a defect they have shown must not run again where it can reach
    somebody else's memory.  It is then recorded as failed, not as skipped."""
    if op is None:
        return None
    bad0 = len(rep.bad)
    ff = fp.run(torch, eng, op, 0xFF)
    zero = fp.run(torch, eng, op, 0x00)
    fence = fp.run(torch, eng, op, 0x00, input_guard_byte=0xFF)
    skew = fp.run(torch, eng, op, 0xFF, skew=True)
    for tag, (hits, _o, _a) in (("0xFF", ff), ("0x00", zero), ("fence", fence), ("skew", skew)):
        rep.note("F1", not hits, f"{op.name} [{tag}]: guard or input changed: {hits}")
    for b in op.outputs():
        k = b.name
        rep.note("F2", fp.same_bytes(torch, ff[1][k], zero[1][k]),
                 f"{op.name} {k}: 0xFF fill against 0x00 fill, {_diff(torch, ff[1][k], zero[1][k], b.dtype)}")
        rep.note("F4", fp.same_bytes(torch, fence[1][k], zero[1][k]),
                 f"{op.name} {k}: input guards 0xFF against 0x00, {_diff(torch, fence[1][k], zero[1][k], b.dtype)}")
        rep.note("F6", fp.same_bytes(torch, skew[1][k], ff[1][k]),
                 f"{op.name} {k}: row-slice placement against aligned, {_diff(torch, skew[1][k], ff[1][k], b.dtype)}")
    if f3 and len(rep.bad) > bad0:
        rep.note("F3", False, f"{op.name}: not run, the guarded executions above failed")
    elif f3:
        ref = op.engine(eng)
        torch.cuda.synchronize()
        for k, t in ref.items():
            got = ff[1][k]
            rep.note("F3", fp.same_bytes(torch, got, fp.as_bytes(torch, t)),
                     f"{op.name} {k}: arena against the RolloutEngine call, {_diff(torch, got, fp.as_bytes(torch, t), None)}")
    return ff


def make(rep, ctor, *a, **k):
    """An Op, or None (and a failed F5) when its constructor finds a workspace size of 0 for valid arguments."""
    try:
        return ctor(*a, **k)
    except AssertionError as e:
        rep.note("F5", False, f"{ctor.__name__}{a[-4:]}: a workspace size of 0 for valid arguments ({e})")
        return None


def _ids(pairs):
    return [f"{sid}-{split}" for sid, split in pairs]


# =========================================================================================================== rollouts
@pytest.mark.parametrize("kind", ["grad", "ref", "vjp"])
@pytest.mark.parametrize("sid,split", ENGINES, ids=_ids(ENGINES))
def test_rollout_entries(torch, sid, split, kind):
    """phnn_rollout_fwd with phnn_rollout_grad ('grad'), their _ref twins ('ref') and phnn_rollout_vjp ('vjp') over
    B x H x integrator x stash x optional outputs.  F3 of the 'vjp' gradients is taken where the engine has the same
    call (it passes no stash to phnn_rollout_vjp)."""
    s, eng = vc.CENSUS[sid], engine(sid, split)
    rep = Report(f"rollout {kind} {sid} split={split}")
    for B in BATCHES:
        for H in HORIZONS:
            rng = rng_of("roll", sid, B, H)
            x0, U, cost = vc.states(rng, s["n"], B), vc.controls(rng, B, H, s["m"]), vc.cost_of(s, rng)
            for integ in (0, 1):
                for stash in (True, False):
                    for optional in (True, False):
                        footprint(rep, torch, eng, make(rep, fp.RollOp, eng, cost, x0, U, integ, vc.dt_of(s), kind, stash, optional, rng))
    rep.finish()


@pytest.mark.parametrize("sid,split", ENGINES, ids=_ids(ENGINES))
def test_point_entries(torch, sid, split):
    """phnn_model_forward (H given and NULL) and phnn_model_vjp."""
    s, eng = vc.CENSUS[sid], engine(sid, split)
    rep = Report(f"points {sid} split={split}")
    for B in BATCHES:
        rng = rng_of("point", sid, B)
        x, u = vc.states(rng, s["n"], B), rng.uniform(vc.U_MIN, vc.U_MAX, size=(B, s["m"])).astype(np.float32)
        lam = rng.normal(size=(B, s["n"])).astype(np.float32)
        for with_H in (True, False):
            footprint(rep, torch, eng, fp.PointOp(x, u, lam, with_H))
    rep.finish()


@pytest.mark.parametrize("mode", ["plain", "records", "tapes"])
@pytest.mark.parametrize("sid,split", ENGINES, ids=_ids(ENGINES))
def test_training_entries(torch, sid, split, mode):
    """phnn_rollout_trajectory ('plain': dx given and NULL), phnn_rollout_wgrad in records mode and, after
    phnn_rollout_trajectory_ws, in tapes mode, in a workspace of exactly phnn_wgrad_workspace_bytes; one case per shape
    also accumulates into a grad_theta the test initialised."""
    s, eng = vc.CENSUS[sid], engine(sid, split)
    if mode != "plain" and not s["wgrad"]:
        assert not eng.has_wgrad
        assert eng.lib.phnn_wgrad_workspace_bytes(eng.h, 37, 6, 0) == 0
        return
    rep = Report(f"training {mode} {sid} split={split}")
    for B in BATCHES:
        for H in HORIZONS:
            rng = rng_of("train", sid, B, H)
            x0, U = vc.states(rng, s["n"], B), vc.controls(rng, B, H, s["m"])
            for integ in (0, 1):
                for optional in (True, False):
                    footprint(rep, torch, eng, make(rep, fp.TrainOp, eng, x0, U, integ, vc.dt_of(s), rng, mode, optional))
                if mode != "plain":
                    footprint(rep, torch, eng, make(rep, fp.TrainOp, eng, x0, U, integ, vc.dt_of(s), rng, mode, True, accumulate=True))
    rep.finish()


@pytest.mark.parametrize("sid,split", [e for e in ENGINES if vc.CENSUS[e[0]]["wgrad"]],
                         ids=_ids([e for e in ENGINES if vc.CENSUS[e[0]]["wgrad"]]))
def test_model_wgrad(torch, sid, split):
    """phnn_model_wgrad: Hbar given and NULL, overwrite and accumulate."""
    s, eng = vc.CENSUS[sid], engine(sid, split)
    rep = Report(f"model_wgrad {sid} split={split}")
    for N in BATCHES:
        rng = rng_of("pw", sid, N)
        x, u = vc.states(rng, s["n"], N), rng.uniform(vc.U_MIN, vc.U_MAX, size=(N, s["m"])).astype(np.float32)
        lam, Hbar = rng.normal(size=(N, s["n"])).astype(np.float32), rng.normal(size=N).astype(np.float32)
        for hb in (Hbar, None):
            for acc in (False, True):
                footprint(rep, torch, eng, make(rep, fp.PointWgradOp, eng, x, u, lam, hb, rng, acc))
    rep.finish()


# =========================================================================================================== solves
def _solve_inputs(H, m, B):
    sid = SOLVE_MODEL[m]
    s = vc.CENSUS[sid]
    rng = rng_of("solve", H, m, B)
    return sid, s, rng, vc.states(rng, s["n"], B), vc.controls(rng, B, H, m), vc.cost_of(s, rng)


@pytest.mark.parametrize("H,m", SOLVE_SHAPES)
def test_adam_and_solve(torch, H, m):
    """phnn_adam_step (k_adam, k_best_cost) and phnn_solve with track_best, stash given and NULL, Euler and RK4."""
    rep = Report(f"adam H{H} m{m}")
    for B in SOLVE_BATCHES:
        sid, s, rng, x0, U, cost = _solve_inputs(H, m, B)
        eng = engine(sid)
        footprint(rep, torch, eng, fp.AdamOp(B, H, m, rng, vc.U_MIN, vc.U_MAX))
        for integ in (0, 1):
            for stash in (True, False):
                footprint(rep, torch, eng, make(rep, fp.SolveOp, eng, cost, x0, U, integ, vc.dt_of(s), stash))
    rep.finish()


@pytest.mark.parametrize("H,m", SOLVE_SHAPES)
def test_lbfgs(torch, H, m):
    """phnn_solve_lbfgs (history 3, max_iter 4): the Np = 4 ceil(N / 4) padded workspace rows next to the element access
    on the unpadded u and grad."""
    rep = Report(f"lbfgs H{H} m{m}")
    for B in SOLVE_BATCHES:
        sid, s, rng, x0, U, cost = _solve_inputs(H, m, B)
        footprint(rep, torch, engine(sid), make(rep, fp.LbfgsOp, engine(sid), cost, x0, U, 0, vc.dt_of(s)))
    rep.finish()


@pytest.mark.parametrize("which", ["mppi", "cem"])
@pytest.mark.parametrize("H,m", SOLVE_SHAPES)
def test_sampling(torch, H, m, which):
    """phnn_{mppi,cem}_sample (x0_rep given and NULL), _update and the whole solve in a workspace of exactly the
    reported size: the ALIGNED (N mod 4 = 0) and element forms of the row loads and stores."""
    rep = Report(f"{which} H{H} m{m}")
    for B in SOLVE_BATCHES:
        sid, s, rng, x0, U, cost = _solve_inputs(H, m, B)
        eng = engine(sid)
        for with_x0rep in (True, False):
            footprint(rep, torch, eng, fp.SampleOp(which, cost, x0, U, rng, with_x0rep))
        footprint(rep, torch, eng, fp.UpdateOp(which, cost, B, H, m, rng))
        footprint(rep, torch, eng, make(rep, fp.SampleSolveOp, which, eng, cost, x0, U, 0, vc.dt_of(s)))
    rep.finish()


# =========================================================================================================== loop kernels
def test_loop_kernels(torch):
    """phnn_plant_step with state_f32, done_step and both logs at B = 19, T = 3, steps 0 and T - 1 (the first and the last
    row of the (T + 1, B, 4) float64 log); phnn_shift_controls with a device counter."""
    eng = engine("phnn<n=4,hid=128,fixedG,f16x2>")
    rep = Report("loop kernels")
    for step in (0, 2):
        footprint(rep, torch, eng, fp.PlantOp(19, 3, step, rng_of("plant", step)))
    for B, H, m in ((19, 13, 1), (1, 1, 1), (19, 5, 3)):
        footprint(rep, torch, eng, fp.ShiftOp(B, H, m, rng_of("shift", B, H, m)))
    rep.finish()


@pytest.mark.parametrize("sid", list(SPECS))
def test_device_pack(torch, sid):
    """phnn_update_weights_dev from a blob in the arena, then phnn_read_image: the packed image equals the host-packed
    one (the exp / log1p constants of canonical models to the last bit or two, as the header says), and neither the
    blob nor its guards are written."""
    from phnn_mpc_amd.engine import RolloutEngine
    s = vc.CENSUS[sid]
    sd = vc.build_state_dict(sid, s)
    host = RolloutEngine(sd, "cuda:0", **vc.engine_kwargs(s))
    image = host.read_image()
    other = vc.build_state_dict(sid + "/other weights", s)  # same shapes, other values: something to overwrite
    dev = RolloutEngine(other, "cuda:0", **vc.engine_kwargs(s))
    assert not np.array_equal(dev.read_image(), image)
    rep = Report(f"pack {sid}")
    op = fp.PackOp(host.blob.astype(np.float32))
    for byte, skew in ((0xFF, False), (0x00, False), (0xFF, True)):
        hits, _o, _a = fp.run(torch, dev, op, byte, skew=skew)
        rep.note("F1", not hits, f"pack [{byte:#x} skew={skew}]: {hits}")
        got = dev.read_image()
        diff = np.flatnonzero(got.view(np.uint32) != image.view(np.uint32))
        if s["kind"] == "canonical":  # the bound of tests/test_gpu_device_pack.py: <= 11 libm-dependent constants, one ulp
            ok = diff.size <= 11 and np.allclose(got[diff], image[diff], rtol=2.5e-7, atol=0.0)
        else:
            ok = diff.size == 0
        rep.note("image", ok, f"device-packed image differs from the host-packed one in {diff.size} words")
        dev.update_weights(other)
    rep.finish()


# =========================================================================================================== F5
def test_sizes_positive_zero_monotone(torch):
    """The five size functions: positive for valid arguments, 0 for invalid ones, non-decreasing in each of B, H,
    samples and history."""
    rep = Report("sizes")
    for sid in SPECS:
        eng = engine(sid)
        lib, h = eng.lib, eng.h
        fns = {"stash": lambda B, H, x: lib.phnn_workspace_bytes(h, B, H, x),
               "lbfgs": lambda B, H, x: lib.phnn_lbfgs_workspace_bytes(h, B, H, x),
               "mppi": lambda B, H, x: lib.phnn_mppi_workspace_bytes(h, B, H, x),
               "cem": lambda B, H, x: lib.phnn_cem_workspace_bytes(h, B, H, x)}
        third = {"stash": (0, 1), "lbfgs": (1, 2, 3, 4, 5, 100), "mppi": (2, 3, 4, 6, 7, 64), "cem": (2, 3, 4, 6, 7, 64)}
        if vc.CENSUS[sid]["wgrad"]:
            fns["wgrad"] = lambda B, H, x: lib.phnn_wgrad_workspace_bytes(h, B, H, x)
            third["wgrad"] = (0, 1)
        else:
            rep.note("F5", lib.phnn_wgrad_workspace_bytes(h, 16, 1, 0) == 0, f"{sid}: wgrad size without wgrad kernels")
        Bs, Hs = list(range(1, 50)) + [255, 256, 257, 4096, 4097], list(range(1, 15)) + [50, 64]
        for name, fn in fns.items():
            monotone_in_x = name not in ("stash", "wgrad")  # their third argument is the integrator, not a size
            for x in third[name]:
                tab = np.array([[fn(B, H, x) for H in Hs] for B in Bs], dtype=np.int64)
                rep.note("F5", bool((tab > 0).all()), f"{sid} {name}: a size of 0 for valid arguments (x = {x})")
                rep.note("F5", bool((np.diff(tab, axis=0) >= 0).all()), f"{sid} {name}: decreasing in B (x = {x})")
                rep.note("F5", bool((np.diff(tab, axis=1) >= 0).all()), f"{sid} {name}: decreasing in H (x = {x})")
            if monotone_in_x:
                for B, H in ((1, 1), (19, 13), (37, 6)):
                    row = [fn(B, H, x) for x in third[name]]
                    rep.note("F5", all(a <= b for a, b in zip(row, row[1:])), f"{sid} {name}: decreasing in samples / history")
            bad_x = {"stash": 2, "wgrad": 2, "lbfgs": 0, "mppi": 1, "cem": 1}[name]
            ok_x = third[name][-1]
            invalid = [(0, 4, ok_x), (-1, 4, ok_x), (4, -1, ok_x), (4, 4, bad_x), (4, 4, -1)]
            if name != "wgrad":  # H = 0 is the point mode of the weight-gradient workspace
                invalid.append((4, 0, ok_x))
            for B, H, x in invalid:
                rep.note("F5", fn(B, H, x) == 0, f"{sid} {name}: nonzero size for invalid (B={B}, H={H}, x={x})")
        if "wgrad" in fns:
            rep.note("F5", fns["wgrad"](17, 0, 0) > 0 and fns["wgrad"](17, 0, 0) <= fns["wgrad"](17, 1, 0), f"{sid}: point-mode wgrad size")
    rep.finish()


def test_wgrad_size_of_a_negative_horizon_is_zero(torch):
    """Regression: phnn_wgrad_workspace_bytes took every H <= 0 for the point mode (H = 0) and reported the point-mode
    size for H = -1, -7, ...; the other size functions return 0 for a horizon that is no horizon."""
    for sid in SPECS:
        eng = engine(sid)
        if not vc.CENSUS[sid]["wgrad"]:
            continue
        point = eng.lib.phnn_wgrad_workspace_bytes(eng.h, 17, 0, 0)
        assert point > 0
        for H in (-1, -7, -2 ** 31):
            for integ in (0, 1):
                assert eng.lib.phnn_wgrad_workspace_bytes(eng.h, 17, H, integ) == 0, (sid, H, integ)


def _inside_disjoint(rep, what, buf, views):
    """The carved views lie inside `buf` and do not overlap."""
    lo, hi = buf.data_ptr(), buf.data_ptr() + buf.numel()
    spans = sorted((v.data_ptr(), v.data_ptr() + v.numel() * v.element_size(), k) for k, v in views.items())
    rep.note("F5", all(lo <= a and b <= hi for a, b, _ in spans), f"{what}: a carved region leaves the reported size")
    rep.note("F5", all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), f"{what}: carved regions overlap")
    return spans


@pytest.mark.parametrize("which", ["mppi", "cem"])
@pytest.mark.parametrize("H,m", SOLVE_SHAPES)
def test_carved_sampling_workspace(torch, H, m, which):
    """_mppi_buffers / _cem_buffers against where phnn_solve_mppi / phnn_solve_cem write: after a one-iteration solve
    in a 0xFF-filled workspace of the reported size, the Python views hold the sample tensor (= phnn_*_sample of the
    clamped initial nominal), the replicated x0, K1's costs of those samples and (CEM) the sigma the solve returns; every
    word of the views is written and no byte outside them is."""
    rep = Report(f"carve {which} H{H} m{m}")
    K = fp.K_SAMPLES
    for B in SOLVE_BATCHES:
        sid, s, rng, x0, U, cost = _solve_inputs(H, m, B)
        eng = engine(sid)
        op = fp.SampleSolveOp(which, eng, cost, x0, U, 0, vc.dt_of(s), iters=1)
        hits, outs, arena = fp.run(torch, eng, op, 0xFF)
        rep.note("F1", not hits, f"{op.name}: {hits}")
        if hits:  # the library writes outside what it reports: nothing more of this case runs on unguarded buffers
            continue
        ws = (eng._mppi_buffers if which == "mppi" else eng._cem_buffers)({}, B, H, K)
        buf = ws[which]
        rep.note("F5", buf.numel() == op.nws, f"{op.name}: the Python buffer has {buf.numel()} bytes, the library reports {op.nws}")
        buf.copy_(arena.interior("ws"))
        names = ["v", "x0", "s"] + (["sig"] if which == "cem" else [])
        views = {k: ws[f"{which}_{k}"] for k in names}
        spans = _inside_disjoint(rep, op.name, buf, views)
        Uc = np.clip(U, vc.U_MIN, vc.U_MAX)
        x0r = torch.tensor(x0, device="cuda").repeat_interleave(K, dim=0)
        if which == "mppi":
            v, _ = eng.mppi_sample(x0, Uc, cost, K, op.sigma, fp.SEED, 0, epoch=3, problem_offset=5)
        else:
            sig0 = torch.tensor(np.broadcast_to(np.asarray(op.sigma, np.float32), (B, H, m)).copy(), device="cuda")
            v, _ = eng.cem_sample(x0, Uc, sig0, cost, K, fp.SEED, 0, epoch=3, problem_offset=5)
        rep.note("F5", bool(torch.equal(views["v"], v)), f"{op.name}: the sample tensor is not where {which}_v looks")
        rep.note("F5", bool(torch.equal(views["x0"], x0r)), f"{op.name}: the replicated x0 is not where {which}_x0 looks")
        c = eng.rollout_cost(x0r, v, cost, "euler", vc.dt_of(s))
        rep.note("F5", fp.same_bytes(torch, fp.as_bytes(torch, views["s"]), fp.as_bytes(torch, c)),
                 f"{op.name}: K1's cost vector is not where {which}_s looks")
        if which == "cem":
            rep.note("F5", fp.same_bytes(torch, fp.as_bytes(torch, views["sig"]), outs["sigma_out"]),
                     f"{op.name}: the sigma state is not where cem_sig looks")
        mask = torch.ones(buf.numel(), dtype=torch.bool, device="cuda")
        for a, b, k in spans:
            mask[a - buf.data_ptr(): b - buf.data_ptr()] = False
            rep.note("F5", bool((views[k].reshape(-1).view(torch.int32) != -1).all()), f"{op.name}: {which}_{k} has unwritten words")
        rep.note("F5", bool((buf[mask] == 0xFF).all()), f"{op.name}: the library wrote outside the carved regions")
    rep.finish()


@pytest.mark.parametrize("sid", [k for k in SPECS if vc.CENSUS[k]["wgrad"]])
def test_wgrad_tape_offset(torch, sid):
    """phnn_rollout_trajectory_ws writes its tapes behind the records and the slab: in a 0xFF-filled workspace of exactly
    the reported size, the first byte it writes is the tape offset -- which is the point-mode size of as many records,
    records + slab rounded to 64 floats -- the record region stays untouched, and the last tape ends with the workspace."""
    s, eng = vc.CENSUS[sid], engine(sid)
    rep = Report(f"tape offset {sid}")
    rf = C.c_int32()
    assert eng.lib.phnn_wgrad_record_info(eng.h, C.byref(rf), None, None) == 0
    for B, H, integ in ((1, 1, 0), (17, 6, 0), (37, 6, 1), (37, 1, 1)):
        rng = rng_of("tape", sid, B, H)
        op = fp.TrainOp(eng, vc.states(rng, s["n"], B), vc.controls(rng, B, H, s["m"]), integ, vc.dt_of(s), rng, "tapes")
        arena = fp.Arena(torch, eng.device, op.regions(False))
        arena.fill(0xFF)
        for b in op.bufs:
            if b.init is not None:
                arena.load(b.name, torch.from_numpy(b.init))
        p = {b.name: arena.ptr(b.name) for b in op.bufs}
        fp.check_rc(eng, eng.lib.phnn_rollout_trajectory_ws(eng.h, p["x0"], p["u"], B, H, integ, float(vc.dt_of(s)), p["traj"], p["dX"],
                                                            p["wws"], eng._stream()))
        torch.cuda.synchronize()
        rep.note("F1", not arena.check(), f"{op.name}: {arena.check()}")
        n_rec = (B + 15) // 16 * H * (4 if integ else 1)
        total = arena.at["wws"][1]
        off = int(eng.lib.phnn_wgrad_workspace_bytes(eng.h, 16 * n_rec, 0, 0))
        first, last = arena.written("wws", 0xFF)
        slot = (total - off) // n_rec
        print(f"{op.name}: records {n_rec} x {rf.value} floats, tape offset {off}, size {total}, written [{first}, {last})")
        rep.note("F5", 4 * n_rec * rf.value <= off < total and (total - off) % n_rec == 0, f"{op.name}: records, offset {off} and size {total} do not nest")
        rep.note("F5", first == off, f"{op.name}: first tape byte at {first}, tape offset {off}")
        rep.note("F5", total - slot < last <= total, f"{op.name}: last tape byte at {last}, workspace ends at {total}")
    rep.finish()


def test_mass_cotangent_records(torch):
    """The record view of mass_cotangents against where phnn_model_wgrad writes: with the weight-gradient workspace an
    arena region of exactly the reported size, floats 24, 25 of every point's block are that point's q, the cotangents
    beyond the batch are zero, and both equal the ordinary call's bit for bit."""
    sid = "canonical<hid=128,f16x2,mass=full>"
    s, eng = vc.CENSUS[sid], engine(sid)
    rep = Report("mass cotangent records")
    for N in BATCHES:
        rng = rng_of("mass", N)
        x, u = vc.states(rng, 4, N), rng.uniform(vc.U_MIN, vc.U_MAX, size=(N, 1)).astype(np.float32)
        lam, Hbar = rng.normal(size=(N, 4)).astype(np.float32), rng.normal(size=N).astype(np.float32)
        op = fp.PointWgradOp(eng, x, u, lam, Hbar, rng)
        hits, _outs, arena = footprint(rep, torch, eng, op)
        eng.model_wgrad(x, u, lam, Hbar)
        q_ref, M_ref = (t.clone() for t in eng.mass_cotangents(N))
        keep = eng._wg_ws
        eng._wg_ws = arena.interior("wws")
        try:
            q, Mbar = (t.clone() for t in eng.mass_cotangents(N))
        finally:
            eng._wg_ws = keep
        P = 16 * ((N + 15) // 16)
        rep.note("F5", q.shape == (P, 2) and bool(torch.equal(q[:N], torch.tensor(x[:, :2], device="cuda"))),
                 f"N{N}: floats 24, 25 of the records are not the points' q")
        # lanes beyond the batch run on the last point with a zero cotangent: their Mbar is exactly zero
        rep.note("F5", bool((Mbar[N:] == 0).all()), f"N{N}: points beyond the batch carry a nonzero cotangent")
        rep.note("F5", bool(torch.equal(q, q_ref)) and bool(torch.equal(Mbar, M_ref)), f"N{N}: records differ from the ordinary call's")
    rep.finish()
