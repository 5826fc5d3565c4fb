"""What the MPPI and the CEM solve share on the device: the sample kernel and the host-side argument checks.

  sample   the two sigma sources of the sample kernel -- MPPI's per-component table in the kernel arguments, CEM's
           (B, N) tensor in memory -- give the same samples BIT FOR BIT when the tensor holds the table's value in every
           element: same counter, same normals, same clampf(u + sigma * z) with contraction off.  N = H*m covers every
           N mod 4, one and two float4 per row, m = 2 with a zero component, and bases 4 bytes past a 16-byte boundary.
  faults   one bad argument at a time, through all three entry points of both methods (sample, update, solve): the
           return code and a word of phnn_last_error.  None of these calls launches a kernel, except the two iters = 0
           solves that return 0 (they reset best and clamp u).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cem import bits, on_device
from test_gpu_mppi import engine, make_cost, nominal, npy, states

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a GPU"
    return t


# ----------------------------------------------------------------------------- 1. the two sigma sources agree as bits
B, K, LIM = 3, 17, 2.0
SAMPLE_CASES = [("phnn_cartpole", 5, (1.3,), False), ("phnn_cartpole", 6, (1.3,), False), ("phnn_cartpole", 7, (1.3,), False),
                ("phnn_cartpole", 8, (1.3,), False), ("phnn_m2_fix", 3, (1.3, 0.0), False), ("phnn_m2_fix", 4, (1.3, 0.0), False),
                ("phnn_cartpole", 8, (1.3,), True)]


@pytest.mark.parametrize("model, H, sigma, misalign", SAMPLE_CASES)
def test_table_sigma_and_tensor_sigma_give_the_same_bits(torch, model, H, sigma, misalign):
    eng = engine(model)
    m, N = eng.m, H * eng.m
    assert len(sigma) == m
    cost = make_cost(eng, u_lim=LIM)
    x0 = torch.tensor(states(B, 21), device="cuda")
    un = nominal(B, H, m, 22, lim=1.5)
    sig = np.broadcast_to(np.asarray(sigma, np.float32), (B, H, m))
    it, ep, off = 2, 5, 2 ** 33 + 1
    u = on_device(torch, un, misalign)
    va, xa = eng.mppi_sample(x0, u, cost, K, sigma, SEED, it, epoch=ep, problem_offset=off)
    vb, xb = eng.cem_sample(x0, u, on_device(torch, sig, misalign), cost, K, SEED, it, epoch=ep, problem_offset=off)
    assert va.data_ptr() != vb.data_ptr()
    va, vb = npy(va).reshape(B, K, N), npy(vb).reshape(B, K, N)
    assert np.array_equal(bits(va), bits(vb))
    assert np.array_equal(bits(npy(xa)), bits(npy(xb))) and np.array_equal(npy(xa), np.repeat(npy(x0), K, axis=0))
    # the comparison is not vacuous: noise was drawn, some of it clamped, and only where sigma is not 0
    assert np.array_equal(bits(va[:, 0]), bits(un.reshape(B, N)))
    noisy = va[:, 1:] != un.reshape(B, 1, N)
    comp = np.arange(N) % m
    assert noisy[:, :, np.asarray(sigma)[comp] != 0].mean() > 0.9 and not noisy[:, :, np.asarray(sigma)[comp] == 0].any()
    assert np.abs(va).max() == LIM and (np.abs(va) < LIM).any()


# ----------------------------------------------------------------------------- 2. one fault at a time, both methods
FB, FH, FK = 2, 3, 4
NAN, INF = float("nan"), float("inf")
# (what, changes, return code, word of phnn_last_error); changes: option fields, or H / iteration / null / short
SHARED = [("samples=1", dict(samples=1, elites=1), -1, "samples"), ("samples=2^26+1", dict(samples=2 ** 26 + 1), -1, "samples"),
          ("iters=-1", dict(iters=-1), -1, "iteration count"), ("iters=65537", dict(iters=65537), -1, "iteration count"),
          ("iteration=65536", dict(iteration=65536), -1, "iteration count"),
          ("offset=-1", dict(problem_offset=-1), -1, "problem ids"),
          ("offset=2^48-B+1", dict(problem_offset=2 ** 48 - FB + 1), -1, "problem ids"),
          ("H=0", dict(H=0), -1, "horizon"), ("H*m=257", dict(H=257), -2, "256"),
          ("no best_cost", dict(null="best_cost"), -1, "required"),
          ("no workspace", dict(null="workspace"), -1, "workspace"), ("short workspace", dict(short=1), -1, "workspace"),
          ("no workspace, iters=0", dict(null="workspace", iters=0), 0, ""),
          ("short workspace, iters=0", dict(short=1, iters=0), 0, ""),
          ("best_cost without best_u", dict(null="best_u"), -1, "go together")]
OWN = {"mppi": [("lambda=0", dict(lam=0.0), -1, "lambda"), ("lambda=inf", dict(lam=INF), -1, "lambda"),
                ("lambda=nan", dict(lam=NAN), -1, "lambda"), ("sigma=-1", dict(sigma=-1.0), -1, "sigma"),
                ("sigma=inf", dict(sigma=INF), -1, "sigma")],
       "cem": [("elites=0", dict(elites=0), -1, "elites"), ("elites=samples+1", dict(elites=FK + 1), -1, "elites"),
               ("alpha=1", dict(alpha=1.0), -1, "alpha"), ("alpha=-0.1", dict(alpha=-0.1), -1, "alpha"),
               ("alpha=nan", dict(alpha=NAN), -1, "alpha"), ("sigma_init=-1", dict(sigma=-1.0), -1, "sigma_init"),
               ("sigma_min=-1", dict(sigma_min=-1.0), -1, "sigma_min"), ("sigma_min=inf", dict(sigma_min=INF), -1, "sigma_min")]}
FAULTS = [(meth, *c) for meth in ("mppi", "cem") for c in SHARED + OWN[meth]]
# which entry points a change can reach: the rest go through all three
ONLY = {"iteration": ("sample",), "best_cost": ("solve",), "workspace": ("solve",), "short": ("solve",), "best_u": ("update",)}


@pytest.mark.parametrize("meth, what, chg, rc, word", FAULTS, ids=[f"{f[0]}-{f[1]}" for f in FAULTS])
def test_one_fault_at_a_time(torch, meth, what, chg, rc, word):
    eng = engine("phnn_cartpole")
    lib, h, p = eng.lib, eng.h, eng._p
    cost = make_cost(eng)
    chg = dict(chg)
    H, iteration, null, short = chg.pop("H", FH), chg.pop("iteration", 0), chg.pop("null", None), chg.pop("short", 0)
    o = dict(iters=1, samples=FK, lam=1.0, elites=2, alpha=0.25, sigma=1.0, sigma_min=0.05, seed=0, epoch=0, problem_offset=0)
    o.update(chg)
    if meth == "mppi":
        opt, _ = eng._mppi_options(o["iters"], o["samples"], o["lam"], o["sigma"], o["seed"], o["epoch"], o["problem_offset"])
    else:
        opt, _ = eng._cem_options(o["iters"], o["samples"], o["elites"], o["alpha"], o["sigma"], o["sigma_min"], o["seed"],
                                  o["epoch"], o["problem_offset"])
    f = dict(dtype=torch.float32, device="cuda")
    rows = max(H, 1) * eng.m  # every buffer is real and large enough for the call as it is made, refused or not
    x0, u, sig = torch.zeros(FB, eng.n, **f), torch.full((FB, rows), 20.0, **f), torch.ones(FB, rows, **f)
    v, x0r, s = torch.zeros(FB * FK, rows, **f), torch.zeros(FB * FK, eng.n, **f), torch.zeros(FB * FK, **f)
    best_cost, best_u = torch.zeros(FB, **f), torch.ones(FB, rows, **f)
    nbytes = {"mppi": eng.mppi_workspace_bytes, "cem": eng.cem_workspace_bytes}[meth](FB, FH, FK)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    wp, wn = (None, 0) if null == "workspace" else (p(ws), nbytes - short)
    bc, bu = None if null == "best_cost" else p(best_cost), None if null in ("best_cost", "best_u") else p(best_u)
    ob, cb, st = C.byref(opt), C.byref(cost), eng._stream()
    sg = () if meth == "mppi" else (p(sig),)
    calls = {"sample": lambda: getattr(lib, f"phnn_{meth}_sample")(h, p(x0), p(u), *sg, FB, H, cb, ob, iteration, p(v), p(x0r), st),
             "update": lambda: getattr(lib, f"phnn_{meth}_update")(h, p(u), *sg, p(v), p(s), FB, H, cb, ob, None, bc, bu, st),
             "solve": lambda: getattr(lib, f"phnn_solve_{meth}")(h, p(x0), p(u), FB, H, cb, None, 0, 0.02, ob, wp, wn, None, bc, bu,
                                                                *(() if meth == "mppi" else (None,)), st)}
    kinds = next((k for key, k in ONLY.items() if key in (null, "short" if short else None, "iteration" if iteration else None)),
                 ("sample", "update", "solve"))
    for kind in kinds:
        got = calls[kind]()
        msg = (lib.phnn_last_error(h) or b"").decode()
        assert got == rc, (kind, got, msg)
        if rc:
            assert word in msg and (meth in msg.lower() or word == "horizon"), (kind, msg)
    torch.cuda.synchronize()
    if rc == 0:  # iters = 0: no workspace needed, best reset and u clamped all the same
        assert bool(torch.isinf(best_cost).all()) and bool((best_u == 0).all()) and bool((u == 10.0).all())
    else:  # refused before anything was written
        assert bool((best_cost == 0).all()) and bool((best_u == 1).all()) and bool((u == 20.0).all())
