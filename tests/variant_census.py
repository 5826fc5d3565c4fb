"""Census of the kernel variants the library instantiates (csrc/phnn_variants.h PHNN_FOR_EACH_VARIANT, the split-tile
sets of csrc/phnn_split.hip, the weight-gradient sets PHNN_WCASE of csrc/phnn_wgrad.hip): one model spec per variant,
the RolloutEngine options that select it, which extra kernel sets it is expected to have, and a builder that turns a
spec into a reference-layout state_dict with seeded weights.  A helper module of tests/test_variant_census.py (CPU:
the census covers the source exactly, the float32 oracle leaves room under the tolerances) and
tests/test_gpu_variant_census.py (GPU: every variant against the float64 oracle).

Weights: MLP layers use PyTorch's default nn.Linear init, U(+-1/sqrt(fan_in)) for weights and biases, seeded from
zlib.crc32(spec id); the other parameters (J, G, R_diag_raw, mass-matrix parameters) come from the fixtures of the
same kind where one exists and are seeded random of the same shape otherwise.
"""
import os
import re
import zlib

import numpy as np

from phnn_mpc_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "phnn_mpc_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def spec(kind, n, width, m=1, fixed_G=True, mass="cartpole", act="tanh", matmul="default", force=False, split=False,
         wgrad=False, tol=1.0, widths=None, salt=0):
    """kind 'phnn' | 'canonical' | 'odefunc'.  width: the kernel's hidden width.  widths: the model's own hidden widths
    when narrower (zero-padded by the library): {'H': [..], 'R': [..], 'G': [..]} (pHNN), {'H': [..]} (canonical),
    {'net': [..]} (ODEFunc).  tol: factor on every stated tolerance of this variant (1.0 unless measured otherwise).
    salt: added to the seed where the first one drew an ill-conditioned case (a rollout whose gradient or a parameter
    tensor whose gradient nearly cancels, so that even the float32 oracle misses a fifth of the tolerance)."""
    if widths is None:
        widths = {"phnn": {"H": [width] * 2, "R": [width], "G": [width]},
                  "canonical": {"H": [width] * 2}, "odefunc": {"net": [width] * 3}}[kind]
    return dict(kind=kind, n=n, m=m, width=width, fixed_G=fixed_G, mass=mass, act=act, matmul=matmul, force=force,
                split=split, wgrad=wgrad, tol=tol, widths=widths, salt=salt)


def phnn(n, w, fixed, m=1, **kw):
    return spec("phnn", n, w, m=m, fixed_G=fixed, **kw)


def canon(w, m=1, **kw):
    return spec("canonical", 4, w, m=m, **kw)


def ode(n, w, **kw):
    return spec("odefunc", n, w, **kw)


# variant name (phnn_variant_name) -> spec that selects it
CENSUS = {
    "phnn<n=4,hid=128,fixedG>": phnn(4, 128, True, matmul="f32", wgrad=True),
    "phnn<n=4,hid=64,fixedG>": phnn(4, 64, True, wgrad=True),
    "phnn<n=2,hid=64,Gnet>": phnn(2, 64, False, wgrad=True),
    "phnn<n=2,hid=64,fixedG>": phnn(2, 64, True, wgrad=True),
    "canonical<hid=128>": canon(128, matmul="f32", wgrad=True),
    "canonical<hid=64>": canon(64, wgrad=True),
    "odefunc<n=2,hid=128>": ode(2, 128, matmul="f32"),
    "odefunc<n=2,hid=64>": ode(2, 64, salt=1),
    "odefunc<n=3,hid=128>": ode(3, 128, matmul="f32", salt=1),
    "phnn<n=4,hid=128,fixedG,bf16x3>": phnn(4, 128, True, matmul="bf16x3"),
    "canonical<hid=128,bf16x3>": canon(128, matmul="bf16x3"),
    "phnn<n=4,hid=128,fixedG,f16x2>": phnn(4, 128, True, split=True, wgrad=True),
    "canonical<hid=128,f16x2>": canon(128, split=True, wgrad=True),
    "odefunc<n=2,hid=128,f16x2>": ode(2, 128),
    "odefunc<n=3,hid=128,f16x2>": ode(3, 128),
    "odefunc<n=4,hid=128>": ode(4, 128, salt=2),
    "phnn<n=4,hid=128,Gnet,f16x2>": phnn(4, 128, False, wgrad=True),
    "phnn<n=2,hid=128,Gnet,f16x2>": phnn(2, 128, False, wgrad=True),
    "phnn<n=2,hid=128,fixedG,f16x2>": phnn(2, 128, True, split=True, wgrad=True),
    # f16x2 on the 64-wide models sits behind force_matmul
    "phnn<n=4,hid=64,fixedG,f16x2>": phnn(4, 64, True, matmul="f16x2", force=True),
    "phnn<n=2,hid=64,Gnet,f16x2>": phnn(2, 64, False, matmul="f16x2", force=True),
    "phnn<n=2,hid=64,fixedG,f16x2>": phnn(2, 64, True, matmul="f16x2", force=True),
    "canonical<hid=64,f16x2>": canon(64, matmul="f16x2", force=True),
    "odefunc<n=2,hid=64,f16x2>": ode(2, 64, matmul="f16x2", force=True, salt=1),
    "phnn<n=4,m=2,hid=128,fixedG,f16x2>": phnn(4, 128, True, m=2, wgrad=True),
    "phnn<n=4,m=2,hid=128,Gnet,f16x2>": phnn(4, 128, False, m=2, wgrad=True),
    "canonical<m=2,hid=128,f16x2>": canon(128, m=2, wgrad=True),
    "phnn<n=4,m=3,hid=128,fixedG,f16x2>": phnn(4, 128, True, m=3, wgrad=True),
    "phnn<n=4,m=3,hid=128,Gnet,f16x2>": phnn(4, 128, False, m=3, wgrad=True),
    "canonical<m=3,hid=128,f16x2>": canon(128, m=3, wgrad=True),
    "phnn<n=4,m=4,hid=128,fixedG,f16x2>": phnn(4, 128, True, m=4, wgrad=True),
    "phnn<n=4,m=4,hid=128,Gnet,f16x2>": phnn(4, 128, False, m=4, wgrad=True),
    "canonical<m=4,hid=128,f16x2>": canon(128, m=4, wgrad=True),
    "canonical<hid=128,f16x2,mass=constant>": canon(128, mass="constant", wgrad=True),
    "canonical<hid=128,f16x2,mass=diagonal>": canon(128, mass="diagonal", wgrad=True),
    "canonical<hid=128,f16x2,mass=full>": canon(128, mass="full", wgrad=True, salt=1),
    "phnn<n=4,hid=128,fixedG,silu>": phnn(4, 128, True, act="silu"),
    "phnn<n=4,hid=128,fixedG,relu>": phnn(4, 128, True, act="relu"),
    "canonical<hid=128,silu>": canon(128, act="silu"),
    "canonical<hid=128,relu>": canon(128, act="relu"),
    "odefunc<n=2,hid=128,relu>": ode(2, 128, act="relu"),
    "odefunc<n=4,hid=128,relu>": ode(4, 128, act="relu"),
    "phnn<n=4,hid=128,fixedG,elu>": phnn(4, 128, True, act="elu"),
    "phnn<n=4,hid=128,fixedG,gelu>": phnn(4, 128, True, act="gelu", salt=1),
    "canonical<hid=128,elu>": canon(128, act="elu"),
    "canonical<hid=128,gelu>": canon(128, act="gelu"),
    "odefunc<n=2,hid=128,elu>": ode(2, 128, act="elu"),
    "odefunc<n=2,hid=128,gelu>": ode(2, 128, act="gelu", salt=1),
    "odefunc<n=4,hid=128,elu>": ode(4, 128, act="elu", salt=1),
    "odefunc<n=4,hid=128,gelu>": ode(4, 128, act="gelu", salt=2),
}

# narrower models the library zero-pads to a variant's width (one per family; the weight-gradient ones go through
# the unpad map back to the model's own layout): spec id -> (variant that serves it, spec)
PADDED = {
    "phnn<n=4,fixedG>/H96,80,R48": ("phnn<n=4,hid=128,fixedG,f16x2>",
                                    phnn(4, 128, True, split=True, wgrad=True, widths={"H": [96, 80], "R": [48]}, salt=1)),
    "phnn<n=2,Gnet>/H48,40,R56,G36": ("phnn<n=2,hid=64,Gnet>",
                                      phnn(2, 64, False, wgrad=True, widths={"H": [48, 40], "R": [56], "G": [36]}, salt=1)),
    "phnn<n=4,m=3,Gnet>/H100,128,R64,G90": ("phnn<n=4,m=3,hid=128,Gnet,f16x2>",
                                            phnn(4, 128, False, m=3, wgrad=True,
                                                 widths={"H": [100, 128], "R": [64], "G": [90]})),
    "canonical/H40,56": ("canonical<hid=64>", canon(64, wgrad=True, widths={"H": [40, 56]})),
    "canonical/H96,72": ("canonical<hid=128,f16x2>", canon(128, split=True, wgrad=True, widths={"H": [96, 72]})),
    "odefunc<n=2>/96,128,72": ("odefunc<n=2,hid=128>", ode(2, 128, matmul="f32", widths={"net": [96, 128, 72]})),
    "odefunc<n=4,gelu>/120,100,128": ("odefunc<n=4,hid=128,gelu>", ode(4, 128, act="gelu", salt=1,
                                                                       widths={"net": [120, 100, 128]})),
}

# every spec the GPU test runs: spec id -> (variant, spec)
ALL_SPECS = dict({k: (k, v) for k, v in CENSUS.items()}, **PADDED)

# the (n, m) a handle can have (pick_variant refuses m >= 2 unless n = 4), and the spec the tests of the per-problem
# dense-algebra kernels dispatched on (n, m) use for each: k_tvlqr, k_gn_direction(_box), k_dare, k_terminal_cost<N>,
# k_feedback_control.  Those kernels read n and m from the handle and nothing else of the model.
NM_PAIRS = [(2, 1), (3, 1), (4, 1), (4, 2), (4, 3), (4, 4)]
NM_SPEC = {
    (2, 1): "phnn<n=2,hid=64,Gnet>",
    (3, 1): "odefunc<n=3,hid=128,f16x2>",
    (4, 1): "phnn<n=4,hid=128,fixedG,f16x2>",
    (4, 2): "phnn<n=4,m=2,hid=128,fixedG,f16x2>",
    (4, 3): "phnn<n=4,m=3,hid=128,fixedG,f16x2>",
    (4, 4): "phnn<n=4,m=4,hid=128,fixedG,f16x2>",
}

# requests phnn_create must refuse: spec id -> (spec, regex the error message must match)
REFUSED = {
    "odefunc<n=2,silu>": (ode(2, 128, act="silu"), "activation"),
    "phnn<n=4,relu> f16x2": (phnn(4, 128, True, act="relu", matmul="f16x2"), "activation"),
    "canonical<gelu> bf16x3": (canon(128, act="gelu", matmul="bf16x3"), "activation"),
    "odefunc<n=4,elu> f16x2": (ode(4, 128, act="elu", matmul="f16x2"), "activation"),
    "phnn<n=4,m=2,silu>": (phnn(4, 128, True, m=2, act="silu"), "activation"),
    "canonical<m=2,mass=diagonal>": (canon(128, m=2, mass="diagonal"), "input_dim m = 2..4"),
    "canonical<m=3,mass=constant>": (canon(128, m=3, mass="constant"), "input_dim m = 2..4"),
    "phnn<n=2,hid=64> f16x2 unforced": (phnn(2, 64, False, matmul="f16x2"), "force_matmul"),
    "canonical<hid=64> f16x2 unforced": (canon(64, matmul="f16x2"), "force_matmul"),
    "odefunc<n=2,hid=64> f16x2 unforced": (ode(2, 64, matmul="f16x2"), "force_matmul"),
    "phnn<n=3>": (phnn(3, 128, True), "no kernel instantiated"),
    "phnn<n=2,hid=128,fixedG> f32": (phnn(2, 128, True, matmul="f32"), "f16x2 kernels only"),
    "phnn<n=4,hid=128,Gnet> bf16x3": (phnn(4, 128, False, matmul="bf16x3"), "f16x2 kernels only"),
    "phnn<n=4,m=2> f32": (phnn(4, 128, True, m=2, matmul="f32"), "input_dim m = 2..4"),
    "canonical<mass=full> f32": (canon(128, mass="full", matmul="f32"), "MassMatrixNetwork"),
    "odefunc<n=4,hid=128> m=2": (spec("odefunc", 4, 128, m=2), "input_dim m = 2..4"),
}

# requests served by another variant than the options ask for, without an error (what pick_variant does today):
# spec id -> (spec, variant that serves it)
FALLBACKS = {
    "odefunc<n=2,hid=128> bf16x3": (ode(2, 128, matmul="bf16x3"), "odefunc<n=2,hid=128>"),
    "odefunc<n=3,hid=128> bf16x3": (ode(3, 128, matmul="bf16x3"), "odefunc<n=3,hid=128>"),
    "odefunc<n=4,hid=128> f16x2": (ode(4, 128, matmul="f16x2"), "odefunc<n=4,hid=128>"),
    "odefunc<n=4,hid=128> bf16x3": (ode(4, 128, matmul="bf16x3"), "odefunc<n=4,hid=128>"),
    "odefunc<n=2,hid=64> bf16x3": (ode(2, 64, matmul="bf16x3"), "odefunc<n=2,hid=64>"),
    "phnn<n=2,hid=64,Gnet> bf16x3": (phnn(2, 64, False, matmul="bf16x3"), "phnn<n=2,hid=64,Gnet>"),
    "phnn<n=4,hid=64,fixedG> bf16x3": (phnn(4, 64, True, matmul="bf16x3"), "phnn<n=4,hid=64,fixedG>"),
    "canonical<hid=64> bf16x3": (canon(64, matmul="bf16x3"), "canonical<hid=64>"),
    "odefunc<n=3>/64,64,64": (ode(3, 64), "odefunc<n=3,hid=128,f16x2>"),  # no 64-wide n = 3 kernel: padded to 128
}


# ----------------------------------------------------------------------------- the source's own lists
def _read(name, csrc):
    with open(os.path.join(csrc, name)) as f:
        return f.read()


def source_variants(csrc=CSRC):
    """-> ({enum: variant name} of PHNN_FOR_EACH_VARIANT, [variant names with split-tile kernels],
    [variant names with weight-gradient kernels])."""
    src = _read("phnn_variants.h", csrc)
    body = src[src.index("#define PHNN_FOR_EACH_VARIANT"):]
    names = dict(re.findall(r'X\((V_\w+),\s*M_\w+,\s*"([^"]+)"\)', body))
    split = re.findall(r"case\s+(V_\w+)\s*:\s*\*g\s*=\s*split_set<", _read("phnn_split.hip", csrc))
    wsrc = _read("phnn_wgrad.hip", csrc)
    wgrad = re.findall(r"^\s*PHNN_WCASE\((V_\w+),\s*M_\w+\)\s*$", wsrc, flags=re.M)
    return names, [names[v] for v in split], [names[v] for v in wgrad]


# ----------------------------------------------------------------------------- seeded state_dicts
def seed_of(spec_id, s):
    return zlib.crc32(spec_id.encode()) + s["salt"]


def _fixture(fname):
    with np.load(os.path.join(GOLDEN, fname)) as z:
        return {k: z[k] for k in z.files}


def _linear(rng, fan_out, fan_in):
    b = 1.0 / np.sqrt(fan_in)
    return (rng.uniform(-b, b, size=(fan_out, fan_in)).astype(np.float32),
            rng.uniform(-b, b, size=(fan_out,)).astype(np.float32))


def _mlp(sd, rng, prefix, d_in, hidden, d_out):
    dims = [d_in] + list(hidden) + [d_out]
    for i in range(len(dims) - 1):
        W, b = _linear(rng, dims[i + 1], dims[i])
        sd[f"{prefix}{2 * i}.weight"], sd[f"{prefix}{2 * i}.bias"] = W, b


def _canonical_G(m, rng):
    if m == 1:
        return _fixture("weights_canonical_cartpole.npz")["G"]
    if m == 2:
        return _fixture("golden_m2.npz")["w/canonical_m2/G"]
    if m == 3:
        return _fixture("golden_m34.npz")["w/canonical_m3/G"]
    return rng.uniform(-1, 1, size=(4, m)).astype(np.float32)


def _phnn_G(n, m, rng):
    if n == 4 and m == 1:
        return _fixture("weights_phnn_cartpole.npz")["G_fixed"]
    if n == 4 and m == 2:
        return _fixture("golden_m2.npz")["w/phnn_m2_fix/G_fixed"]
    if n == 4 and m == 3:
        return _fixture("golden_m34.npz")["w/phnn_m3_fix/G_fixed"]
    return rng.uniform(-1, 1, size=(n, m)).astype(np.float32)


def build_state_dict(spec_id, s, hidden_scale=1.0):
    """Reference-layout state_dict (numpy float32) of spec `s`, seeded from crc32(spec_id).  hidden_scale multiplies
    every MLP weight matrix (tanh saturation, other f16x2 image scales)."""
    rng = np.random.default_rng(seed_of(spec_id, s))
    n, m, wd = s["n"], s["m"], s["widths"]
    sd = {}
    if s["kind"] == "phnn":
        J = (_fixture("weights_phnn_cartpole.npz")["J"] if n == 4 else
             _fixture("weights_phnn_pendulum.npz")["J"] if n == 2 else None)
        if J is None:
            A = rng.uniform(-1, 1, size=(n, n))
            J = (A - A.T).astype(np.float32)
        sd["J"] = J
        if s["fixed_G"]:
            sd["G_fixed"] = _phnn_G(n, m, rng)
        _mlp(sd, rng, "R_net.net.", n, wd["R"], n * n)
        _mlp(sd, rng, "H_net.net.", n, wd["H"], 1)
        if not s["fixed_G"]:
            _mlp(sd, rng, "G_net.net.", n, wd["G"], n * m)
    elif s["kind"] == "canonical":
        if s["mass"] == "cartpole":
            w = _fixture("weights_canonical_cartpole.npz")
            for k in ("R_diag_raw", "J", "M_net.log_a", "M_net.b", "M_net.log_c"):
                sd[k] = w[k]
            sd["G"] = _canonical_G(m, rng)
        else:
            g = _fixture("golden_mass.npz")
            pre = f"w/{s['mass']}/"
            for k in g:
                if k.startswith(pre) and (k[len(pre):].startswith("M_net.") or k[len(pre):] in ("R_diag_raw", "J")):
                    sd[k[len(pre):]] = g[k]
            sd["G"] = g[pre + "G"] if m == 1 else rng.uniform(-1, 1, size=(4, m)).astype(np.float32)
        _mlp(sd, rng, "H_net.net.", n, wd["H"], 1)
    else:
        _mlp(sd, rng, "network.", n + m, wd["net"], n)
    if hidden_scale != 1.0:
        mlp = ("R_net.net.", "H_net.net.", "G_net.net.", "network.")
        for k in sd:
            if k.endswith(".weight") and k.startswith(mlp):
                sd[k] = (sd[k] * np.float32(hidden_scale)).astype(np.float32)
    return sd


def engine_kwargs(s):
    return dict(activation=s["act"], matmul=s["matmul"], force_matmul=s["force"])


# ----------------------------------------------------------------------------- seeded inputs
X_SCALE = {2: [1.5, 0.8], 3: [1.0, 0.5, 0.5], 4: [1.0, 0.3, 0.5, 0.5]}
U_MIN, U_MAX = -1.5, 2.0  # asymmetric, exactly representable
POINT_B = 37
ROLL_SHAPES = [(1, 1), (1, 13), (37, 1), (37, 13)]
BARRIER_SHAPE = (37, 13)  # the one shape also run with the state barrier active


def dt_of(s):
    return 0.02 if s["n"] == 4 else 0.05


def states(rng, n, B):
    return (rng.uniform(-1, 1, size=(B, n)) * X_SCALE[n]).astype(np.float32)


def controls(rng, B, H, m):
    """(B,H,m) controls: about 20 % outside [U_MIN, U_MAX], about 10 % exactly on a bound."""
    w = U_MAX - U_MIN
    U = rng.uniform(U_MIN - 0.125 * w, U_MAX + 0.125 * w, size=(B, H, m)).astype(np.float32)
    on = rng.random(size=U.shape) < 0.1
    U[on] = np.where(rng.random(size=int(on.sum())) < 0.5, U_MIN, U_MAX).astype(np.float32)
    return U


def cost_of(s, rng, barrier=False):
    """Full non-symmetric Q, non-symmetric m x m R, nonzero x_target; optionally the soft state barrier."""
    n, m = s["n"], s["m"]
    Q = np.diag([10.0, 20.0, 1.0, 5.0][:n]) + 0.1 * rng.uniform(-1, 1, size=(n, n))
    R = 0.01 * (np.eye(m) + 0.1 * rng.uniform(-1, 1, size=(m, m)))
    xt = 0.1 * rng.uniform(-1, 1, size=n) * X_SCALE[n]
    if not barrier:
        return _capi.make_cost(n, m, Q, R, xt, U_MIN, U_MAX)
    sc = np.asarray(X_SCALE[n])
    return _capi.make_cost(n, m, Q, R, xt, U_MIN, U_MAX, x_min=list(-0.4 * sc), x_max=list(0.35 * sc))


def inputs(spec_id, s):
    """The census inputs of one spec, shared by the CPU and GPU tests."""
    rng = np.random.default_rng(seed_of(spec_id, s) + 1)
    n, m, B = s["n"], s["m"], POINT_B
    d = {"dt": dt_of(s), "cost": cost_of(s, rng), "cost_barrier": cost_of(s, rng, barrier=True)}
    d["x"], d["u"] = states(rng, n, B), rng.uniform(U_MIN, U_MAX, size=(B, m)).astype(np.float32)
    d["lam"], d["Hbar"] = rng.normal(size=(B, n)).astype(np.float32), rng.normal(size=B).astype(np.float32)
    for B_, H in ROLL_SHAPES:
        d[(B_, H)] = (states(rng, n, B_), controls(rng, B_, H, m))
    Bw, Hw = 37, 13
    d["traj_bar"] = rng.normal(size=(Bw, Hw + 1, n)).astype(np.float32)
    d["dx_bar"] = rng.normal(size=(Bw, Hw, n)).astype(np.float32)
    d["cost_bar"] = rng.normal(size=Bw).astype(np.float32)
    return d


# ----------------------------------------------------------------------------- stated tolerances (test_gpu_parity.py)
COST_RTOL = 1e-5
TRAJ_RTOL, TRAJ_ATOL = 1e-5, 1e-5
GRAD_TOL = 1e-4   # of max|grad| per rollout
POINT_TOL = 2e-5  # f(x,u), VJP: of max|.| over the batch
WGRAD_TOL = 1e-4  # every parameter tensor: of its largest reference entry (test_gpu_wgrad.py TOL)
RELU_GRAD_TOL = 2e-3  # ReLU: one unit's mask may flip where float32 rounds a pre-activation across 0 (test_gpu_activations.py)


def grad_tol(s):
    return (RELU_GRAD_TOL if s["act"] == "relu" else GRAD_TOL) * s["tol"]


def err_cost(c, ref):
    return float(np.abs(np.asarray(c, np.float64) / ref - 1).max())


def err_traj(tr, ref):
    """max |tr - ref| / (atol + rtol |ref|): <= 1 within the stated tolerance."""
    return float((np.abs(np.asarray(tr, np.float64) - ref) / (TRAJ_ATOL + TRAJ_RTOL * np.abs(ref))).max())


def err_rows(g, ref):
    """max over rows of max|g - ref| / max|ref| (per rollout; rows whose reference is all zero need g == 0)."""
    g, ref = np.asarray(g, np.float64).reshape(len(ref), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    mx = np.abs(ref).max(axis=1)
    d = np.abs(g - ref).max(axis=1)
    return float(np.max(np.where(mx > 0, d / np.where(mx > 0, mx, 1.0), np.where(d > 0, np.inf, 0.0))))


def err_max(a, ref, floor=1e-30):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / max(float(np.abs(ref).max()), floor))


def err_named(named, ref_named):
    """worst over parameter tensors of max|ours - ref| / max|ref| (test_gpu_wgrad.check_named; zero tensors exact)."""
    worst = 0.0
    for k, ref in ref_named.items():
        ref = np.asarray(ref, np.float64)
        ours = np.asarray(named[k], np.float64).reshape(ref.shape)
        mx = np.abs(ref).max()
        e = (np.abs(ours - ref).max() / mx) if mx > 0 else (0.0 if np.all(ours == 0) else np.inf)
        worst = max(worst, float(e))
    return worst
