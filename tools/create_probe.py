#!/usr/bin/env python3
"""Host time of phnn_create_ex and phnn_destroy for one handle that has all three kernel sets (the cart-pole pHNN:
phnn<n=4,hid=128,fixedG,f16x2> has whole-tile, split-tile and weight-gradient kernels): 20 create / destroy pairs after 3
warm-up pairs, medians.  For A/B runs of two builds of the library: AB_PROBES=tools/create_probe.py tools/ab_bench.sh."""
import ctypes as C, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from phnn_mpc_amd.engine import RolloutEngine

with np.load(os.path.join(ROOT, "tests", "golden", "weights_phnn_cartpole.npz")) as z:
    w = {k: z[k] for k in z.files}
eng = RolloutEngine(w)
lib = eng.lib
blob = eng.blob.ctypes.data_as(C.POINTER(C.c_float))
ts, td = [], []
for k in range(23):
    h = C.c_void_p()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = lib.phnn_create_ex(C.byref(eng.desc), blob, eng.blob.size, 0, C.byref(eng.options), C.byref(h))
    t1 = time.perf_counter()
    assert rc == 0 and h.value, rc
    lib.phnn_destroy(h)
    t2 = time.perf_counter()
    if k >= 3:
        ts.append((t1 - t0) * 1e3)
        td.append((t2 - t1) * 1e3)
print(f"variant {eng.variant}", flush=True)
print(f"create: {np.median(ts):.4f} ms median of {len(ts)} (min {min(ts):.4f})", flush=True)
print(f"destroy: {np.median(td):.4f} ms median of {len(td)} (min {min(td):.4f})", flush=True)
