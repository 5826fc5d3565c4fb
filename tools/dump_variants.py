#!/usr/bin/env python3
"""Outputs of every entry point for every kernel variant on seeded inputs, to compare two builds bit for bit.

    PHNN_LIB_PATH=/path/to/libphnn_mpc.so python tools/dump_variants.py out.npz

Walks tests/variant_census.CENSUS.  Per variant: forward and vjp on 40 points; K1 cost and trajectory and K2
grad_u / grad_x0 at B = 40 (two full tiles and a ragged one), H = 3, Euler and RK4, use_stash on and off, split-tile
"never" and "always" where the spec has split-tile kernels; where it has weight-gradient kernels also
rollout_trajectory, rollout_wgrad without and with K1's tapes, and model_wgrad.  Every array goes into out.npz under
"<variant>|<what>"; one sha256 per variant and one over all of them are printed.
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import variant_census as vc  # noqa: E402
from phnn_mpc_amd.engine import RolloutEngine  # noqa: E402

B, H = 40, 3


def npy(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def dump_variant(sid, s, out):
    sd = vc.build_state_dict(sid, s)
    rng = np.random.default_rng(vc.seed_of(sid + "/dump", s))
    n, m, dt = s["n"], s["m"], vc.dt_of(s)
    cost = vc.cost_of(s, rng)
    x, u = vc.states(rng, n, B), rng.uniform(vc.U_MIN, vc.U_MAX, size=(B, m)).astype(np.float32)
    lam, Hbar = rng.normal(size=(B, n)).astype(np.float32), rng.normal(size=B).astype(np.float32)
    x0, U = vc.states(rng, n, B), vc.controls(rng, B, H, m)
    traj_bar = rng.normal(size=(B, H + 1, n)).astype(np.float32)
    dx_bar = rng.normal(size=(B, H, n)).astype(np.float32)

    def put(what, *tensors):
        for k, t in enumerate(tensors):
            out[f"{sid}|{what}|{k}"] = npy(t)

    for split in ("never", "always") if s["split"] else ("never",):
        eng = RolloutEngine(sd, "cuda:0", **vc.engine_kwargs(s), split=split)
        assert eng.variant == sid, (eng.variant, sid)
        if split == "never":
            put("forward", *eng.forward(x, u))
            put("vjp", *eng.vjp(x, u, lam))
        for integ in ("euler", "rk4"):
            for stash in (True, False):
                eng.use_stash = stash
                tag = f"{integ} stash={int(stash)} split={split}"
                put("K1 " + tag, *eng.rollout_cost(x0, U, cost, integ, dt, want_traj=True))
                put("K2 " + tag, *eng.rollout_cost_grad(x0, U, cost, integ, dt, want_grad_x0=True))
            eng.use_stash = True
            if not s["wgrad"]:
                continue
            traj, dX = eng.rollout_trajectory(x0, U, integ, dt, want_dx=True)
            put(f"trajectory {integ} split={split}", traj, dX)
            if split == "never":
                put(f"rollout_wgrad {integ}", *eng.rollout_wgrad(x0, U, traj, integ, dt, traj_bar=traj_bar, dx_bar=dx_bar))
                traj_t = eng.rollout_trajectory(x0, U, integ, dt, tapes=True)
                put(f"rollout_wgrad {integ} tapes", traj_t, *eng.rollout_wgrad(x0, U, traj_t, integ, dt, traj_bar=traj_bar,
                                                                             dx_bar=dx_bar, tape_token=eng.tape_token))
        if s["wgrad"] and split == "never":
            put("model_wgrad", *eng.model_wgrad(x, u, lam, Hbar))
            put("model_wgrad no_Hbar", *eng.model_wgrad(x, u, lam))
        eng.close()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out, total = {}, hashlib.sha256()
    for sid, s in vc.CENSUS.items():
        before = len(out)
        dump_variant(sid, s, out)
        h = hashlib.sha256()
        for k in list(out)[before:]:
            h.update(k.encode() + out[k].tobytes())
        total.update(h.digest())
        print(f"{sid}: {len(out) - before} arrays sha256 {h.hexdigest()[:16]}", flush=True)
    np.savez(sys.argv[1], **out)
    print(f"all variants: {len(out)} arrays sha256 {total.hexdigest()[:16]} (library: "
          f"{os.environ.get('PHNN_LIB_PATH', 'the package build')})")


if __name__ == "__main__":
    main()
