"""The variant census (tests/variant_census.py) on the CPU: it covers the library's kernel variants, split-tile sets and
weight-gradient sets exactly; every spec packs and builds in the float64 oracle; refused requests are refused by
phnn_create before any device is touched; and on the census inputs the float32 oracle stays within a fifth of every
stated tolerance of the float64 oracle, so a correct float32 kernel has room to pass tests/test_gpu_variant_census.py."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import oracle_lib as ol
import variant_census as vc
from phnn_mpc_amd import _capi, weights

MARGIN = 0.2  # float32-vs-float64 error of the oracle, as a fraction of the stated tolerance


def test_census_covers_the_source_exactly():
    names, split, wgrad = vc.source_variants()
    assert len(names) == len(set(names.values())) == 50
    assert set(vc.CENSUS) == set(names.values()), (sorted(set(names.values()) - set(vc.CENSUS)),
                                                   sorted(set(vc.CENSUS) - set(names.values())))
    assert {k for k, s in vc.CENSUS.items() if s["split"]} == set(split)
    assert {k for k, s in vc.CENSUS.items() if s["wgrad"]} == set(wgrad)
    assert len(split) == 3 and len(wgrad) == 23
    for sid, (variant, s) in vc.PADDED.items():
        ref = vc.CENSUS[variant]
        assert (s["split"], s["wgrad"]) == (ref["split"], ref["wgrad"]), sid


def test_census_check_fails_on_an_uncovered_variant(tmp_path):
    """A variant added to PHNN_FOR_EACH_VARIANT without a census entry is noticed."""
    for f in ("phnn_variants.h", "phnn_split.hip", "phnn_wgrad.hip"):
        shutil.copy(os.path.join(vc.CSRC, f), tmp_path / f)
    p = tmp_path / "phnn_variants.h"
    src = p.read_text()
    last = re.findall(r'  X\(V_\w+, M_\w+, "[^"]+"\)$', src, flags=re.M)[-1]
    p.write_text(src.replace(last, last + ' \\\n  X(V_ODE_4_64, M_ODE_4_64, "odefunc<n=4,hid=64>")'))
    names, _, _ = vc.source_variants(str(tmp_path))
    assert "odefunc<n=4,hid=64>" in names.values() and set(vc.CENSUS) != set(names.values())


@pytest.mark.parametrize("sid", list(vc.ALL_SPECS))
def test_spec_packs_and_builds_in_the_oracle(sid):
    variant, s = vc.ALL_SPECS[sid]
    sd = vc.build_state_dict(sid, s)
    assert all(v.dtype == np.float32 for v in sd.values())
    d, blob = weights.pack_state_dict(sd, activation=s["act"])
    assert (d.n, d.m) == (s["n"], s["m"])
    assert blob.size == sum(int(np.prod(sh)) for _, _, sh in weights.blob_layout(sd))
    ol.OracleModel(sd, "f64", activation=s["act"])
    # same seed, same weights; another spec id, other weights
    assert all(np.array_equal(v, vc.build_state_dict(sid, s)[k]) for k, v in sd.items())
    if "H_net.net.0.weight" in sd:
        assert not np.array_equal(sd["H_net.net.0.weight"], vc.build_state_dict(sid + "/x", s)["H_net.net.0.weight"])


def test_nm_table_covers_every_reachable_pair():
    """Every (n, m) a handle can have is listed and mapped to a spec with that pair, so the tests of the kernels
    dispatched on (n, m), which take their specs from NM_SPEC, leave no reachable instantiation out."""
    assert set(vc.NM_PAIRS) == {(s["n"], s["m"]) for s in vc.CENSUS.values()}
    assert list(vc.NM_SPEC) == vc.NM_PAIRS
    for pair, sid in vc.NM_SPEC.items():
        assert (vc.CENSUS[sid]["n"], vc.CENSUS[sid]["m"]) == pair, (pair, sid)


def _create_error(s, sd):
    """phnn_create_ex on this machine: the description is validated and a variant picked before any device is
    opened, so a refusal reads the same with or without a GPU."""
    lib = _capi.load_library()
    d, blob = weights.pack_state_dict(sd, activation=s["act"])
    opt = _capi.Options()
    opt.matmul_mode = _capi.MATMUL_MODES[s["matmul"]]
    opt.force_matmul = int(s["force"])
    h = C.c_void_p()
    rc = lib.phnn_create_ex(C.byref(d), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, 0, C.byref(opt),
                            C.byref(h))
    if rc == 0:
        lib.phnn_destroy(h)
        return None
    msg = lib.phnn_last_error(None)
    return msg.decode() if msg else ""


@pytest.mark.parametrize("sid", list(vc.REFUSED))
def test_refused_requests_are_refused_with_a_reason(sid):
    s, why = vc.REFUSED[sid]
    msg = _create_error(s, vc.build_state_dict(sid, s))
    assert msg is not None and re.search(why, msg), (sid, msg)


@pytest.mark.parametrize("sid", list(vc.ALL_SPECS) + list(vc.FALLBACKS))
def test_served_requests_pass_variant_selection(sid):
    """Specs with a kernel get past phnn_create's validation (without a GPU they stop at opening the device)."""
    s = vc.ALL_SPECS[sid][1] if sid in vc.ALL_SPECS else vc.FALLBACKS[sid][0]
    msg = _create_error(s, vc.build_state_dict(sid, s))
    if msg is not None:
        assert "HIP device" in msg or "hip" in msg.lower(), (sid, msg)


def _margins(sid, s):
    """{check: float32-oracle error / stated tolerance} on the census inputs."""
    sd = vc.build_state_dict(sid, s)
    m32, m64 = ol.OracleModel(sd, "f32", activation=s["act"]), ol.OracleModel(sd, "f64", activation=s["act"])
    d = vc.inputs(sid, s)
    gt = vc.grad_tol(s)
    out = {}
    for scale in (1.0, 3.0):
        if scale != 1.0:
            sd3 = vc.build_state_dict(sid, s, hidden_scale=scale)
            m32, m64 = ol.OracleModel(sd3, "f32", activation=s["act"]), ol.OracleModel(sd3, "f64", activation=s["act"])
        (dx, H), (rdx, rH) = m32.forward(d["x"], d["u"]), m64.forward(d["x"], d["u"])
        out[f"f x{scale:g}"] = vc.err_max(dx, rdx) / vc.POINT_TOL
        out[f"H x{scale:g}"] = float(np.abs(H - rH).max() / max(1.0, np.abs(rH).max())) / vc.POINT_TOL
        (xb, ub), (rxb, rub) = m32.vjp(d["x"], d["u"], d["lam"]), m64.vjp(d["x"], d["u"], d["lam"])
        out[f"vjp x{scale:g}"] = max(vc.err_max(xb, rxb), vc.err_max(ub, rub)) / (vc.POINT_TOL if s["act"] != "relu" else gt)
    m32, m64 = ol.OracleModel(sd, "f32", activation=s["act"]), ol.OracleModel(sd, "f64", activation=s["act"])
    for integ in ("euler", "rk4"):
        for (B, H) in vc.ROLL_SHAPES:
            x0, U = d[(B, H)]
            for ck in ("cost", "cost_barrier") if (B, H) == vc.BARRIER_SHAPE else ("cost",):
                a = m32.rollout(x0, U, d[ck], integ, d["dt"], nthreads=8)
                r = m64.rollout(x0, U, d[ck], integ, d["dt"], nthreads=8)
                k = f"{integ} B{B} H{H} {ck}"
                out[k + " cost"] = vc.err_cost(a["cost"], r["cost"]) / vc.COST_RTOL
                out[k + " traj"] = vc.err_traj(a["traj"], r["traj"])
                out[k + " grad_u"] = vc.err_rows(a["grad_u"], r["grad_u"]) / gt
                out[k + " grad_x0"] = vc.err_rows(a["grad_x0"], r["grad_x0"]) / gt
        x0, U = d[(37, 13)]
        for cb in (None, d["cost_bar"]):
            a = m32.rollout_vjp(x0, U, d["cost"], integ, d["dt"], traj_bar=d["traj_bar"], cost_bar=cb)
            r = m64.rollout_vjp(x0, U, d["cost"], integ, d["dt"], traj_bar=d["traj_bar"], cost_bar=cb)
            out[f"{integ} rollout_vjp cost_bar={cb is not None}"] = max(vc.err_rows(a[0], r[0]), vc.err_rows(a[1], r[1])) / gt
        if s["wgrad"]:
            a = m32.rollout_wgrad(x0, U, integ, d["dt"], d["traj_bar"], d["dx_bar"])
            r = m64.rollout_wgrad(x0, U, integ, d["dt"], d["traj_bar"], d["dx_bar"])
            lay = weights.blob_layout(sd)
            out[f"{integ} rollout_wgrad"] = vc.err_named(weights.unpack_grad_blob(None, a["grad_theta"], layout=lay),
                                                         weights.unpack_grad_blob(None, r["grad_theta"], layout=lay)) / vc.WGRAD_TOL
    if s["wgrad"]:
        lay = weights.blob_layout(sd)
        a, r = m32.wgrad(d["x"], d["u"], d["lam"], d["Hbar"]), m64.wgrad(d["x"], d["u"], d["lam"], d["Hbar"])
        out["model_wgrad"] = vc.err_named(weights.unpack_grad_blob(None, a, layout=lay),
                                          weights.unpack_grad_blob(None, r, layout=lay)) / vc.WGRAD_TOL
    return out


@pytest.mark.parametrize("sid", list(vc.ALL_SPECS))
def test_float32_oracle_leaves_room_under_the_tolerances(sid):
    variant, s = vc.ALL_SPECS[sid]
    out = _margins(sid, s)
    bad = {k: round(v, 3) for k, v in out.items() if not v <= MARGIN}
    assert not bad, (sid, bad)


def test_census_controls_hit_the_bounds():
    rng = np.random.default_rng(0)
    U = vc.controls(rng, 37, 13, 2)
    outside = (U < vc.U_MIN) | (U > vc.U_MAX)
    on = (U == vc.U_MIN) | (U == vc.U_MAX)
    assert 0.12 < outside.mean() < 0.25 and 0.06 < on.mean() < 0.14
    assert (U == vc.U_MIN).any() and (U == vc.U_MAX).any()
