"""CPU tests of reference tracking's host side: how a reference tensor maps to phnn_reference (engine.reference_view:
broadcast dimensions become stride 0, nothing is materialised, a copy only for a non-contiguous last dimension), the
ctypes struct against the header, and that an engine without reference tracking refuses x_ref instead of ignoring it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import yaml

import oracle_lib as ol
from oracle_engine import OracleEngine
from phnn_mpc_amd import _capi
from phnn_mpc_amd.engine import reference_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "configs", "cartpole_mpc.yaml")
B, ROWS, N = 5, 7, 4


def addressed(t, bs, ts, rows, B=B, n=N):
    """(B, rows, n) of what the kernel reads: element [b, row, i] at t.data_ptr() + 4 * (b * bs + row * ts + i)."""
    assert t.dtype == torch.float32 and (n == 1 or t.stride(-1) == 1)
    return torch.as_strided(t, (B, rows, n), (bs, ts, 1))


def check(x_ref, want, bs, ts, rows, in_place=None):
    """in_place: the tensor whose storage the view must share (no copy)."""
    t, got_bs, got_ts, got_rows = reference_view(x_ref, B, N)
    assert (got_bs, got_ts, got_rows) == (bs, ts, rows)
    assert torch.equal(addressed(t, got_bs, got_ts, got_rows), want)
    if in_place is not None:
        assert t.untyped_storage().data_ptr() == in_place.untyped_storage().data_ptr()
    return t


def test_shared_setpoint():
    r = torch.arange(N, dtype=torch.float32)
    check(r, r.expand(B, 1, N), 0, 0, 1, in_place=r)


def test_per_problem_setpoints():
    r = torch.randn(B, 1, N)
    check(r, r, N, 0, 1, in_place=r)


def test_shared_time_varying_trajectory():
    r = torch.randn(ROWS, N)
    check(r, r.expand(B, ROWS, N), 0, N, ROWS, in_place=r)


def test_per_problem_time_varying():
    r = torch.randn(B, ROWS, N)
    check(r, r, ROWS * N, N, ROWS, in_place=r)


def test_expanded_dimensions_map_to_stride_zero_without_a_copy():
    base = torch.randn(1, ROWS, N)
    check(base.expand(B, ROWS, N), base.expand(B, ROWS, N), 0, N, ROWS, in_place=base)
    const = torch.randn(B, 1, N)
    check(const.expand(B, ROWS, N), const.expand(B, ROWS, N), N, 0, ROWS, in_place=const)


def test_permuted_layout_is_used_in_place():
    src = torch.randn(ROWS, B, N)  # time-major storage, (B, rows, n) view
    r = src.permute(1, 0, 2)
    check(r, r, N, B * N, ROWS, in_place=src)


def test_non_contiguous_last_dimension_is_copied():
    wide = torch.randn(B, ROWS, 2 * N)
    r = wide[..., ::2]
    t = check(r, r, ROWS * N, N, ROWS, in_place=None)
    assert t.untyped_storage().data_ptr() != wide.untyped_storage().data_ptr()
    # a broadcast problem dimension is not materialised by that copy
    shared = wide[:1, :, ::2].expand(B, ROWS, N)
    t = check(shared, shared, 0, N, ROWS, in_place=None)
    assert t.untyped_storage().nbytes() == 4 * ROWS * N


def test_last_dimension_of_one_broadcasts_over_the_state():
    r = torch.randn(B, ROWS, 1)
    check(r, r.expand(B, ROWS, N), ROWS * N, N, ROWS)


def test_numpy_and_other_dtypes_become_float32():
    r = np.linspace(0, 1, ROWS * N).reshape(ROWS, N)  # float64
    check(r, torch.tensor(r, dtype=torch.float32).expand(B, ROWS, N), 0, N, ROWS)


@pytest.mark.parametrize("shape", [(B + 1, ROWS, N), (2, ROWS, N), (B, ROWS, N + 1), (ROWS, N - 1), (1, B, ROWS, N), (),
                                   (B, 0, N)])
def test_non_broadcastable_shapes_are_rejected(shape):
    with pytest.raises(ValueError):
        reference_view(torch.zeros(shape), B, N)


def test_reference_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "phnn_mpc.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef).)*?)\} phnn_reference;", header, re.S).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _capi.Reference._fields_]
    # pointer, 2 x int64, int32 (+4 padding), pointer, int32 (+4 padding)
    assert C.sizeof(_capi.Reference) == 48
    assert _capi.Reference.offset_dev.offset == 32


def test_engines_without_reference_tracking_refuse_x_ref():
    from phnn_mpc_amd.models import pHNN, pHNN_Canonical
    from phnn_mpc_amd.mpc_controller import create_mpc_from_config
    from phnn_mpc_amd.mpc_controller_canonical import create_mpc_controller
    from phnn_mpc_amd.solver import shooting_solve
    cfg = yaml.safe_load(open(CFG))
    x = np.zeros((2, 4), np.float32)
    r = np.ones((2, 3, 4), np.float32)
    for name, cls, make in (("phnn_cartpole", pHNN, create_mpc_from_config),
                            ("canonical_cartpole", pHNN_Canonical, create_mpc_controller)):
        w = ol.load_weights(name)
        m = cls(CFG)
        m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
        eng = OracleEngine(w)
        c = make(m.set_engine(eng), cfg)
        with pytest.raises(NotImplementedError):
            c.control_batch(x, x_ref=r) if hasattr(c, "control_batch") else c.compute_control_batch(x, x_ref=r)
        with pytest.raises(NotImplementedError):
            shooting_solve(eng, torch.zeros(2, 4), torch.zeros(2, 3, 1), c._cost(), "euler", 0.02, 0.1, 2, x_ref=r)
