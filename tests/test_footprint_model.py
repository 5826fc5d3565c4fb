"""The footprint arena (tests/footprint.py) on CPU tensors: the layout arithmetic, what check() reports and what it
ignores, and that the 0xFF fill is NaN to every float view.  The GPU properties are in tests/test_gpu_footprint.py."""
import numpy as np
import pytest
import torch

import footprint as fp

REGIONS = [
    ("x0", 19 * 2 * 4, fp.IN, 8),
    ("u", 19 * 13 * 4, fp.IN, 52),
    ("cost", 19 * 4, fp.OUT, 4),
    ("traj", 19 * 14 * 2 * 4, fp.OUT, 0),
    ("state", 19 * 4 * 8, fp.INOUT, 32),
    ("empty", 0, fp.OUT, 0),
    ("ws", 4096 + 256, fp.WS, 0),
    ("odd", 37, fp.OUT, 12),
]


def _regions():
    return [fp.Region(*r) for r in REGIONS]


@pytest.mark.parametrize("guard", [fp.GUARD, 256, 1000])
def test_layout_disjoint_and_aligned(guard):
    at, total = fp.layout(_regions(), guard)
    spans = []
    for name, nbytes, _role, skew in REGIONS:
        s, n = at[name]
        assert n == nbytes
        assert s % fp.ALIGN == skew, (name, s)
        spans.append((s - guard, s, name + ".front"))
        spans.append((s, s + n, name))
        spans.append((s + n, s + n + guard, name + ".back"))
    assert spans[0][0] >= guard and spans[-1][1] + guard <= total and total % fp.ALIGN == 0  # slack at both ends
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a0 <= a1 <= b0 <= b1, (an, bn)  # in order and disjoint: neighbours' guards do not overlap either


def test_guard_width_is_the_stated_condition():
    assert fp.GUARD == 64 * 1024
    # larger than a vector access, a workspace sub-region rounding, one tile's store of an activation vector (1 KiB)
    # and the whole tape of one dynamics evaluation of a 128-wide model (one Euler stash step, 17.5 KiB)
    assert fp.GUARD > 16 and fp.GUARD > fp.ALIGN and fp.GUARD > 1024 and fp.GUARD > 17920


def test_workspaces_are_never_skewed():
    with pytest.raises(AssertionError):
        fp.Region("ws", 256, fp.WS, 8)


def test_views_and_pointers():
    a = fp.Arena(torch, "cpu", _regions())
    base = a.buf.data_ptr()
    for name, nbytes, _role, skew in REGIONS:
        assert a.ptr(name).value == base + a.at[name][0]
        assert (a.ptr(name).value - base) % fp.ALIGN == skew
        assert a.interior(name).numel() == nbytes
    assert a.view("x0", torch.float32, (19, 2)).data_ptr() == a.ptr("x0").value
    assert a.view("state", torch.float64, (19, 4)).shape == (19, 4)


def test_fill_spares_inputs_and_covers_the_rest():
    a = fp.Arena(torch, "cpu", _regions())
    x0 = torch.arange(38, dtype=torch.float32).reshape(19, 2)
    a.load("x0", x0)
    st = torch.arange(76, dtype=torch.float64).reshape(19, 4)
    a.load("state", st)
    a.fill(0xFF)
    assert torch.equal(a.view("x0", torch.float32, (19, 2)), x0)
    assert torch.equal(a.view("state", torch.float64, (19, 4)), st)
    mask = torch.ones(a.total, dtype=torch.bool)
    for name in ("x0", "u", "state"):
        s, n = a.at[name]
        mask[s: s + n] = False
    assert bool((a.buf[mask] == 0xFF).all())
    assert a.check() == []
    a.fill(0x00, input_guard_byte=0xFF)
    for name, _n, role, _s in REGIONS:
        for (g0, g1) in a.guards(name):
            assert bool((a.buf[g0:g1] == (0xFF if role == fp.IN else 0x00)).all()), name
    assert bool((a.interior("traj") == 0).all()) and a.check() == []


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_check_reports_guard_edges_and_ignores_interiors(byte):
    a = fp.Arena(torch, "cpu", _regions())
    a.fill(byte)
    for name, nbytes, _role, _skew in REGIONS:  # interiors are free to change
        if nbytes:
            a.interior(name).fill_(0x5A)
    assert a.check() == []
    other = byte ^ 0x01
    for name, _n, _role, _skew in REGIONS:
        (f0, f1), (b0, b1) = a.guards(name)
        assert f1 - f0 == fp.GUARD and b1 - b0 == fp.GUARD
        for side, pos, off in (("front", f0, 0), ("front", f1 - 1, fp.GUARD - 1), ("back", b0, 0), ("back", b1 - 1, fp.GUARD - 1)):
            a.buf[pos] = other
            assert a.check() == [(name, side, off)], (name, side, off)
            a.buf[pos] = byte
    assert a.check() == []
    # two hits: both reported, each with its first changed byte
    (f0, f1), (b0, b1) = a.guards("cost")
    a.buf[f1 - 4: f1] = other
    a.buf[b0 + 8: b0 + 12] = other
    assert a.check() == [("cost", "front", fp.GUARD - 4), ("cost", "back", 8)]


def test_read_fence_bytes_are_tracked_per_guard():
    a = fp.Arena(torch, "cpu", _regions())
    a.fill(0x00, input_guard_byte=0xFF)
    assert a.check() == []
    g = a.guards("u")[1][0]
    a.buf[g] = 0x00  # an input's guard holds 0xFF: a zero there is a change
    assert a.check() == [("u", "back", 0)]


def test_ff_fill_is_nan_in_float_views():
    a = fp.Arena(torch, "cpu", _regions())
    a.fill(0xFF)
    assert bool(torch.isnan(a.view("traj", torch.float32, (19, 14, 2))).all())
    assert bool(torch.isnan(a.view("cost", torch.float32, (19,))).all())
    assert bool(torch.isnan(a.interior("ws")[:4096].view(torch.float64)).all())
    (f0, f1), _ = a.guards("ws")
    assert bool(torch.isnan(a.buf[f0:f1].view(torch.float32)).all()) and bool(torch.isnan(a.buf[f0:f1].view(torch.float64)).all())
    assert bool((a.view("cost", torch.float32, (19,)).view(torch.int32) == -1).all())


def test_written_span():
    a = fp.Arena(torch, "cpu", _regions())
    a.fill(0xFF)
    assert a.written("ws", 0xFF) is None
    a.interior("ws")[256:512] = 0
    assert a.written("ws", 0xFF) == (256, 512)


def test_buf_row_skew_is_a_row_slice():
    for shape, dt in (((19, 2), np.float32), ((19, 3), np.float32), ((19, 13, 1), np.float32), ((19, 4), np.float32),
                      ((19, 4), np.float64), ((19,), np.int32)):
        b = fp.Buf("t", dt, shape, fp.IN, np.zeros(shape, dt))
        t = torch.zeros(*shape, dtype=fp._torch_dtype(torch, dt))
        assert b.row_skew == (t[1:].data_ptr() - t.data_ptr()) % fp.ALIGN
    assert [fp.Buf("t", np.float32, s, fp.IN).row_skew for s in ((19, 2), (19, 3), (19, 13, 1))] == [8, 12, 52]
    assert fp.Buf("w", np.uint8, (4096,), fp.WS).row_skew == 0
    # rows of n = 4 states stay 16-byte aligned under a row slice
    assert fp.Buf("t", np.float32, (19, 4), fp.IN).row_skew % 16 == 0
