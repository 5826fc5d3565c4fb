"""The workspace sizes of the three filter steps as include/phnn_mpc.h states them -- a sum of 256-byte aligned regions
written out here, not computed by the layout code under test (csrc/phnn_filter_layout.h).  A
handle is needed, no kernel runs."""
import pytest

from test_gpu_mppi import engine

pytestmark = pytest.mark.gpu


def regions(*floats):
    """Bytes of float32 regions laid out one after the other, each starting at a multiple of 256; at least 256."""
    return max(sum((4 * f + 255) // 256 * 256 for f in floats), 256)


@pytest.mark.parametrize("B", [0, 1, 17, 65, 4096])
def test_the_filter_workspaces_are_the_stated_regions(B):
    eng = engine("phnn_cartpole")
    n, m = 4, 1
    assert (eng.n, eng.m) == (n, m)
    S = 2 * n + 1
    # the control row (B,1,m), K1's trajectory (B,2,n) and cost (B), A (B,n,n), Bm (B,n,m)
    step = regions(B * m, B * 2 * n, B, B * n * n, B * n * m)
    # the sigma points (B,S,n), their control rows (B,S,1,m), K1's trajectory (B*S,2,n) and cost (B*S), xm (B,n), the identity
    ukf = regions(B * S * n, B * S * m, B * S * 2 * n, B * S, B * n, B * n * n)
    if B == 0:
        assert step == ukf == 256
    if B == 4096:  # profiles/ukf_probe.txt
        assert (step, ukf) == (491520, 2392064)
    assert eng.ekf_workspace_bytes(B) == step
    assert eng.dekf_workspace_bytes(B) == step
    assert eng.ukf_workspace_bytes(B) == ukf


def test_a_negative_batch_has_no_workspace():
    eng = engine("phnn_cartpole")
    assert eng.ekf_workspace_bytes(-1) == eng.dekf_workspace_bytes(-1) == eng.ukf_workspace_bytes(-1) == 0
