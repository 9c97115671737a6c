"""Host side of the full-catalogue top-K / full-ranking path (ops.full_topk, the c2dsr_full_topk_* queries): argument
checks that must come before any device call, and the workspace contract (O(M · k · n_split), independent of n).
No GPU: tests/test_gpu_fullrank.py holds the compute."""
import pytest
import torch

from c2dsr_amd import ops
from c2dsr_amd._lib import HipLibError, lib


def _qwb(M=4, n=100, d=16):
    return torch.zeros(M, d), torch.zeros(n, d), torch.zeros(n)


@pytest.mark.parametrize('k', [0, -1, 129, 101])
def test_full_topk_refuses_bad_k(k):
    q, W, b = _qwb()  # host tensors: a ValueError here shows the check ran before any device call
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, k)


def test_full_topk_refuses_wide_and_mismatched_shapes():
    q, W, b = _qwb(d=257)
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, 5)
    q, W, b = _qwb()
    with pytest.raises(ValueError):
        ops.full_topk(q, torch.zeros(100, 17), b, 5)
    with pytest.raises(ValueError):
        ops.full_topk(q, W, torch.zeros(99), 5)
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, 5, target=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, 5, exclude=torch.zeros(3, 7, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, 5, dom=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, 5, dom=torch.zeros(4, dtype=torch.int64), which=2)
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, 5, n_split=0)
    with pytest.raises(ValueError):
        ops.full_topk(q, W, b, 5, out=(torch.zeros(4, 4, dtype=torch.int64), torch.zeros(4, 5), None))


def test_full_topk_and_eval_query_refuse_host_tensors():
    q, W, b = _qwb()
    with pytest.raises(HipLibError, match='HIP device'):
        ops.full_topk(q, W, b, 5)
    h = torch.zeros(4, 8, 16)
    i = torch.zeros(4, 1, dtype=torch.int64)
    with pytest.raises(HipLibError, match='HIP device'):
        ops.eval_query(h, h, h, i, i, i)


def test_workspace_is_independent_of_n_and_grows_with_the_rest():
    ws = lib.raw('c2dsr_full_topk_workspace')
    for M, k, s in ((1, 1, 1), (300, 20, 3), (2048, 128, 16)):
        assert int(ws(M, 1000, k, s)) == int(ws(M, 10_000_000, k, s)) > 0
    base = int(ws(300, 1000, 20, 3))
    assert int(ws(3000, 1000, 20, 3)) > base
    assert int(ws(300, 1000, 100, 3)) > base
    assert int(ws(300, 1000, 20, 6)) > base
    assert int(ws(300, 1000, 129, 3)) == 0 and int(ws(300, 10, 20, 3)) == 0  # k > 128, k > n: refused


def test_supported_widths():
    sup = lib.raw('c2dsr_full_topk_supported')
    assert [int(sup(d)) for d in (64, 128, 256)] == [1, 1, 1]
    assert int(sup(30)) == 0 and int(sup(512)) == 0
