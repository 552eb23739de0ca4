"""K19 row_topk (top-k + log-sum-exp) vs the stable-sort oracle.

The oracle is ops/reference.py::row_topk: a stable descending sort
truncated to k (descending value, ties to the smallest column) plus
torch.logsumexp.  Indices and values must match it exactly; lse within
the 1e-4 relative bound test_kernels_gpu.py uses for the head's lse
partials.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R

NINF = float("-inf")


def relerr(a, b):
    a = a.detach().float()
    b = b.detach().float()
    d = (a - b).norm()
    n = b.norm()
    return float(d / n) if float(n) > 0 else float(d)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


_CASES = {}


def bf16_case(B, L, dev):
    """Seeded randn -> bf16 input and its k = 16 oracle, computed once per
    shape and shared (read-only) by every test that uses the shape."""
    key = (B, L)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * B + L)
        x = torch.randn(B, L, generator=g).to(torch.bfloat16).to(dev)
        _CASES[key] = (x,) + R.row_topk(x, min(16, L))
    return _CASES[key]


def check_against_oracle(x, k, oracle=None):
    vals, idx, lse = Fn.row_topk(x, k)
    rv, ri, rl = oracle if oracle is not None else R.row_topk(x, k)
    assert vals.dtype == torch.float32 and vals.shape == (x.shape[0], k)
    assert idx.dtype == torch.int64 and idx.shape == (x.shape[0], k)
    assert lse.dtype == torch.float32 and lse.shape == (x.shape[0],)
    assert torch.equal(idx, ri[:, :k])
    assert torch.equal(vals, rv[:, :k])
    err = relerr(lse, rl)
    print(f"lse relerr {tuple(x.shape)} k={k}: {err:.3e}")
    assert err < 1e-4
    return vals, idx, lse


# (33, 517): unaligned rows (scalar loads), one chunk; (64, 30000): one
# chunk, 16-B loads; (8, 261000): many chunks, tie-rich; (3, 16): k = L
@pytest.mark.parametrize("B,L", [(33, 517), (64, 30000), (8, 261000),
                                 (3, 16)])
def test_oracle_equality_k16(dev, B, L):
    x, rv, ri, rl = bf16_case(B, L, dev)
    check_against_oracle(x, 16, (rv, ri, rl))


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("B,L", [(33, 517), (8, 261000)])
def test_small_k(dev, B, L, k):
    x, rv, ri, rl = bf16_case(B, L, dev)
    check_against_oracle(x, k, (rv, ri, rl))


@pytest.mark.parametrize("B,L", [(33, 517), (8, 261000)])
def test_k1_agrees_with_row_max_argmax(dev, B, L):
    x = bf16_case(B, L, dev)[0]
    vals, idx, _ = Fn.row_topk(x, 1)
    mv, mi = Fn.row_max_argmax(x)
    assert torch.equal(vals[:, 0], mv)
    assert torch.equal(idx[:, 0], mi)


# the attention use: fp32 softmax rows; 200 takes 16-B loads, 203 scalar
@pytest.mark.parametrize("B,L", [(16, 200), (5, 203)])
@pytest.mark.parametrize("k", [5, 16])
def test_fp32_softmax_rows(dev, B, L, k):
    g = torch.Generator().manual_seed(B + L)
    x = torch.softmax(torch.randn(B, L, generator=g) * 3.0, dim=1).to(dev)
    assert x.dtype == torch.float32
    check_against_oracle(x, k)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ties_resolve_to_smallest_columns(dev, dtype):
    L, k = Fn.ROW_TOPK_CHUNK + 4096, 16  # two chunks
    x = torch.full((2, L), -2.0, dtype=dtype, device=dev)
    x[0] = 0.0  # all-zeros row
    g = torch.Generator().manual_seed(5)
    cols = torch.randperm(L, generator=g)[:20].to(dev)  # both chunks
    x[1, cols] = 3.5
    vals, idx, _ = check_against_oracle(x, k)
    assert torch.equal(idx[0], torch.arange(k, device=dev))
    assert torch.equal(idx[1], torch.sort(cols).values[:k])
    assert bool((vals[1] == 3.5).all())


# 3*CHUNK + 5 has unaligned rows (scalar loads); + 8 keeps 16-B loads
@pytest.mark.parametrize("extra", [5, 8])
def test_chunk_boundaries(dev, extra):
    CH = Fn.ROW_TOPK_CHUNK
    L = 3 * CH + extra
    x = torch.full((2, L), -1.0, dtype=torch.bfloat16, device=dev)
    cols = [0, CH - 1, CH, 2 * CH - 1, 2 * CH, L - 1]
    big = [10.0, 60.0, 20.0, 50.0, 30.0, 40.0]  # distinct, exact in bf16
    for c, v in zip(cols, big):
        x[0, c] = v
        x[1, c] = 100.0 - v
    vals, idx, _ = check_against_oracle(x, 6)
    order0 = sorted(range(6), key=lambda i: -big[i])
    order1 = sorted(range(6), key=lambda i: big[i])
    assert idx[0].tolist() == [cols[i] for i in order0]
    assert vals[0].tolist() == [big[i] for i in order0]
    assert idx[1].tolist() == [cols[i] for i in order1]
    check_against_oracle(x, 16)


@pytest.mark.parametrize("L", [517, Fn.ROW_TOPK_CHUNK + 1000])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_neg_inf_rows(dev, L, dtype):
    # 517: one chunk, scalar loads; CHUNK + 1000: two chunks, 16-B loads,
    # the second chunk all -inf in both rows
    k = 16
    x = torch.full((2, L), NINF, dtype=dtype, device=dev)
    x[0, 301] = 2.5  # single finite entry; row 1 stays all -inf
    vals, idx, lse = Fn.row_topk(x, k)
    assert not torch.isnan(vals).any() and not torch.isnan(lse).any()
    # finite entry first, then -inf columns in index order (301 > k)
    assert idx[0].tolist() == [301] + list(range(k - 1))
    assert vals[0].tolist() == [2.5] + [NINF] * (k - 1)
    assert float(lse[0]) == 2.5
    assert torch.equal(idx[1], torch.arange(k, device=dev))
    assert bool((vals[1] == NINF).all())
    assert float(lse[1]) == NINF


# (8, 261000) adds stage 2 and the waves' shared pre-filter, whose timing
# varies run to run while the result must not
@pytest.mark.parametrize("B,L", [(64, 30000), (8, 261000)])
def test_bitwise_deterministic(dev, B, L):
    x = bf16_case(B, L, dev)[0]
    a = Fn.row_topk(x, 16)
    b = Fn.row_topk(x, 16)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))


def test_hipgraph_capture_replay(dev):
    x = bf16_case(64, 30000, dev)[0]
    static = x.clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        Fn.row_topk(static, 16)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = Fn.row_topk(static, 16)
    g = torch.Generator().manual_seed(77)
    fresh = torch.randn(64, 30000, generator=g).to(torch.bfloat16).to(dev)
    static.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    eager = Fn.row_topk(fresh, 16)
    for u, v in zip(out, eager):
        assert torch.equal(u, v)
    assert not torch.equal(out[1], bf16_case(64, 30000, dev)[2])


def test_argument_errors(dev):
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    for k in (0, 17):
        with pytest.raises((ValueError, RuntimeError)):
            Fn.row_topk(x, k)
    with pytest.raises((ValueError, RuntimeError)):
        Fn.row_topk(x[:, :8].contiguous(), 9)  # k > L
    with pytest.raises((ValueError, RuntimeError)):
        Fn.row_topk(x.t(), 2)  # non-contiguous
    with pytest.raises((ValueError, RuntimeError)):
        Fn.row_topk(x[:, ::2], 2)  # non-contiguous
