"""Pipelined head backward (head_bwd_dw_pipe, head_bwd_dcv_pipe) and
pipelined split-K wgrad (wgrad_pipe) against the kernels they replace.

The pipelined kernels run the same arithmetic in the same order, so every
check is bitwise (torch.equal) at the extension level on the same buffers;
accuracy against fp64 is test_head_numerics_gpu.py's job.  Shapes are the
smallest at which a pipeline can go wrong: fewer stages than the depth,
exactly the depth, a ragged last stage, partial label blocks and slabs.

Clamped loads must not leak: the logits are a contiguous [B, L] view into
a larger NaN-filled buffer (NaN in front of and behind the view), and the
fragment images, scratch and outputs are NaN-filled before each run.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import ext

# head_bwd_dw_pipe as shipped (HB_DW_DEPTH in head_bwd.hip): a stage is
# DW_SUB 64-row sub-stages and two stages are prefetched, so DW_DEPTH
# 64-row sub-stages of logits are in flight per thread
DW_SUB = 2
DW_DEPTH = 2 * DW_SUB
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def stop_after_gpu_fault():
    """A HIP error is sticky: nothing more is launched after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def _head_inputs(B, L, weighted, dev, seed):
    """logits as a [B, L] view inside a NaN buffer, labels that hit the
    first chunk and the last 8 columns, and the packed per-row
    (coef, lse, y) from head_bwd_prep."""
    g = torch.Generator().manual_seed(seed)
    off, pad = 64, 4096  # multiples of 8 elements
    store = torch.full((off + B * L + pad,), NAN, dtype=torch.bfloat16,
                       device=dev)
    vals = (torch.randn(B, L, generator=g) * 3.0).to(torch.bfloat16)
    logits = store[off:off + B * L].view(B, L)
    logits.copy_(vals.to(dev))
    assert logits.is_contiguous() and logits.data_ptr() % 16 == 0
    label = torch.randint(0, L, (B,), generator=g)
    label[0] = min(3, L - 1)        # first 8-label chunk
    label[-1] = L - 1 - (seed % 8)  # last 8 columns
    label = label.to(dev)
    lse = torch.logsumexp(logits.float(), dim=1).contiguous()
    if weighted:
        weight = (torch.rand(L, generator=g) + 0.5).to(dev)
        wsum = weight[label].sum()
    else:
        weight = torch.empty(0, device=dev)
        wsum = torch.tensor(float(B), device=dev)
    acc = torch.stack([torch.zeros((), device=dev), wsum.float()])
    gscale = torch.full((1,), 0.75, device=dev)
    coef_lse = torch.full((B, 4), NAN, device=dev)
    ext().head_bwd_prep(label, weight, acc, gscale, lse, coef_lse)
    return g, logits, coef_lse, store


def _image(x, nchunk, dev):
    img = torch.full((nchunk, 8, 64, 8), NAN, dtype=torch.bfloat16,
                     device=dev)
    ext().swizzle_cv(x, img)
    return img


# fewer rows than one sub-stage / one stage / the prefetch depth, exactly
# those, and ragged last (sub-)stages past each; odd and even stage counts
DW_B = sorted({8, 64, 72} | {64 * d + r for d in (DW_SUB, DW_DEPTH)
                             for r in (0, 8)}
              | {64 * (d + 1) + 8 for d in (DW_SUB, DW_DEPTH)})
DW_L = [8, 72, 1096]  # one partial block; 1096 = 17*64 + 8: 8-label tail


@pytest.mark.parametrize("L", DW_L)
@pytest.mark.parametrize("B", DW_B)
def test_dw_pipe_matches_bitwise(dev, B, L):
    for weighted in (True, False):
        g, logits, coef_lse, _store = _head_inputs(
            B, L, weighted, dev, seed=B * 7 + L + weighted)
        cv = (torch.randn(B, 128, generator=g) * 0.5).to(torch.bfloat16)
        cvimg = _image(cv.to(dev), (B + 63) // 64 * 2, dev)

        def run(fn):
            dw = torch.full((L, 128), NAN, dtype=torch.bfloat16, device=dev)
            dbias = torch.full((L,), NAN, device=dev)
            fn(dw, dbias)
            return dw, dbias

        dw0, db0 = run(lambda dw, db: ext().head_bwd_dw(
            logits, cvimg, coef_lse, dw, db))
        assert bool(torch.isfinite(dw0.float()).all())
        assert bool(torch.isfinite(db0).all())
        # 0 = the shipped depth; the other instantiations ship as sweep knobs
        for depth in (0, 0, 1, 2):
            dw1, db1 = run(lambda dw, db: ext().head_bwd_dw_pipe(
                logits, cvimg, coef_lse, dw, db, depth))
            assert not bool(torch.isnan(dw1.float()).any()), depth
            assert not bool(torch.isnan(db1).any()), depth
            assert torch.equal(dw1, dw0), (depth, weighted)
            assert torch.equal(db1, db0), (depth, weighted)


DCV_B = [8, 16, 136]       # 136: GYB = 2 and a wave with 8 valid rows
DCV_L = [8, 136, 1096]     # 1096 with chunk 1024: a second slab of 72 labels
DCV_CHUNK = [128, 512, 1024]


@pytest.mark.parametrize("chunk", DCV_CHUNK)
@pytest.mark.parametrize("L", DCV_L)
@pytest.mark.parametrize("B", DCV_B)
def test_dcv_pipe_matches_bitwise(dev, B, L, chunk):
    g, logits, coef_lse, _store = _head_inputs(
        B, L, True, dev, seed=B * 11 + L + chunk)
    w = (torch.randn(L, 128, generator=g) * 0.2).to(torch.bfloat16)
    wimg = _image(w.to(dev), (L + 127) // 128 * 4, dev)
    split = (L + chunk - 1) // chunk

    def run(fn):
        partials = torch.full((split, B, 128), NAN, device=dev)
        fn(partials)
        dcv = torch.full((B, 128), NAN, dtype=torch.bfloat16, device=dev)
        ext().slab_sum_bf16(partials, dcv)
        return partials, dcv

    p0, d0 = run(lambda p: ext().head_bwd_dcv(
        logits, wimg, coef_lse, p, chunk))
    assert bool(torch.isfinite(p0).all())
    # -1 = the default buffering, called twice (run to run); 0 / 1 = the
    # single- and double-buffered instantiations
    for dbuf in (-1, -1, 0, 1):
        p1, d1 = run(lambda p: ext().head_bwd_dcv_pipe(
            logits, wimg, coef_lse, p, chunk, dbuf))
        assert not bool(torch.isnan(p1).any()), dbuf
        assert not bool(torch.isnan(d1.float()).any()), dbuf
        assert torch.equal(p1, p0), dbuf
        assert torch.equal(d1, d0), dbuf


# S = 4 slabs: blocks with 0, 1, 2 and 3+ K-steps, a ragged last step and
# idle trailing blocks
WG_M = [8, 40, 100, 136, 264, 400]


@pytest.mark.parametrize("KP", [32, 320])
@pytest.mark.parametrize("M", WG_M)
def test_wgrad_pipe_matches_bitwise(dev, M, KP):
    g = torch.Generator().manual_seed(M * 3 + KP)
    EP, S = 128, 4
    x = torch.randn(M, KP, generator=g).to(torch.bfloat16).to(dev)
    dz = (torch.randn(M, EP, generator=g) * 0.3).to(torch.bfloat16).to(dev)

    def run(fn):
        partials = torch.full((S, KP, EP), NAN, device=dev)
        fn(partials)
        return partials

    p0 = run(lambda p: ext().wgrad(x, dz, p))
    assert bool(torch.isfinite(p0).all())
    for _ in range(2):  # run to run
        p1 = run(lambda p: ext().wgrad_pipe(x, dz, p, 0))
        assert not bool(torch.isnan(p1).any())
        assert torch.equal(p1, p0)
