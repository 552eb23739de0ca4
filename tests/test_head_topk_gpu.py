"""K23 head_topk (fused head + top-k + log-sum-exp) on the GPU.

The four-point rule of test_sim_topk_gpu.py against fp64 logits
Z = scale * q.double() @ w.double().T + bias of the bf16 inputs as stored,
no element excluded.  For every query i:
  1. indices in [0, L) and distinct;
  2. |vals[j] - Z[i, idx[j]]| <= tol_z[i, idx[j]];
  3. vals non-increasing, equal values with ascending labels;
  4. |vals[j] - sortdesc(Z[i])[j]| <= max_l tol_z[i, l] (the j-th largest of
     perturbed values moves by at most the largest perturbation).

Bounds (derived, none fitted):
  tol_z[i, l] = (EP + 2) * 2^-23 * (scale * sum_e |q_ie||w_le| + |bias_l|)
    head_numerics.py's "products of exact bf16 inputs" form for an fp32
    output: EP - 1 additions of the MFMA chain, one fma with the scale and
    the bias, u doubled to 2^-23 to cover a truncating adder.
  lse: (n_chain + 64) * 2^-24 + 2^-17 + 2^-22 |ref| + logit term
    head_numerics.py's lse line with the logits' own error added.  lse is
    1-Lipschitz in the sup norm, so max_l tol_z[i, l] over the labels that
    carry weight bounds that term; the test uses its exact form
    log(sum_l p_l exp(tol_z[i, l])), p = softmax(Z[i]) (head_topk_rule.py),
    which weighs every label's tolerance by the weight it carries and never
    exceeds that maximum: a planted row that belongs to another query does
    not widen this query's bound.  n_chain is the longest serial fp32 chain
    of positive terms: a lane adds 4 labels per tile over ceil(tps / 4)
    tiles of its slice (tps = tiles per slice), then 2 DPP-row merges and 3
    wave merges; with nsplit > 1 stage 2 adds ceil(nsplit / 256) slice
    merges, 6 shuffle merges and 3 wave merges.  The composed path's chain
    is K19's: 32768 / 256 = 128 elements per thread plus the same merges
    (160 covers it).

Planted spikes (logit about 30, at least 20 above the rest of the row, whose
maximum is about 7) sit on labels 0, 15, 16, slice_rows - 1, slice_rows,
L - 16, L - 1 of queries 0, 15, 16, nq - 1 in turn; the other queries carry
none, so a dropped slice moves their lse visibly.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from head_topk_rule import (K19_CHAIN, check_rule, lse_bound, lse_logit_tol,
                            n_chain)

from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def planted_labels(L, rows):
    want = [0, 15, 16, rows - 1, rows, L - 16, L - 1]
    return sorted({l for l in want if 0 <= l < L})


_CASES = {}


def make_case(nq, L, EP, mode, dev, rows=None, ref=True):
    """mode "bias": random q, w, bias, scale 1.  mode "cos": unit rows, no
    bias, scale 30.  Returns a dict with the device tensors and the fp64
    logits, tolerances and lse of the stored bf16 values; computed once per
    key, shared read-only."""
    rows = rows or Fn.head_topk_slice_rows(
        L, Fn.head_topk_default_nsplit(L, EP))
    key = (nq, L, EP, mode, rows)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000003 * nq + 31 * L + EP
                                      + (mode == "cos"))
    h = EP // 2
    if mode == "bias":
        q = 0.3 * torch.randn(nq, EP, generator=g)
        w = 0.3 * torch.randn(L, EP, generator=g)
        bias = torch.randn(L, generator=g)
        scale = 1.0
    else:
        # queries live in the first half of the columns and the labels
        # mostly in the second, so random cosines stay small (30 * cos has
        # a standard deviation of about 1) and a planted cos = 1 stands out
        q = torch.randn(nq, EP, generator=g)
        q[:, h:] = 0
        w = torch.randn(L, EP, generator=g)
        w[:, :h] *= 0.3
        q = q / q.norm(dim=1, keepdim=True)
        w = w / w.norm(dim=1, keepdim=True)
        bias = None
        scale = 30.0
    q = q.to(torch.bfloat16)
    labels = planted_labels(L, rows)
    qs = [x for x in dict.fromkeys([0, 15, 16, nq - 1]) if x < nq]
    plants = []
    for i, l in enumerate(labels):
        qi = qs[i % len(qs)]
        qv = q[qi].float()
        if mode == "bias":
            w[l] = qv * (30.0 / float(qv @ qv))
            bias[l] = 0.0
        else:
            w[l] = qv / qv.norm()
        plants.append((qi, l))
    w = w.to(torch.bfloat16)
    if not ref:  # inputs only (the bitwise tests need no fp64 logits)
        case = dict(q=q.to(dev), w=w.to(dev),
                    bias=None if bias is None else bias.to(dev), scale=scale)
        _CASES[key] = case
        return case
    qd, wd = q.double(), w.double()
    Z = scale * (qd @ wd.t())
    mag = scale * (qd.abs() @ wd.abs().t())
    if bias is not None:
        Z = Z + bias.double()
        mag = mag + bias.double().abs()
    tol = (EP + 2) * 2.0 ** -23 * mag
    case = dict(q=q.to(dev), w=w.to(dev),
                bias=None if bias is None else bias.to(dev), scale=scale,
                Z=Z, tol=tol, lse=torch.logsumexp(Z, dim=1), plants=plants,
                spiked={qi for qi, _ in plants})
    _CASES[key] = case
    return case


def slices_L(EP=128):
    # two default-width slices and nine labels
    return 2 * Fn._HEAD_TOPK_SLICE_TILES * Fn.SIM_ROW_TILE + 9


# (nq, L, EP, k, nsplit); L = None: slices_L()
RULE_SHAPES = [
    (1, 16, 128, 16, None),       # one tile, k == L
    (37, 1000, 128, 16, None),    # query tail and label tail
    (5, 533, 320, 3, None),       # generic EP, L odd
    (17, None, 128, 10, None),    # slices, default
    (17, None, 128, 10, 1),
    (17, None, 128, 10, 3),
    (64, 20011, 128, 10, None),
    (8, 131080, 128, 16, None),   # L past 2^17
]


@pytest.mark.parametrize("mode", ["bias", "cos"])
@pytest.mark.parametrize("nq,L,EP,k,nsplit", RULE_SHAPES)
def test_tolerance_rule(dev, nq, L, EP, k, nsplit, mode):
    L = L or slices_L()
    ns = nsplit or Fn.head_topk_default_nsplit(L, EP)
    if L == slices_L() and nsplit is None:
        assert ns == 2
    c = make_case(nq, L, EP, mode, dev, rows=Fn.head_topk_slice_rows(L, ns))
    vals, idx, lse = Fn.head_topk(c["q"], c["w"], k, c["bias"], c["scale"],
                                  nsplit=nsplit)
    check_rule(vals, idx, lse, c, k, n_chain(L, ns),
               tag=f"{mode} EP={EP} nsplit={ns}")


def int_case(nq, L, EP, dev, seed=0):
    g = torch.Generator().manual_seed(seed + nq + L + EP)
    q = torch.randint(-3, 4, (nq, EP), generator=g).to(torch.bfloat16)
    w = torch.randint(-3, 4, (L, EP), generator=g).to(torch.bfloat16)
    bias = torch.randint(-8, 9, (L,), generator=g).float()
    return q.to(dev), w.to(dev), bias.to(dev)


@pytest.mark.parametrize("nq,L,EP,k,scale", [
    (37, 1000, 128, 16, 2.0), (33, 4099, 128, 10, 0.5),
    (5, 533, 320, 5, 1.0), (20, 300, 512, 7, 4.0), (3, 16, 32, 16, 0.25)])
def test_integer_data_equals_oracle(dev, nq, L, EP, k, scale):
    """Entries in [-3, 3], integer bias, power-of-two scale: every logit is
    exact in fp32 (|sum| <= 9 * 512), so vals and idx equal the oracle bit
    for bit whatever the slicing; lse stays within its bound."""
    q, w, bias = int_case(nq, L, EP, dev)
    rv, ri, _ = R.head_topk(q.cpu(), w.cpu(), k, bias.cpu(), scale)
    Z = scale * (q.cpu().double() @ w.cpu().double().t()) + bias.cpu().double()
    ref = torch.logsumexp(Z, dim=1)
    for nsplit in (None, 1, 2, 5):
        vals, idx, lse = Fn.head_topk(q, w, k, bias, scale, nsplit=nsplit)
        assert torch.equal(idx.cpu(), ri)
        assert torch.equal(vals.cpu(), rv)
        ns = nsplit or Fn.head_topk_default_nsplit(L, EP)
        lb = lse_bound(ref, torch.zeros_like(ref), n_chain(L, ns))
        assert bool(((lse.cpu().double() - ref).abs() <= lb).all())


@pytest.mark.parametrize("EP", [128, 96])
def test_duplicates_across_slice_boundaries(dev, EP):
    L, nsplit = 1000, 3
    rows = Fn.head_topk_slice_rows(L, nsplit)
    assert rows % Fn.SIM_ROW_TILE == 0 and 2 * rows < L <= 3 * rows
    q, w, bias = int_case(2, L, EP, dev, seed=9)
    planted = [0, rows - 1, rows, 2 * rows - 1, 2 * rows, L - 1]
    w[planted] = 3.0  # the best possible partner of an all-3 query
    bias[planted] = 8.0
    q[0] = 3.0
    q[1] = -3.0
    vals, idx, _ = Fn.head_topk(q, w, len(planted), bias, nsplit=nsplit)
    assert idx[0].tolist() == planted
    assert vals[0].tolist() == [9.0 * EP + 8.0] * len(planted)
    rv, ri, _ = R.head_topk(q.cpu(), w.cpu(), 16, bias.cpu())
    vals, idx, _ = Fn.head_topk(q, w, 16, bias, nsplit=nsplit)
    assert torch.equal(idx.cpu(), ri) and torch.equal(vals.cpu(), rv)


@pytest.mark.parametrize("EP", [128, 64])
def test_identical_rows_return_arange(dev, EP):
    L, k = 5000, 16
    row = torch.randint(-3, 4, (EP,),
                        generator=torch.Generator().manual_seed(1))
    w = row.to(torch.bfloat16).repeat(L, 1).contiguous().to(dev)
    q = w[:3].contiguous()
    for nsplit in (None, 1, 5):
        vals, idx, lse = Fn.head_topk(q, w, k, nsplit=nsplit)
        assert torch.equal(idx, torch.arange(k, device=dev).repeat(3, 1))
        z = float((row * row).sum())
        assert bool((vals == z).all())
        assert float((lse - (z + math.log(L))).abs().max()) <= 1e-3


@pytest.mark.parametrize("nq,L,EP,mode", [
    (37, 1000, 128, "bias"), (5, 533, 320, "cos"), (17, None, 128, "bias")])
def test_nsplit_changes_no_vals_or_idx_bits(dev, nq, L, EP, mode):
    L = L or slices_L()
    c = make_case(nq, L, EP, mode, dev)
    k = 10
    base = Fn.head_topk(c["q"], c["w"], k, c["bias"], c["scale"], nsplit=1)
    ltol = lse_logit_tol(c["Z"], c["tol"])
    for nsplit in (1, 2, 3, 7):
        got = Fn.head_topk(c["q"], c["w"], k, c["bias"], c["scale"],
                           nsplit=nsplit)
        assert torch.equal(got[0].view(torch.int32),
                           base[0].view(torch.int32))
        assert torch.equal(got[1], base[1])
        lb = lse_bound(c["lse"], ltol, n_chain(L, nsplit))
        assert bool(((got[2].cpu().double() - c["lse"]).abs() <= lb).all())


@pytest.mark.parametrize("L,mode", [(1000, "bias"), (20011, "bias"),
                                    (20011, "cos")])
def test_batch_independence(dev, L, mode):
    """With the default nsplit a query's (vals, idx, lse) bits are the same
    alone, at positions 0, 15, 16 and last of a 37-query batch, and inside a
    1,024-query batch."""
    EP, k = 128, 10
    c = make_case(1024, L, EP, mode, dev, ref=False)
    q, w, bias, scale = c["q"], c["w"], c["bias"], c["scale"]
    big = Fn.head_topk(q, w, k, bias, scale)
    for row in (0, 517, 1023):
        alone = Fn.head_topk(q[row:row + 1].contiguous(), w, k, bias, scale)
        for pos in (0, 15, 16, 36):
            batch = q[100:137].clone()
            batch[pos] = q[row]
            got = Fn.head_topk(batch, w, k, bias, scale)
            for a, b in zip(alone, got):
                assert torch.equal(a[0].view(torch.int32).flatten(),
                                   b[pos].view(torch.int32).flatten())
        for a, b in zip(alone, big):
            assert torch.equal(a[0].view(torch.int32).flatten(),
                               b[row].view(torch.int32).flatten())


def test_run_to_run_bits_into_nan_filled_outputs(dev):
    c = make_case(64, 20011, 128, "bias", dev)
    nq, L, k = 64, 20011, 16
    nsplit = Fn.head_topk_default_nsplit(L, 128)
    assert nsplit > 1
    outs = []
    for _ in range(2):
        vals = torch.full((nq, k), float("nan"), device=dev)
        idx = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
        lse = torch.full((nq,), float("nan"), device=dev)
        part = torch.full((nq, nsplit, 16), -1, dtype=torch.int64,
                          device=dev)
        pm = torch.full((nq, nsplit), float("nan"), device=dev)
        ps = torch.full((nq, nsplit), float("nan"), device=dev)
        Fn.ext().head_topk(c["q"], c["w"], c["bias"], 1.0, k, nsplit,
                           Fn.SIM_QUERY_TILE, Fn.SIM_ROW_TILE, part, pm, ps,
                           vals, idx, lse)
        outs.append((vals, idx, lse))
    (v0, i0, l0), (v1, i1, l1) = outs
    assert not bool(torch.isnan(v0).any()) and not bool(torch.isnan(l0).any())
    assert bool((i0 >= 0).all())
    assert torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    assert torch.equal(i0, i1)
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))


def test_hipgraph_capture_replay(dev):
    c = make_case(64, 20011, 128, "bias", dev)
    sq, sw, sb = c["q"].clone(), c["w"].clone(), c["bias"].clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        Fn.head_topk(sq, sw, 16, sb)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = Fn.head_topk(sq, sw, 16, sb)
    g = torch.Generator().manual_seed(77)
    fq = torch.randn(64, 128, generator=g).to(torch.bfloat16).to(dev)
    fw = torch.randn(20011, 128, generator=g).to(torch.bfloat16).to(dev)
    fb = torch.randn(20011, generator=g).to(dev)
    sq.copy_(fq)
    sw.copy_(fw)
    sb.copy_(fb)
    graph.replay()
    torch.cuda.synchronize()
    eager = Fn.head_topk(fq, fw, 16, fb)
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    assert not torch.equal(out[1], Fn.head_topk(c["q"], c["w"], 16,
                                                c["bias"])[1])


@pytest.mark.parametrize("nq,L,EP,k,mode", [(37, 1000, 128, 16, "bias"),
                                            (5, 533, 320, 3, "cos")])
def test_fused_and_composed_pass_the_same_rule(dev, nq, L, EP, k, mode,
                                               monkeypatch):
    c = make_case(nq, L, EP, mode, dev)
    args = (c["q"], c["w"], k, c["bias"], c["scale"])
    ns = Fn.head_topk_default_nsplit(L, EP)
    check_rule(*Fn.head_topk(*args), c, k, n_chain(L, ns), tag="fused")
    comp = Fn.head_topk_composed(*args)
    check_rule(*comp, c, k, K19_CHAIN, tag="composed")
    # C2V_HEAD_TOPK_FUSED=0 routes the public op to the composed path
    monkeypatch.setattr(Fn, "_HEAD_TOPK_FUSED", False)
    routed = Fn.head_topk(*args)
    for a, b in zip(routed, comp):
        assert torch.equal(a, b)


@pytest.mark.parametrize("nsplit", [1, 4])
def test_masked_labels(dev, nsplit):
    """-inf bias entries are never returned while finite labels remain and
    add nothing to lse, also when they fill a whole slice."""
    nq, L, EP, k = 5, 1000, 128, 16
    q, w, bias = int_case(nq, L, EP, dev, seed=4)
    rows = Fn.head_topk_slice_rows(L, 4)
    masked = torch.zeros(L, dtype=torch.bool)
    masked[rows:2 * rows] = True  # slice 1 of 4 entirely
    masked[[0, 7, L - 1]] = True
    bias[masked.to(dev)] = float("-inf")
    vals, idx, lse = Fn.head_topk(q, w, k, bias, nsplit=nsplit)
    assert not bool(masked[idx.cpu()].any())
    rv, ri, _ = R.head_topk(q.cpu(), w.cpu(), k, bias.cpu())
    assert torch.equal(idx.cpu(), ri) and torch.equal(vals.cpu(), rv)
    Z = q.cpu().double() @ w.cpu().double().t() + bias.cpu().double()
    ref = torch.logsumexp(Z[:, ~masked], dim=1)
    lb = lse_bound(ref, torch.zeros_like(ref), n_chain(L, nsplit))
    assert bool(((lse.cpu().double() - ref).abs() <= lb).all())
    # everything masked: lse is -inf, not NaN, and the labels come in order
    bias[:] = float("-inf")
    vals, idx, lse = Fn.head_topk(q, w, 3, bias, nsplit=nsplit)
    assert bool((lse == float("-inf")).all())
    assert bool((vals == float("-inf")).all())
    assert idx[0].tolist() == [0, 1, 2]


def test_empty_batch(dev):
    w = torch.zeros(32, 64, dtype=torch.bfloat16, device=dev)
    q = torch.zeros(0, 64, dtype=torch.bfloat16, device=dev)
    vals, idx, lse = Fn.head_topk(q, w, 4)
    assert vals.shape == (0, 4) and idx.shape == (0, 4) and lse.shape == (0,)


def test_argument_and_device_errors(dev):
    q = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(32, 64, dtype=torch.bfloat16, device=dev)
    bias = torch.zeros(32, device=dev)
    err = ValueError  # the contract's own checks, never the binding's
    for k in (0, 17):
        with pytest.raises(err):
            Fn.head_topk(q, w, k)
    with pytest.raises(err):
        Fn.head_topk(q, w[:8].contiguous(), 9)  # k > L
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(err):
            Fn.head_topk(q, w, 2, scale=scale)
    with pytest.raises(err):
        Fn.head_topk(q.float(), w.float(), 2)  # fp32 on the device
    with pytest.raises(err):
        Fn.head_topk(q[:, :32], w[:, :32].contiguous(), 2)  # non-contiguous
    with pytest.raises(err):
        Fn.head_topk(q, w[::2], 2)  # non-contiguous
    with pytest.raises(err):
        Fn.head_topk(q, w[:, :32].contiguous(), 2)  # mismatched EP
    with pytest.raises(err):
        Fn.head_topk(q[:, :48].contiguous(), w[:, :48].contiguous(), 2)
    with pytest.raises(err):
        Fn.head_topk(q, w, 2, bias[:31])  # one bias per label
    with pytest.raises(err):
        Fn.head_topk(q, w, 2, bias.double())
    with pytest.raises(err):
        Fn.head_topk(q, w, 2, bias.cpu())  # bias on another device
    with pytest.raises(err):
        Fn.head_topk(q, w, 2, nsplit=0)
    with pytest.raises(err):
        Fn.head_topk_composed(q.float(), w.float(), 2)
