"""K23 on the CPU: the head_topk oracle and its argument contract, the
models' encode + head_topk against forward, and Predictor(fused_head=True)
on the torch backend."""

import pytest
import torch
import torch.nn.functional as F

from code2vec_amd.data.reader import CorpusReader
from code2vec_amd.engine.predict import Predictor
from code2vec_amd.models.code2vec import Code2VecTorch, init_logical_params
from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R
from code2vec_amd.utils.options import Option


def rand_case(nq, L, EP, seed=0, bias=True):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(nq, EP, generator=g)
    w = torch.randn(L, EP, generator=g)
    b = torch.randn(L, generator=g) if bias else None
    return q, w, b


@pytest.mark.parametrize("nq,L,EP,k,scale,bias", [
    (3, 16, 32, 16, 1.0, True), (7, 301, 64, 10, 2.5, True),
    (5, 533, 96, 3, 30.0, False), (1, 40, 128, 1, 0.5, True)])
def test_oracle_against_fp64_sort_and_logsumexp(nq, L, EP, k, scale, bias):
    q, w, b = rand_case(nq, L, EP, seed=L, bias=bias)
    vals, idx, lse = R.head_topk(q, w, k, b, scale)
    assert vals.dtype == torch.float32 and vals.shape == (nq, k)
    assert idx.dtype == torch.int64 and lse.shape == (nq,)
    Z = scale * (q.double() @ w.double().t())
    if b is not None:
        Z = Z + b.double()
    sv, si = torch.sort(Z, dim=1, descending=True, stable=True)
    assert torch.equal(idx, si[:, :k])  # random data: no near ties at 1e-5
    assert torch.allclose(vals.double(), sv[:, :k], atol=1e-4, rtol=1e-6)
    assert torch.allclose(lse.double(), torch.logsumexp(Z, 1), atol=1e-4,
                          rtol=1e-6)
    # the public op on CPU tensors is the oracle
    for a, c in zip(Fn.head_topk(q, w, k, b, scale), (vals, idx, lse)):
        assert torch.equal(a, c)
    for a, c in zip(Fn.head_topk_composed(q, w, k, b, scale),
                    (vals, idx, lse)):
        assert torch.allclose(a.double(), c.double(), atol=1e-4)


def test_tie_order_identical_rows_return_arange():
    w = torch.ones(50, 32) * 0.5
    q = torch.ones(2, 32)
    vals, idx, lse = R.head_topk(q, w, 16)
    assert torch.equal(idx, torch.arange(16).repeat(2, 1))
    assert bool((vals == 16.0).all())


def test_argument_errors_one_by_one():
    q, w, b = rand_case(4, 40, 64)
    R.check_head_topk_args(q, w, 5, b, 1.0)
    bad = [
        (q[0], w, 2, None, 1.0),                  # q not 2-D
        (q, w[0], 2, None, 1.0),                  # w not 2-D
        (q, w[:, :32], 2, None, 1.0),             # EP differs
        (q[:, :48], w[:, :48], 2, None, 1.0),     # EP no multiple of 32
        (torch.zeros(2, 544), torch.zeros(9, 544), 2, None, 1.0),  # EP > 512
        (q, w, 0, None, 1.0),
        (q, w, 17, None, 1.0),
        (q, w[:8], 9, None, 1.0),                 # k > L
        (q, w, 2, b[:39], 1.0),                   # bias length
        (q, w, 2, b.double(), 1.0),               # bias dtype
        (q, w, 2, b.view(1, -1), 1.0),            # bias not 1-D
        (q, w, 2, b, 0.0),
        (q, w, 2, b, -2.0),
        (q, w, 2, b, float("inf")),
        (q, w, 2, b, float("nan")),
    ]
    for args in bad:
        with pytest.raises(ValueError, match="head_topk"):
            R.check_head_topk_args(*args)
        with pytest.raises(ValueError, match="head_topk"):
            Fn.head_topk(*args)


def test_bias_changes_the_winner():
    q, w, _ = rand_case(6, 100, 32, seed=3, bias=False)
    dots = q @ w.t()
    bias = torch.zeros(100)
    worst = int(dots[0].argmin())
    bias[worst] = float(dots[0].max() - dots[0].min()) + 5.0
    _, idx, _ = R.head_topk(q, w, 3, bias)
    assert int(idx[0, 0]) == worst
    _, idx0, _ = R.head_topk(q, w, 3, None)
    assert int(idx0[0, 0]) == int(dots[0].argmax()) != worst


def test_scale_keeps_ranks_and_moves_vals_and_lse():
    q, w, _ = rand_case(5, 200, 64, seed=5, bias=False)
    v1, i1, l1 = R.head_topk(q, w, 10, None, 1.0)
    v4, i4, l4 = R.head_topk(q, w, 10, None, 4.0)
    assert torch.equal(i1, i4)
    assert torch.allclose(v4, 4.0 * v1, rtol=1e-6)
    Z = q @ w.t()
    assert torch.allclose(l4, torch.logsumexp(4.0 * Z, 1), rtol=1e-6)
    assert not torch.allclose(l4, l1)


def test_minus_inf_bias_masks_a_label():
    q, w, b = rand_case(4, 60, 32, seed=8)
    masked = [0, 17, 59]
    b[masked] = float("-inf")
    vals, idx, lse = R.head_topk(q, w, 16, b)
    assert not any(m in idx.flatten().tolist() for m in masked)
    keep = torch.ones(60, dtype=torch.bool)
    keep[masked] = False
    Z = q @ w.t() + b
    assert torch.allclose(lse, torch.logsumexp(Z[:, keep], 1))
    assert bool(torch.isfinite(lse).all())


# ---------------------------------------------------------------------------
def small_option(angular=False, E=16, L=37):
    return Option(terminal_count=30, path_count=25, label_count=L,
                  max_path_length=6, terminal_embed_size=8,
                  path_embed_size=8, encode_size=E, dropout_prob=0.0,
                  angular_margin_loss=angular, batch_size=4,
                  device=torch.device("cpu"))


def small_batch(opt, B=9, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = opt.max_path_length
    starts = torch.randint(1, opt.terminal_count, (B, C), generator=g)
    paths = torch.randint(1, opt.path_count, (B, C), generator=g)
    ends = torch.randint(1, opt.terminal_count, (B, C), generator=g)
    starts[:, C - 2:] = 0  # pads
    starts[0, 1:] = 0
    return starts, paths, ends


def test_torch_model_default_head_equals_forward_through_row_topk():
    opt = small_option()
    g = torch.Generator().manual_seed(1)
    logical = init_logical_params(opt, g)
    logical["output_bias"] = torch.randn(opt.label_count, generator=g)
    model = Code2VecTorch(opt, logical).eval()
    s, p, e = small_batch(opt)
    with torch.no_grad():
        outputs, cv, attn = model(s, p, e, torch.zeros(9, dtype=torch.int64))
    cv2, cvb, attn2 = model.encode(s, p, e)
    assert torch.equal(cv2, cv) and torch.equal(attn2, attn)
    assert cvb.dtype == torch.float32 and torch.equal(cvb, cv)
    vals, idx, lse = model.head_topk(cvb, 7)
    rv, ri, rl = R.row_topk(outputs, 7)
    assert torch.equal(idx, ri)
    assert torch.allclose(vals, rv, atol=1e-5)
    assert torch.allclose(lse, rl, atol=1e-5)


def test_torch_model_angular_head_is_margin_free_cosine():
    opt = small_option(angular=True)
    model = Code2VecTorch(opt, init_logical_params(
        opt, torch.Generator().manual_seed(2))).eval()
    s, p, e = small_batch(opt)
    cv, cvb, _ = model.encode(s, p, e)
    k = 16
    vals, idx, lse = model.head_topk(cvb, k)
    cos = F.normalize(cv) @ F.normalize(model.output_weight.detach()).t()
    Z = opt.inverse_temp * cos
    rv, ri, rl = R.row_topk(Z, k)
    assert torch.equal(idx, ri)
    assert torch.allclose(vals, rv, atol=1e-5)
    assert torch.allclose(lse, rl, atol=1e-5)
    # forward(label) differs from these logits in the label's column only
    label = torch.arange(9) % opt.label_count
    with torch.no_grad():
        outputs, _, _ = model(s, p, e, label)
    other = torch.ones_like(outputs, dtype=torch.bool)
    other[torch.arange(9), label] = False
    assert torch.allclose(outputs[other], Z[other], atol=1e-5)
    hit = cos[torch.arange(9), label] > 0
    assert bool(hit.any())
    assert bool((outputs[torch.arange(9), label][hit]
                 < Z[torch.arange(9), label][hit] - 1e-3).all())


# ---------------------------------------------------------------------------
def corpus_model(tiny_corpus, angular, seed=0):
    reader = CorpusReader(tiny_corpus["corpus_path"],
                          tiny_corpus["path_idx_path"],
                          tiny_corpus["terminal_idx_path"])
    opt = Option(terminal_count=len(reader.terminal_vocab),
                 path_count=len(reader.path_vocab),
                 label_count=len(reader.label_vocab), max_path_length=24,
                 terminal_embed_size=12, path_embed_size=12, encode_size=16,
                 dropout_prob=0.0, batch_size=16,
                 angular_margin_loss=angular, device=torch.device("cpu"))
    g = torch.Generator().manual_seed(seed)
    logical = init_logical_params(opt, g)
    if not angular:
        logical["output_bias"] = torch.randn(opt.label_count, generator=g)
    return reader, Code2VecTorch(opt, logical)


@pytest.mark.parametrize("all_contexts", [False, True])
def test_predictor_fused_head_default_head_matches_unfused(tiny_corpus,
                                                           all_contexts):
    reader, model = corpus_model(tiny_corpus, angular=False)
    cpu = torch.device("cpu")
    kw = dict(topk=5, top_contexts=3, batch_size=16,
              all_contexts=all_contexts)
    base = list(Predictor(model, reader, cpu, **kw)
                .predict_items(reader.items))
    fused = list(Predictor(model, reader, cpu, fused_head=True, **kw)
                 .predict_items(reader.items))
    assert len(base) == len(fused) == 48
    for a, b in zip(base, fused):
        assert a.id == b.id
        assert [n for n, _ in a.names] == [n for n, _ in b.names]
        for (_, pa), (_, pb) in zip(a.names, b.names):
            assert abs(pa - pb) <= 1e-5 * max(pa, 1e-3)  # fp32 noise
        assert a.contexts == b.contexts
        assert torch.equal(a.code_vector, b.code_vector)


@pytest.mark.parametrize("all_contexts", [False, True])
def test_predictor_fused_head_accepts_the_angular_head(tiny_corpus,
                                                       all_contexts):
    reader, model = corpus_model(tiny_corpus, angular=True)
    cpu = torch.device("cpu")
    with pytest.raises(ValueError, match="angular") as e:
        Predictor(model, reader, cpu, all_contexts=all_contexts)
    assert "fused_head=True" in str(e.value)
    assert "--fused_head" in str(e.value)
    preds = list(Predictor(model, reader, cpu, topk=5, top_contexts=3,
                           batch_size=16, all_contexts=all_contexts,
                           fused_head=True).predict_items(reader.items))
    assert len(preds) == 48
    known = set(reader.label_vocab.stoi)
    for p in preds:
        probs = [x for _, x in p.names]
        assert len(probs) == 5 and all(n in known for n, _ in p.names)
        assert all(0.0 < x <= 1.0 for x in probs)
        assert probs == sorted(probs, reverse=True)
        assert sum(probs) <= 1.0 + 1e-5
        assert 1 <= len(p.contexts) <= 3
    # forward_packed keeps its rejection: no label-free [B, L] exists there
    model.eval()
    with pytest.raises(ValueError, match="angular"):
        model.forward_packed(torch.ones(3, dtype=torch.int64),
                             torch.ones(3, dtype=torch.int64),
                             torch.ones(3, dtype=torch.int64), [3])
