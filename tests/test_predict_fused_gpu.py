"""K23 through the model and the Predictor on the HIP backend: encode's
bits, the default and the angular-margin head against fp64 logits of the
stored bf16 operands (the rule and bounds of test_head_topk_gpu.py), the
fused predictor against the logits path on a planted checkpoint, packed and
graphed prediction, and peak memory.

Planted checkpoints: the output weight solves cv . W^T = target exactly
(minimum-norm least squares over the batch's code vectors, B <= E), so each
method's top-k logits sit 2 apart (3 for the angular head) above a floor of
small random values; the tests assert the premise they need — separation
>= 1 and |z| <= 32 — on the fp64 logits of the tensors as stored.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from head_topk_rule import (K19_CHAIN, check_rule, lse_bound, lse_logit_tol,
                            n_chain)

from code2vec_amd.data.synthetic import _IndexVocab
from code2vec_amd.engine.predict import Predictor
from code2vec_amd.models.code2vec import (
    Code2VecHIP, Code2VecTorch, _unit_rows, init_logical_params)
from code2vec_amd.ops import functional as Fn
from code2vec_amd.utils.options import Option

T, P, C, B = 400, 300, 12, 16
K = 5


class StubReader:
    """The vocab surface Predictor reads names from."""

    def __init__(self, L):
        self.terminal_vocab = _IndexVocab(
            ["<PAD/>"] + [f"t{i}" for i in range(1, T)])
        self.path_vocab = _IndexVocab(
            ["<PAD/>"] + [f"p{i}" for i in range(1, P)])
        self.label_vocab = _IndexVocab([f"name{i}" for i in range(L)])


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_option(dev, L, E=100, angular=False, batch_size=B):
    return Option(terminal_count=T, path_count=P, label_count=L,
                  max_path_length=C, terminal_embed_size=100,
                  path_embed_size=100, encode_size=E, dropout_prob=0.0,
                  angular_margin_loss=angular, batch_size=batch_size,
                  device=dev)


def make_batch(n=B, seed=3):
    rng = np.random.default_rng(seed)
    starts = rng.integers(1, T, (n, C)).astype(np.int32)
    paths = rng.integers(1, P, (n, C)).astype(np.int32)
    ends = rng.integers(1, T, (n, C)).astype(np.int32)
    lens = rng.integers(3, C + 1, n)
    lens[0] = 2
    lens[1] = C
    pad = np.arange(C)[None, :] >= lens[:, None]
    for a in (starts, paths, ends):
        a[pad] = 0
    return {"id": torch.arange(100, 100 + n),
            "starts": torch.from_numpy(starts),
            "paths": torch.from_numpy(paths),
            "ends": torch.from_numpy(ends),
            "label": torch.zeros(n, dtype=torch.int64)}


def make_model(dev, L, E=100, angular=False, seed=11, batch_size=B):
    opt = make_option(dev, L, E, angular, batch_size)
    logical = init_logical_params(opt, torch.Generator().manual_seed(seed))
    if not angular:
        logical["output_bias"] = 0.5 * torch.randn(
            L, generator=torch.Generator().manual_seed(seed + 1))
    return Code2VecHIP(opt, logical, device=dev).eval(), logical


def on_dev(batch, dev):
    return tuple(batch[k].to(dev) for k in ("starts", "paths", "ends"))


def head_case(q, w, bias, scale):
    """fp64 logits, tolerances and lse of stored operands, as the rule's
    case dict."""
    qd, wd = q.double().cpu(), w.double().cpu()
    Z = scale * (qd @ wd.t())
    mag = scale * (qd.abs() @ wd.abs().t())
    if bias is not None:
        Z = Z + bias.double().cpu()
        mag = mag + bias.double().cpu().abs()
    return dict(Z=Z, tol=(q.shape[1] + 2) * 2.0 ** -23 * mag,
                lse=torch.logsumexp(Z, dim=1), plants=[])


def default_chain(L, EP):
    return n_chain(L, Fn.head_topk_default_nsplit(L, EP))


# ---------------------------------------------------------------------------
def test_encode_has_forward_bits(dev):
    model, _ = make_model(dev, 512)
    s, p, e = on_dev(make_batch(), dev)
    with torch.no_grad():
        _, cv, attn = model(s, p, e, torch.zeros(B, dtype=torch.int64,
                                                 device=dev))
    cv2, cvb, attn2 = model.encode(s, p, e)
    assert torch.equal(cv2, cv) and torch.equal(attn2, attn)
    assert cvb.dtype == torch.bfloat16 and cvb.shape == (B, model.EP)

    lens = torch.tensor([3, 1, 12, 7, 30])
    M = int(lens.sum())
    g = torch.Generator().manual_seed(5)
    fs = torch.randint(1, T, (M,), generator=g).to(dev)
    fp = torch.randint(1, P, (M,), generator=g).to(dev)
    fe = torch.randint(1, T, (M,), generator=g).to(dev)
    _, pcv, pattn = model.forward_packed(fs, fp, fe, lens)
    pcv2, pcvb, pattn2 = model.encode_packed(fs, fp, fe, lens)
    assert torch.equal(pcv2, pcv) and torch.equal(pattn2, pattn)
    assert pcvb.dtype == torch.bfloat16 and pcvb.shape == (5, model.EP)


@pytest.mark.parametrize("L,E", [(512, 100), (4105, 100), (533, 40)])
def test_default_head_passes_the_rule(dev, L, E):
    model, _ = make_model(dev, L, E)
    _, cvb, _ = model.encode(*on_dev(make_batch(), dev))
    c = head_case(cvb, model.output_weight.detach(),
                  model.output_bias.detach(), 1.0)
    vals, idx, lse = model.head_topk(cvb, 10)
    check_rule(vals, idx, lse, c, 10, default_chain(L, model.EP),
               tag=f"model default E={E}")


def plant_default_head(model, cvb, k, seed=0):
    """Rewrite the head so every method's top-k logits are 24, 22, ... on
    its own labels and everything else lies in [-4, 4]."""
    n, L = cvb.shape[0], model.option.label_count
    assert L >= n * k
    g = torch.Generator().manual_seed(seed)
    target = (torch.rand(n, L, generator=g) * 8 - 4).double()
    for i in range(n):
        for j in range(k):
            target[i, k * i + j] = 24.0 - 2.0 * j
    bias = torch.rand(L, generator=g) * 2 - 1
    X = cvb.double().cpu()
    Wt = torch.linalg.pinv(X) @ (target - bias.double())  # [EP, L]
    with torch.no_grad():
        model.output_weight.copy_(Wt.t().to(torch.bfloat16))
        model.output_bias.copy_(bias)


def test_fused_predictor_equals_the_logits_path_on_a_planted_head(dev):
    L = 4105  # two default slices
    model, _ = make_model(dev, L)
    batch = make_batch()
    _, cvb, _ = model.encode(*on_dev(batch, dev))
    plant_default_head(model, cvb, K)
    c = head_case(cvb, model.output_weight.detach(),
                  model.output_bias.detach(), 1.0)
    top = torch.sort(c["Z"], dim=1, descending=True).values[:, :K + 1]
    assert float(c["Z"].abs().max()) <= 32.0            # premise
    assert float((top[:, :-1] - top[:, 1:]).min()) >= 1.0  # premise
    reader = StubReader(L)
    kw = dict(topk=K, top_contexts=3, batch_size=B, use_graph=False)
    base = Predictor(model, reader, dev, **kw).predict_batch(batch)
    fused = Predictor(model, reader, dev, fused_head=True,
                      **kw).predict_batch(batch)
    # bf16 rounding of a stored logit with |z| <= 32 is at most 0.125, in
    # the value and in the lse; the lse's own error is the K23 bound
    lb = lse_bound(c["lse"], lse_logit_tol(c["Z"], c["tol"]),
                   max(default_chain(L, model.EP), K19_CHAIN))
    for i, (a, b) in enumerate(zip(base, fused)):
        assert [n for n, _ in a.names] == [n for n, _ in b.names]
        assert [n for n, _ in b.names] == [f"name{K * i + j}"
                                           for j in range(K)]
        rel = float(torch.exp(2 * 0.125 + lb[i]) - 1.0)
        for (_, pa), (_, pb) in zip(a.names, b.names):
            assert abs(pa - pb) <= rel * pb, (i, pa, pb, rel)
        assert a.contexts == b.contexts
        assert torch.equal(a.code_vector, b.code_vector)


# ---------------------------------------------------------------------------
def angular_case(model, cvb):
    ucv = _unit_rows(cvb)
    uw = model._unit_output_weight()
    return ucv, uw, head_case(ucv, uw, None, model.option.inverse_temp)


@pytest.mark.parametrize("E", [100, 40])  # EP = 128 and EP = 64
def test_angular_head_passes_the_rule(dev, E):
    L = 4105
    model, _ = make_model(dev, L, E, angular=True)
    batch = make_batch()
    _, cvb, _ = model.encode(*on_dev(batch, dev))
    ucv, uw, c = angular_case(model, cvb)
    uw = uw.clone()  # the image is one buffer, refreshed in place
    # unit rows as stored: bf16 images of fp32-normalized rows
    assert float((uw.float().norm(dim=1) - 1).abs().max()) < 2e-2
    vals, idx, lse = model.head_topk(cvb, K)
    check_rule(vals, idx, lse, c, K, default_chain(L, model.EP),
               tag=f"model angular E={E}")
    preds = Predictor(model, StubReader(L), dev, topk=K, top_contexts=3,
                      batch_size=B, use_graph=False,
                      fused_head=True).predict_batch(batch)
    probs = torch.exp(vals - lse[:, None]).cpu()
    for i, p in enumerate(preds):
        assert [n for n, _ in p.names] == [f"name{int(j)}" for j in idx[i]]
        assert [x for _, x in p.names] == [float(x) for x in probs[i]]
        assert sum(x for _, x in p.names) <= 1.0 + 1e-5

    # the cached unit rows follow an in-place change of the weight
    with torch.no_grad():
        model.output_weight.neg_()
    v2, i2, l2 = model.head_topk(cvb, K)
    ucv, uw2, c2 = angular_case(model, cvb)
    assert torch.equal(uw2, -uw)
    # one buffer for the model's lifetime: eval() on a model in eval mode
    # and a refresh keep its address
    ptr = uw2.data_ptr()
    model.eval()
    assert model._unit_output_weight().data_ptr() == ptr
    model.train()
    model.eval()  # marks the image stale: rebuilt in place
    assert model._unit_output_weight().data_ptr() == ptr
    assert torch.equal(model._unit_output_weight(), -uw)
    check_rule(v2, i2, l2, c2, K, default_chain(L, model.EP),
               tag="model angular, negated weight")
    assert not torch.equal(i2, idx)


def plant_angular_head(ucv, E, L, k, seed=0):
    """Unit rows W [L, E] with cos(ucv_i, W_l) = target exactly: the
    minimum-norm solution of U w = c plus a component orthogonal to every
    code vector that brings the row to unit length.  A method's own labels
    get cosines 0.6, 0.5, ... (logits 3 apart at inverse_temp 30), all
    others |cos| <= 0.03."""
    U = ucv[:, :E].double().cpu()
    U = U / U.norm(dim=1, keepdim=True)
    n = U.shape[0]
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(n, L, generator=g) * 0.06 - 0.03).double()
    for i in range(n):
        for j in range(k):
            c[i, k * i + j] = 0.6 - 0.1 * j
    X = U.t() @ torch.linalg.solve(U @ U.t(), c)  # [E, L], U X = c
    norm2 = (X * X).sum(dim=0)
    assert float(norm2.max()) < 1.0, float(norm2.max())  # premise
    Q, _ = torch.linalg.qr(torch.cat(
        [U.t(), torch.randn(E, E - n, generator=g).double()], dim=1))
    comp = Q[:, n:] @ torch.randn(E - n, L, generator=g).double()
    comp = comp / comp.norm(dim=0, keepdim=True)
    return (X + torch.sqrt(1.0 - norm2) * comp).t().contiguous()


def test_angular_names_equal_the_cpu_oracle_model(dev):
    L, E = 533, 100
    model, logical = make_model(dev, L, E, angular=True)
    batch = make_batch()
    _, cvb, _ = model.encode(*on_dev(batch, dev))
    W = plant_angular_head(_unit_rows(cvb), E, L, K).to(torch.bfloat16)
    with torch.no_grad():
        model.output_weight[:, :E].copy_(W)
    logical = dict(logical, output_weight=W.float())
    oracle = Code2VecTorch(make_option(torch.device("cpu"), L, E, True),
                           logical).eval()
    reader = StubReader(L)
    kw = dict(topk=K, top_contexts=3, batch_size=B, fused_head=True)
    got = Predictor(model, reader, dev, **kw).predict_batch(batch)
    want = Predictor(oracle, reader, torch.device("cpu"),
                     **kw).predict_batch(batch)
    for i, (a, b) in enumerate(zip(got, want)):
        assert [n for n, _ in a.names] == [f"name{K * i + j}"
                                           for j in range(K)]
        assert [n for n, _ in a.names] == [n for n, _ in b.names]


# ---------------------------------------------------------------------------
def packed_batch(lens, seed, ids=None):
    g = torch.Generator().manual_seed(seed)
    M = int(lens.sum())
    return {"id": ids if ids is not None else torch.arange(len(lens)),
            "starts": torch.randint(1, T, (M,), generator=g),
            "paths": torch.randint(1, P, (M,), generator=g),
            "ends": torch.randint(1, T, (M,), generator=g),
            "lengths": lens}


@pytest.mark.parametrize("angular", [False, True])
def test_packed_prediction_is_batch_independent(dev, angular):
    L = 4105
    model, _ = make_model(dev, L, angular=angular)
    pred = Predictor(model, StubReader(L), dev, topk=K, top_contexts=3,
                     all_contexts=True, fused_head=True)
    lens = torch.randint(1, 31, (50,),
                         generator=torch.Generator().manual_seed(2))
    batch = packed_batch(lens, 9)
    full = pred.predict_packed_batch(batch)
    offs = torch.cumsum(lens, 0) - lens
    for i in (0, 7, 49):
        lo, hi = int(offs[i]), int(offs[i] + lens[i])
        one = {"id": torch.tensor([i]), "lengths": lens[i:i + 1],
               **{k: batch[k][lo:hi] for k in ("starts", "paths", "ends")}}
        alone = pred.predict_packed_batch(one)[0]
        assert alone.names == full[i].names  # floats compared exactly
        assert alone.contexts == full[i].contexts
        assert torch.equal(alone.code_vector, full[i].code_vector)


@pytest.mark.parametrize("angular", [False, True])
def test_graph_replay_equals_eager_with_a_tail_batch(dev, angular):
    L = 4105
    model, _ = make_model(dev, L, angular=angular)
    reader = StubReader(L)
    kw = dict(topk=K, top_contexts=3, batch_size=B, fused_head=True)
    graphed = Predictor(model, reader, dev, use_graph=True, **kw)
    assert graphed.graphed is not None and graphed.graphed.topk == K
    eager = Predictor(model, reader, dev, use_graph=False, **kw)
    batch = make_batch()
    tail = {k: v[:5] for k, v in batch.items()}
    for b in (batch, tail, batch):
        for x, y in zip(graphed.predict_batch(b), eager.predict_batch(b)):
            assert x.id == y.id and x.names == y.names
            assert x.contexts == y.contexts
            assert torch.equal(x.code_vector, y.code_vector)


@pytest.mark.parametrize("E", [100, 40])  # EP = 128 and EP = 64
def test_angular_graph_outlives_eval_and_follows_the_weight(dev, E):
    """The captured graph reads the angular head's unit-row image.  The image
    is one buffer of the model: eval(), a second Predictor and an emptied
    allocator cache leave the replay valid, and after an in-place weight
    change the replay scores the new weight, as the eager path does."""
    L = 4105
    model, _ = make_model(dev, L, E, angular=True)
    reader = StubReader(L)
    kw = dict(topk=K, top_contexts=3, batch_size=B, fused_head=True)
    graphed = Predictor(model, reader, dev, use_graph=True, **kw)
    assert graphed.graphed is not None
    ptr = model._unit_output_weight().data_ptr()
    batch = make_batch()
    first = graphed.predict_batch(batch)

    model.eval()
    eager = Predictor(model, reader, dev, use_graph=False, **kw)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert model._unit_output_weight().data_ptr() == ptr
    junk = torch.full((L, model.EP), 7.0, dtype=torch.bfloat16, device=dev)
    again = graphed.predict_batch(batch)
    want = eager.predict_batch(batch)
    for x, y, z in zip(again, want, first):
        assert x.names == y.names == z.names
        assert torch.equal(x.code_vector, y.code_vector)

    with torch.no_grad():
        model.output_weight.neg_()
    changed = graphed.predict_batch(batch)
    want = eager.predict_batch(batch)
    assert model._unit_output_weight().data_ptr() == ptr
    for x, y, z in zip(changed, want, first):
        assert x.names == y.names
        assert [n for n, _ in x.names] != [n for n, _ in z.names]
    del junk


def test_fused_head_never_allocates_the_logits(dev):
    L, n = 131080, 64
    model, _ = make_model(dev, L, batch_size=n)
    reader = StubReader(L)
    batch = make_batch(n)
    logits_bytes = n * L * 2  # one [B, L] bf16 matrix
    kw = dict(topk=K, top_contexts=3, batch_size=n, use_graph=False)

    def peak(pred, fn, arg):
        fn(pred, arg)  # warm-up: persistent scratch is allocated once
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fn(pred, arg)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated(dev) - before

    fused = Predictor(model, reader, dev, fused_head=True, **kw)
    base = Predictor(model, reader, dev, **kw)
    pf = peak(fused, Predictor.predict_batch, batch)
    pb = peak(base, Predictor.predict_batch, batch)
    print(f"peak above the pre-call level at B={n}, L={L}: fused "
          f"{pf / 2**20:.1f} MiB, logits path {pb / 2**20:.1f} MiB, one "
          f"[B, L] bf16 matrix {logits_bytes / 2**20:.1f} MiB")
    assert pf < logits_bytes
    assert pb > logits_bytes
    lens = torch.full((n,), C, dtype=torch.int64)
    packed = Predictor(model, reader, dev, fused_head=True,
                       all_contexts=True, **kw)
    pp = peak(packed, Predictor.predict_packed_batch,
              packed_batch(lens, 4))
    assert pp < logits_bytes
