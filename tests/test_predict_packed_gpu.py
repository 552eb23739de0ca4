"""Packed prediction on the HIP backend: Code2VecHIP.forward_packed against
the torch oracle and against the padded HIP forward, its independence from
the batch composition, and Predictor(all_contexts=True)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.data.builder import PackedData
from code2vec_amd.engine.loader import PackedBatchIterator
from code2vec_amd.engine.predict import Predictor
from code2vec_amd.models.code2vec import (
    Code2VecHIP, Code2VecTorch, init_logical_params)
from code2vec_amd.utils.options import Option

from test_predict_gpu import StubReader, relerr, T, P, L, C, TOPK, TOPC

MC = 40   # max_path_length of the model test
MODEL_LENGTHS = [1, 5, MC, MC + 1, 100, 17, 300, MC - 1, 64, 2, 3 * MC, 9]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def flat_inputs(lengths, n_term, n_path, seed):
    rng = np.random.default_rng(seed)
    M = int(sum(lengths))
    return tuple(torch.from_numpy(rng.integers(1, hi, M).astype(np.int32))
                 for hi in (n_term, n_path, n_term))


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(int)


def hand_pad(flat, lengths, width):
    out = torch.zeros(len(lengths), width, dtype=flat.dtype)
    for i, (lo, n) in enumerate(zip(offsets_of(lengths), lengths)):
        out[i, :n] = flat[lo:lo + n]
    return out


@pytest.fixture(scope="module")
def models(dev):
    opt = Option(terminal_count=3000, path_count=2500, label_count=700,
                 max_path_length=MC, terminal_embed_size=100,
                 path_embed_size=100, encode_size=100, dropout_prob=0.25,
                 batch_size=32, device=dev)
    logical = init_logical_params(opt, torch.Generator().manual_seed(21))
    hip = Code2VecHIP(opt, logical, device=dev).eval()
    ref = Code2VecTorch(opt, logical).eval()
    s, p, e = flat_inputs(MODEL_LENGTHS, 3000, 2500, seed=4)
    with torch.no_grad():
        out = hip.forward_packed(s.to(dev), p.to(dev), e.to(dev),
                                 MODEL_LENGTHS)
    torch.cuda.synchronize()
    return hip, ref, (s, p, e), tuple(t.float().cpu() for t in out)


def test_forward_packed_matches_torch_oracle(models):
    hip, ref, (s, p, e), (out_h, cv_h, attn_h) = models
    B, M = len(MODEL_LENGTHS), sum(MODEL_LENGTHS)
    assert out_h.shape == (B, 700) and cv_h.shape == (B, 100)
    assert attn_h.shape == (M,)
    out_r, cv_r, attn_r = ref.forward_packed(s, p, e, MODEL_LENGTHS)
    # the bounds of tests/test_model_gpu.py
    assert relerr(attn_h, attn_r) < 3e-2
    assert relerr(cv_h, cv_r) < 3e-2
    assert relerr(out_h, out_r) < 5e-2
    for lo, n in zip(offsets_of(MODEL_LENGTHS), MODEL_LENGTHS):
        assert abs(float(attn_h[lo:lo + n].sum()) - 1.0) < 1e-4


def test_forward_packed_matches_padded_hip_forward(models, dev):
    hip, _, (s, p, e), (out_h, cv_h, attn_h) = models
    offs = offsets_of(MODEL_LENGTHS)
    short = [i for i, n in enumerate(MODEL_LENGTHS) if n <= MC]
    assert len(short) >= 6 and len(short) < len(MODEL_LENGTHS)
    lens = [MODEL_LENGTHS[i] for i in short]
    rows = torch.cat([torch.arange(offs[i], offs[i + 1]) for i in short])
    with torch.no_grad():
        out_p, cv_p, attn_p = hip(
            *(hand_pad(t[rows], lens, MC).to(dev) for t in (s, p, e)),
            torch.zeros(len(short), dtype=torch.int64, device=dev))
    out_p, cv_p, attn_p = (t.float().cpu() for t in (out_p, cv_p, attn_p))
    ragged = torch.cat([attn_p[j, :n] for j, n in enumerate(lens)])
    assert relerr(attn_h[rows], ragged) < 3e-2
    assert relerr(cv_h[short], cv_p) < 3e-2
    assert relerr(out_h[short], out_p) < 5e-2
    for j, n in enumerate(lens):          # pads carry no weight
        assert float(attn_p[j, n:].abs().sum()) == 0.0


def test_code_vector_and_attention_independent_of_batch(models, dev):
    """Gather and combiner are row-local, K21 is segment-local: a method's
    code vector and attention have the same bits in another batch."""
    hip, _, (s, p, e), (_, cv_h, attn_h) = models
    offs = offsets_of(MODEL_LENGTHS)
    order = [6, 0, 11, 3, 4]              # other neighbours, other positions
    lens = [MODEL_LENGTHS[i] for i in order]
    rows = torch.cat([torch.arange(offs[i], offs[i + 1]) for i in order])
    with torch.no_grad():
        _, cv2, attn2 = hip.forward_packed(
            s[rows].to(dev), p[rows].to(dev), e[rows].to(dev), lens)
    cv2, attn2 = cv2.float().cpu(), attn2.float().cpu()
    assert torch.equal(attn2, attn_h[rows])
    assert torch.equal(cv2, cv_h[order])
    for i in (2, 6):                       # alone
        r = torch.arange(offs[i], offs[i + 1])
        with torch.no_grad():
            _, cv1, attn1 = hip.forward_packed(
                s[r].to(dev), p[r].to(dev), e[r].to(dev),
                [MODEL_LENGTHS[i]])
        assert torch.equal(attn1.float().cpu(), attn_h[r])
        assert torch.equal(cv1.float().cpu()[0], cv_h[i])


# ---------------------------------------------------------------------------
# Predictor(all_contexts=True)

N_POOL = 256
N_KEEP = 12


@pytest.fixture(scope="module")
def predictor_setup(dev):
    """The model of tests/test_predict_gpu.py (same sizes, same seed) and
    methods on which its logits are well separated: from a seeded pool,
    those whose top TOPK + 1 ORACLE logits (torch backend, fp32) are
    pairwise at least 5e-2 of the method's logit RMS apart — the logits
    bound of tests/test_model_gpu.py, so that the bf16 path cannot
    legitimately swap two of them.  A bag of 3 * C contexts and a
    zero-context method (one PAD row) are always included."""
    opt = Option(terminal_count=T, path_count=P, label_count=L,
                 max_path_length=C, terminal_embed_size=100,
                 path_embed_size=100, encode_size=100, dropout_prob=0.0,
                 batch_size=16, device=dev)
    logical = init_logical_params(opt, torch.Generator().manual_seed(11))
    hip = Code2VecHIP(opt, logical, device=dev)
    ref = Code2VecTorch(opt, logical).eval()
    rng = np.random.default_rng(3)
    lengths = rng.integers(1, 3 * C + 1, N_POOL).tolist()
    s, p, e = flat_inputs(lengths, T, P, seed=5)
    out_r, _, _ = ref.forward_packed(s, p, e, lengths)
    top = torch.sort(out_r, dim=1, descending=True).values[:, :TOPK + 1]
    gap = (top[:, :-1] - top[:, 1:]).min(dim=1).values
    ok = torch.nonzero(gap >= 5e-2 * out_r.pow(2).mean(dim=1).sqrt())
    keep = ok.flatten().tolist()[:N_KEEP]
    assert len(keep) >= 6, "pool too small for the separation rule"
    offs = offsets_of(lengths)
    segs = [(s[offs[i]:offs[i + 1]], p[offs[i]:offs[i + 1]],
             e[offs[i]:offs[i + 1]]) for i in keep]
    big = flat_inputs([3 * C], T, P, seed=6)
    pad = tuple(torch.zeros(1, dtype=torch.int32) for _ in range(3))
    segs = segs[:3] + [big] + segs[3:] + [pad]
    data = PackedData(
        ids=list(range(100, 100 + len(segs))),
        starts=torch.cat([x[0] for x in segs]).numpy(),
        paths=torch.cat([x[1] for x in segs]).numpy(),
        ends=torch.cat([x[2] for x in segs]).numpy(),
        lengths=np.asarray([x[0].numel() for x in segs], dtype=np.int64),
        labels=np.zeros(len(segs), dtype=np.int64))
    return hip, ref, data, len(keep)


def run_predictor(model, data, device, budget, seed=123):
    pr = Predictor(model, StubReader(), device, topk=TOPK, top_contexts=TOPC,
                   batch_size=16, seed=seed, all_contexts=True,
                   max_batch_contexts=budget)
    assert pr.graphed is None
    preds = []
    for batch in PackedBatchIterator(data, budget, device=pr.device):
        preds += pr.predict_packed_batch(batch)
    return preds


def test_all_contexts_names_match_torch_backend(predictor_setup, dev):
    hip, ref, data, n_sep = predictor_setup
    got = run_predictor(hip, data, dev, 10 ** 6)
    want = run_predictor(ref, data, torch.device("cpu"), 10 ** 6)
    assert [g.id for g in got] == data.ids == [w.id for w in want]
    separated = [i for i in range(len(got)) if i != 3][:n_sep]
    for i in separated:
        assert [n for n, _ in got[i].names] == [n for n, _ in want[i].names]
    # probabilities against the softmax of the model's own logits, at the
    # bound of tests/test_predict_gpu.py
    with torch.no_grad():
        outputs, cv, _ = hip.forward_packed(
            torch.from_numpy(data.starts).to(dev),
            torch.from_numpy(data.paths).to(dev),
            torch.from_numpy(data.ends).to(dev), data.lengths.tolist())
    outputs = outputs.float().cpu()
    _, order = torch.sort(outputs, dim=1, descending=True, stable=True)
    soft = torch.softmax(outputs, dim=1)
    for i, pred in enumerate(got):
        idx = order[i, :TOPK].tolist()
        assert [n for n, _ in pred.names] == [f"name{j}" for j in idx]
        err = relerr(torch.tensor([q for _, q in pred.names]), soft[i, idx])
        assert err < 1e-4, (i, err)
        assert torch.equal(pred.code_vector, cv[i].float().cpu())


def test_all_contexts_reports_top_real_contexts_of_whole_bag(
        predictor_setup, dev):
    hip, _, data, _ = predictor_setup
    got = run_predictor(hip, data, dev, 10 ** 6)
    with torch.no_grad():
        _, _, attn = hip.forward_packed(
            torch.from_numpy(data.starts).to(dev),
            torch.from_numpy(data.paths).to(dev),
            torch.from_numpy(data.ends).to(dev), data.lengths.tolist())
    attn = attn.float().cpu()
    offs = offsets_of(data.lengths)
    assert int(data.lengths[3]) == 3 * C
    for i, pred in enumerate(got):
        lo, n = int(offs[i]), int(data.lengths[i])
        real = [c for c in range(n) if int(data.starts[lo + c]) != 0]
        real.sort(key=lambda c: (-float(attn[lo + c]), c))
        want = real[:TOPC]
        assert pred.contexts == [
            (f"t{int(data.starts[lo + c])}", f"p{int(data.paths[lo + c])}",
             f"t{int(data.ends[lo + c])}", float(attn[lo + c]))
            for c in want]
        assert all(s != "<PAD/>" for s, _, _, _ in pred.contexts)
    assert len(got[3].contexts) == TOPC
    assert got[-1].contexts == []          # the zero-context method
    # some reported context of the long bag lies past max_path_length
    top3c = sorted(range(3 * C),
                   key=lambda c: (-float(attn[offs[3] + c]), c))[:TOPC]
    assert max(top3c) >= C


def test_all_contexts_same_output_for_two_seeds_and_budgets(
        predictor_setup, dev):
    hip, _, data, _ = predictor_setup
    a = run_predictor(hip, data, dev, 10 ** 6, seed=1)
    b = run_predictor(hip, data, dev, 10 ** 6, seed=99)
    c = run_predictor(hip, data, dev, 2 * C, seed=99)
    for x, y, z in zip(a, b, c):
        assert x.id == y.id == z.id
        assert x.names == y.names and x.contexts == y.contexts
        assert torch.equal(x.code_vector, y.code_vector)
        # another batch composition: code vector and attention keep their
        # bits (the head's GEMM tiles over the batch, so names are compared
        # through the fixed seed pair above)
        assert torch.equal(x.code_vector, z.code_vector)
        assert x.contexts == z.contexts
