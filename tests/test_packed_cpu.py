"""Packed (variable-length) prediction on the CPU: build_packed, the packed
batch iterator, the K21 oracle, Code2VecTorch.forward_packed, the
Predictor's all_contexts path and tools/predict.py --all_contexts."""

import copy
import json

import numpy as np
import pytest
import torch

from code2vec_amd.data.builder import DatasetBuilder, PackedData
from code2vec_amd.data.reader import CodeItem, CorpusReader
from code2vec_amd.engine.loader import PackedBatchIterator
from code2vec_amd.engine.predict import Predictor
from code2vec_amd.models.code2vec import (
    Code2VecTorch, init_logical_params)
from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R
from code2vec_amd.utils.options import Option
from tools import predict as predict_cli

from test_predict_cpu import predict_argv, train_checkpoint

C = 16


def make_reader(tiny_corpus, **kw):
    return CorpusReader(tiny_corpus["corpus_path"],
                        tiny_corpus["path_idx_path"],
                        tiny_corpus["terminal_idx_path"], **kw)


def make_option(reader, **kw):
    defaults = dict(max_path_length=C, terminal_embed_size=8,
                    path_embed_size=8, encode_size=12, dropout_prob=0.0,
                    batch_size=4, device=torch.device("cpu"))
    defaults.update(kw)
    return Option(terminal_count=len(reader.terminal_vocab),
                  path_count=len(reader.path_vocab),
                  label_count=len(reader.label_vocab), **defaults)


def long_item(reader, n, item_id=900):
    """A method of ``n`` contexts over the reader's vocabularies, the
    first of which starts at @method_0."""
    rng = np.random.default_rng(n)
    pcs = np.stack([
        rng.integers(2, len(reader.terminal_vocab), n),
        rng.integers(1, len(reader.path_vocab), n),
        rng.integers(2, len(reader.terminal_vocab), n)], axis=1
    ).astype(np.int32)
    pcs[0, 0] = reader.terminal_vocab.stoi["@method_0"]
    src = reader.items[0]
    return CodeItem(id=item_id, label=src.label,
                    normalized_label=src.normalized_label,
                    source=src.source, aliases=dict(src.aliases),
                    path_contexts=pcs)


def segments(packed: PackedData):
    offs = np.concatenate([[0], np.cumsum(packed.lengths)])
    return [(int(offs[i]), int(offs[i + 1])) for i in range(len(packed))]


# ---------------------------------------------------------------------------
# build_packed


def test_build_packed_keeps_every_context_in_corpus_order(tiny_corpus):
    r = make_reader(tiny_corpus)
    b = DatasetBuilder(r, make_option(r), split_ratio=0.0, seed=5)
    empty = copy.copy(r.items[1])
    empty.path_contexts = np.empty((0, 3), dtype=np.int32)
    big = long_item(r, 3 * C)
    items = [r.items[0], empty, big] + list(r.items[2:6])
    before = b.build_data(items, C)
    packed = b.build_packed(items)
    after = b.build_data(items, C)
    # build_data's RNG stream is undisturbed
    for name in ("starts", "paths", "ends", "labels"):
        assert np.array_equal(getattr(before, name), getattr(after, name))
    assert before.ids == after.ids

    assert packed.ids == [it.id for it in items]
    assert packed.starts.dtype == packed.paths.dtype == np.int32
    assert packed.ends.dtype == np.int32 and packed.lengths.dtype == np.int64
    assert int(packed.lengths.sum()) == packed.starts.shape[0] \
        == packed.paths.shape[0] == packed.ends.shape[0]
    assert packed.labels.tolist() == before.labels.tolist()

    mtok = r.terminal_vocab.stoi["@method_0"]
    q = r.QUESTION_TOKEN_INDEX
    segs = segments(packed)
    for it, (lo, hi) in zip(items, segs):
        pcs = np.asarray(it.path_contexts).reshape(-1, 3)
        if pcs.shape[0] == 0:
            # the zero-context item is one PAD row
            assert hi - lo == 1
            assert (packed.starts[lo], packed.paths[lo],
                    packed.ends[lo]) == (0, 0, 0)
            continue
        assert hi - lo == pcs.shape[0]       # nothing truncated
        want_s = np.where(pcs[:, 0] == mtok, q, pcs[:, 0])
        want_e = np.where(pcs[:, 2] == mtok, q, pcs[:, 2])
        assert np.array_equal(packed.starts[lo:hi], want_s)   # corpus order
        assert np.array_equal(packed.paths[lo:hi], pcs[:, 1])
        assert np.array_equal(packed.ends[lo:hi], want_e)
    assert int(packed.lengths[2]) == 3 * C
    assert packed.starts[segs[2][0]] == q    # the planted @method_0
    assert not np.any(packed.starts == mtok)
    assert not np.any(packed.ends == mtok)


def test_build_packed_variable_task_one_segment_per_alias(tiny_corpus):
    r = make_reader(tiny_corpus, infer_method=False, infer_variable=True)
    b = DatasetBuilder(r, make_option(r, max_path_length=2),
                       split_ratio=0.0, seed=5)
    # a method whose first @var alias touches 5 of its 7 contexts
    planted = copy.copy(r.items[0])
    alias0 = [a for a in planted.aliases if a.startswith("@var_")][0]
    v0 = r.terminal_vocab.stoi[alias0]
    planted.path_contexts = np.array(
        [[v0, 1, 5], [6, 2, 7], [8, 3, v0], [v0, 4, v0], [9, 5, 10],
         [11, 6, v0], [v0, 7, 12]], dtype=np.int32)
    items = [planted] + list(r.items[1:12])
    packed = b.build_packed(items)
    q = r.QUESTION_TOKEN_INDEX
    want_ids, want_labels, want_segs = [], [], []
    for it in items:
        for alias in [a for a in it.aliases if a.startswith("@var_")]:
            v = r.terminal_vocab.stoi[alias]
            pcs = np.asarray(it.path_contexts).reshape(-1, 3)
            sel = pcs[(pcs[:, 0] == v) | (pcs[:, 2] == v)].copy()
            sel[:, 0] = np.where(sel[:, 0] == v, q, sel[:, 0])
            sel[:, 2] = np.where(sel[:, 2] == v, q, sel[:, 2])
            if sel.shape[0] == 0:
                sel = np.zeros((1, 3), dtype=np.int32)
            want_ids.append(it.id)
            want_labels.append(r.label_vocab.stoi[it.aliases[alias]])
            want_segs.append(sel)
    assert len(want_segs) > 0
    assert packed.ids == want_ids
    assert packed.labels.tolist() == want_labels
    assert packed.lengths.tolist() == [s.shape[0] for s in want_segs]
    # untruncated: some alias has more than max_path_length = 2 contexts
    assert int(packed.lengths[0]) == 5
    assert packed.starts[:5].tolist() == [q, 8, q, 11, q]
    assert packed.paths[:5].tolist() == [1, 3, 4, 6, 7]
    assert packed.ends[:5].tolist() == [5, q, q, q, 12]
    flat = np.concatenate(want_segs, axis=0)
    assert np.array_equal(packed.starts, flat[:, 0])
    assert np.array_equal(packed.paths, flat[:, 1])
    assert np.array_equal(packed.ends, flat[:, 2])
    # the padded builder makes the same rows (one per alias)
    assert b.build_data(items, 2).ids == want_ids


# ---------------------------------------------------------------------------
# packed iterator


def packed_of(lengths):
    lengths = np.asarray(lengths, dtype=np.int64)
    M = int(lengths.sum())
    return PackedData(ids=list(range(100, 100 + len(lengths))),
                      starts=np.arange(1, M + 1, dtype=np.int32),
                      paths=np.arange(1, M + 1, dtype=np.int32) * 2,
                      ends=np.arange(1, M + 1, dtype=np.int32) * 3,
                      lengths=lengths,
                      labels=np.arange(len(lengths), dtype=np.int64))


def test_packed_iterator_budget_order_and_oversized():
    lengths = [3, 4, 2, 50, 1, 1, 9, 10, 10, 1]
    data = packed_of(lengths)
    it = PackedBatchIterator(data, 10)
    batches = list(it)
    assert len(batches) == len(it)
    got_lengths = [b["lengths"].tolist() for b in batches]
    assert got_lengths == [[3, 4, 2], [50], [1, 1], [9], [10], [10], [1]]
    for b in batches:
        n = b["lengths"].tolist()
        assert sum(n) <= 10 or len(n) == 1   # budget, or oversized alone
        assert b["starts"].shape == (sum(n),) == b["paths"].shape
        assert b["starts"].dtype == torch.int32
        assert b["lengths"].dtype == torch.int64
        assert not b["lengths"].is_cuda
    # every item exactly once, in input order; rows follow their method
    assert torch.cat([b["id"] for b in batches]).tolist() == data.ids
    assert torch.cat([b["label"] for b in batches]).tolist() \
        == data.labels.tolist()
    assert np.array_equal(torch.cat([b["starts"] for b in batches]).numpy(),
                          data.starts)
    assert np.array_equal(torch.cat([b["ends"] for b in batches]).numpy(),
                          data.ends)
    # a budget that holds everything: one batch; an empty set: none
    assert [b["lengths"].tolist()
            for b in PackedBatchIterator(data, 1000)] == [lengths]
    assert list(PackedBatchIterator(packed_of([]), 10)) == []
    with pytest.raises(ValueError):
        PackedBatchIterator(data, 0)


# ---------------------------------------------------------------------------
# the K21 oracle and forward_packed against the padded forms


def hand_pad(flat, lengths, width):
    """[B, width, ...] with method i's rows first, in order.  Index tensors
    are filled with 0 (PAD); a float tensor repeats the method's last row,
    as the pad rows of a real batch all hold the PAD row's vector."""
    out = torch.zeros((len(lengths), width) + tuple(flat.shape[1:]),
                      dtype=flat.dtype)
    lo = 0
    for i, n in enumerate(lengths):
        out[i, :n] = flat[lo:lo + n]
        if flat.is_floating_point():
            out[i, n:] = flat[lo + n - 1]
        lo += n
    return out


def test_reference_attention_pool_packed_matches_padded_attention():
    g = torch.Generator().manual_seed(3)
    E = 16
    lengths = [5, 1, 12, 7, 1]
    M = sum(lengths)
    ccv = torch.tanh(torch.randn(M, E, generator=g))
    a = torch.randn(E, generator=g) * 0.3
    starts = torch.randint(1, 50, (M,), generator=g, dtype=torch.int32)
    starts[2] = 0            # a masked row inside a segment
    starts[M - 1] = 0        # the single-PAD method
    cv, cvb, attn = R.attention_pool_packed(ccv, a, starts, lengths, E)
    width = max(lengths)
    p_ccv = hand_pad(ccv, lengths, width)
    p_starts = hand_pad(starts, lengths, width)
    mask = (p_starts > 0).float()
    want_attn = R.attention(p_ccv, a, mask)
    want_cv = R.code_vector(p_ccv, want_attn)
    torch.testing.assert_close(cv, want_cv)
    assert torch.equal(cvb, cv.to(torch.bfloat16))
    lo = 0
    for i, n in enumerate(lengths[:-1]):
        torch.testing.assert_close(attn[lo:lo + n], want_attn[i, :n])
        lo += n
    # one masked row: softmax over a single NINF is weight 1
    assert float(attn[M - 1]) == 1.0
    assert float(attn[2]) == 0.0
    # the functional entry point on CPU tensors is the oracle
    for x, y in zip(Fn.attention_pool_packed(ccv, a, starts, lengths, E),
                    (cv, cvb, attn)):
        assert torch.equal(x, y)
    for x, y in zip(Fn.attention_pool_packed(
            ccv, a, starts, torch.tensor(lengths, dtype=torch.int32), E),
            (cv, cvb, attn)):
        assert torch.equal(x, y)


def small_model(angular=False, **kw):
    opt = Option(terminal_count=60, path_count=50, label_count=24,
                 max_path_length=C, terminal_embed_size=8,
                 path_embed_size=8, encode_size=12, dropout_prob=0.25,
                 angular_margin_loss=angular, batch_size=4,
                 device=torch.device("cpu"), **kw)
    g = torch.Generator().manual_seed(5)
    return Code2VecTorch(opt, init_logical_params(opt, g)).eval()


def test_torch_forward_packed_matches_forward_on_hand_padded_inputs():
    model = small_model()
    g = torch.Generator().manual_seed(9)
    lengths = [3, C, 1, 2 * C + 5, 9]
    M = sum(lengths)
    s = torch.randint(1, 60, (M,), generator=g, dtype=torch.int32)
    p = torch.randint(1, 50, (M,), generator=g, dtype=torch.int32)
    e = torch.randint(1, 60, (M,), generator=g, dtype=torch.int32)
    outputs, cv, attn = model.forward_packed(s, p, e, lengths)
    assert outputs.shape == (5, 24) and cv.shape == (5, 12)
    assert attn.shape == (M,)
    width = max(lengths)
    with torch.no_grad():
        w_out, w_cv, w_attn = model(
            hand_pad(s, lengths, width), hand_pad(p, lengths, width),
            hand_pad(e, lengths, width), torch.zeros(5, dtype=torch.int64))
    torch.testing.assert_close(outputs, w_out)
    torch.testing.assert_close(cv, w_cv)
    lo = 0
    for i, n in enumerate(lengths):
        torch.testing.assert_close(attn[lo:lo + n], w_attn[i, :n])
        lo += n
    # inference only
    model.train()
    with pytest.raises(AssertionError):
        model.forward_packed(s, p, e, lengths)


# ---------------------------------------------------------------------------
# Predictor(all_contexts=True)


def predictions_equal(a, b, bitwise_ids=None):
    """Same ids, names and contexts; probabilities, attention and code
    vector torch.equal for the ids in ``bitwise_ids`` (default: all), close
    at float32 defaults for the rest."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        same = (torch.equal if bitwise_ids is None or x.id in bitwise_ids
                else lambda u, v: torch.testing.assert_close(u, v) is None)
        assert x.id == y.id
        assert [n for n, _ in x.names] == [n for n, _ in y.names]
        assert same(torch.tensor([p for _, p in x.names]),
                    torch.tensor([p for _, p in y.names]))
        assert [c[:3] for c in x.contexts] == [c[:3] for c in y.contexts]
        assert same(torch.tensor([c[3] for c in x.contexts]),
                    torch.tensor([c[3] for c in y.contexts]))
        assert same(x.code_vector, y.code_vector)


def test_all_contexts_independent_of_seed_and_neighbours(tiny_corpus):
    r = make_reader(tiny_corpus)
    opt = make_option(r)
    g = torch.Generator().manual_seed(2)
    model = Code2VecTorch(opt, init_logical_params(opt, g))
    big = long_item(r, 3 * C)
    empty = copy.copy(r.items[1])
    empty.path_contexts = np.empty((0, 3), dtype=np.int32)
    items = list(r.items[:5]) + [big, empty] + list(r.items[5:9])
    cpu = torch.device("cpu")

    def run(**kw):
        pr = Predictor(model, r, cpu, topk=3, top_contexts=4, batch_size=4,
                       all_contexts=True, **kw)
        return list(pr.predict_items(items))

    base = run(seed=1)
    assert [p.id for p in base] == [it.id for it in items]
    predictions_equal(base, run(seed=77))
    # Two other batch compositions.  The torch backend pads a batch to
    # its longest method, so a short method's padded width (and with it
    # the last bits of its sums) follows its neighbours; the 3*C bag is
    # the longest of any batch it joins and must not move at all.
    predictions_equal(base, run(seed=5, max_batch_contexts=7),
                      bitwise_ids={big.id})
    predictions_equal(base, run(seed=1, max_batch_contexts=10 ** 6),
                      bitwise_ids={big.id})
    # the whole bag was used: its contexts are the top 4 of all 3*C rows
    packed = DatasetBuilder(r, opt, split_ratio=0.0).build_packed([big])
    with torch.no_grad():
        _, cv, attn = model.forward_packed(
            torch.from_numpy(packed.starts), torch.from_numpy(packed.paths),
            torch.from_numpy(packed.ends), packed.lengths.tolist())
    order = sorted(range(3 * C), key=lambda c: (-float(attn[c]), c))[:4]
    got = base[5]
    assert [c[3] for c in got.contexts] == [float(attn[c]) for c in order]
    assert [c[1] for c in got.contexts] == [
        r.path_vocab.itos[int(packed.paths[c])] for c in order]
    assert torch.equal(got.code_vector, cv[0])
    # the padded path subsamples that bag: a different answer per seed
    # is what all_contexts removes; here only check it reports no PAD
    assert base[6].contexts == []            # zero-context method
    for p in base:
        assert all(s != "<PAD/>" for s, _, _, _ in p.contexts)
    with pytest.raises(ValueError):
        Predictor(model, r, cpu, all_contexts=True, max_batch_contexts=0)


# ---------------------------------------------------------------------------
# arguments and CLI


def test_lengths_errors_raise_before_anything_runs():
    ccv = torch.zeros(6, 32)
    a = torch.zeros(32)
    starts = torch.ones(6, dtype=torch.int32)
    for bad in ([3, 0, 3], [3, 2], [3, 4], [], [-1, 7],
                torch.tensor([2.0, 4.0])):
        with pytest.raises(ValueError):
            Fn.attention_pool_packed(ccv, a, starts, bad, 30)
        with pytest.raises(ValueError):
            R.attention_pool_packed(ccv, a, starts, bad, 30)
    model = small_model()
    idx = torch.ones(6, dtype=torch.int32)
    for bad in ([6, 0], [5], [4, 3]):
        with pytest.raises(ValueError):
            model.forward_packed(idx, idx, idx, bad)
    with pytest.raises(ValueError):
        Fn.attention_pool_packed(torch.zeros(2, 3, 32), a, starts, [6], 30)


def test_forward_packed_rejects_angular_margin_head():
    model = small_model(angular=True)
    idx = torch.ones(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="angular") as e:
        model.forward_packed(idx, idx, idx, [6])
    with pytest.raises(ValueError, match="angular") as e2:
        Predictor(model, None, torch.device("cpu"), all_contexts=True)
    assert str(e.value) == str(e2.value)


def test_cli_all_contexts_round_trip(tmp_path, tiny_corpus):
    ckpt = train_checkpoint(tmp_path, tiny_corpus)
    reader = make_reader(tiny_corpus)
    out_pad = tmp_path / "pad.jsonl"
    out_all = tmp_path / "all.jsonl"
    out_all2 = tmp_path / "all2.jsonl"
    argv = predict_argv(ckpt, tiny_corpus, tiny_corpus["corpus_path"], out_pad)
    assert predict_cli.main(argv) == 0
    argv[argv.index("--out") + 1] = str(out_all)
    assert predict_cli.main(argv + ["--all_contexts"]) == 0
    argv[argv.index("--out") + 1] = str(out_all2)
    assert predict_cli.main(argv + ["--all_contexts", "--random_seed", "9",
                                    "--with_vector"]) == 0
    rows_pad = [json.loads(x) for x in out_pad.read_text().splitlines()]
    rows = [json.loads(x) for x in out_all.read_text().splitlines()]
    rows2 = [json.loads(x) for x in out_all2.read_text().splitlines()]
    assert len(rows) == len(rows2) == 48
    assert [r["id"] for r in rows] == [it.id for it in reader.items]
    for r, r2, rp, it in zip(rows, rows2, rows_pad, reader.items):
        assert set(r) == set(rp) == {"id", "expected", "predictions",
                                     "contexts"}
        assert set(r2) == set(r) | {"vector"}
        assert r["expected"] == it.normalized_label
        assert len(r["predictions"]) == 5
        for p in r["predictions"]:
            assert set(p) == {"name", "prob"}
        assert 1 <= len(r["contexts"]) <= 5
        for c in r["contexts"]:
            assert set(c) == {"start", "path", "end", "attention"}
        # the seed changes nothing
        assert r2["predictions"] == r["predictions"]
        assert r2["contexts"] == r["contexts"]
        # no method of the tiny corpus exceeds max_path_length: the padded
        # path saw the same bags, in another (shuffled) order
        padded = {p["name"]: p["prob"] for p in rp["predictions"]}
        top = r["predictions"][0]
        assert top["name"] in padded
        assert abs(top["prob"] - padded[top["name"]]) <= 1e-4 * top["prob"]
    with pytest.raises(SystemExit) as e:
        predict_cli.main(argv + ["--all_contexts",
                                 "--max_batch_contexts", "0"])
    assert e.value.code == 2
