"""Training on packed batches, the parts that need no GPU: the packing
mode of BatchIterator, the torch oracle's forward_packed_train, the host
check of the lengths, and the CLI end to end with --pack_batches."""

import json

import numpy as np
import pytest
import torch

import main as cli
from code2vec_amd.data.builder import EpochData
from code2vec_amd.engine.loader import BatchIterator, stripped_lengths
from code2vec_amd.models.code2vec import (
    Code2VecTorch, init_logical_params, logical_from_reference_state_dict,
)
from code2vec_amd.ops import functional as Fn
from code2vec_amd.utils.options import Option

C = 12


def _epoch_data(n=37, seed=3):
    """A padded epoch with ragged methods: row 0 is full, row 1 all PAD,
    row 2 has one context, row 3 a PAD hole inside its real contexts."""
    rng = np.random.default_rng(seed)
    starts = np.zeros((n, C), dtype=np.int32)
    paths = np.zeros((n, C), dtype=np.int32)
    ends = np.zeros((n, C), dtype=np.int32)
    lens = rng.integers(1, C + 1, size=n)
    lens[0], lens[1], lens[2], lens[3] = C, 0, 1, 6
    for i, k in enumerate(lens):
        starts[i, :k] = rng.integers(1, 50, size=k)
        paths[i, :k] = rng.integers(1, 40, size=k)
        ends[i, :k] = rng.integers(1, 50, size=k)
    starts[3, 2] = 0  # a hole: stays, only TRAILING pads are stripped
    labels = rng.integers(0, 9, size=n).astype(np.int64)
    want = lens.copy()
    want[1] = 1
    return EpochData(list(range(n)), starts, paths, ends, labels), want


def test_stripped_lengths():
    data, want = _epoch_data()
    got = stripped_lengths(data.starts)
    assert got.dtype == np.int64
    assert got.tolist() == want.tolist()
    assert got[1] == 1 and got[0] == C and got[3] == 6


@pytest.mark.parametrize("shuffle", [True, False])
def test_packed_iterator_matches_padded(shuffle):
    data, want = _epoch_data()
    bs = 8
    padded = BatchIterator(data, bs, shuffle=shuffle, seed=11)
    packed = BatchIterator(data, bs, shuffle=shuffle, seed=11, pack=True)
    assert len(padded) == len(packed) == 5
    assert packed.row_capacity == bs * C
    nb = 0
    for pb, kb in zip(padded, packed):
        nb += 1
        assert torch.equal(pb["id"], kb["id"])
        assert torch.equal(pb["label"], kb["label"])
        lens = kb["lengths"]
        assert lens.dtype == torch.int64 and not lens.is_cuda
        assert lens.tolist() == [int(want[i]) for i in pb["id"].tolist()]
        M = int(lens.sum())
        assert M <= packed.row_capacity
        for key in ("starts", "paths", "ends"):
            flat = kb[key]
            assert flat.dtype == torch.int32 and flat.shape == (M,)
            rows = [pb[key][r, :n] for r, n in enumerate(lens.tolist())]
            assert torch.equal(flat, torch.cat(rows))
            # what was stripped is all PAD
            for r, n in enumerate(lens.tolist()):
                assert int(pb["starts"][r, n:].abs().sum()) == 0
    assert nb == 5
    assert kb["label"].numel() == 37 - 4 * bs  # the tail batch is smaller


def test_packed_iterator_second_epoch_reshuffles_like_padded():
    data, _ = _epoch_data()
    padded = BatchIterator(data, 8, seed=5)
    packed = BatchIterator(data, 8, seed=5, pack=True)
    for _ in range(2):
        ids_a = torch.cat([b["id"] for b in padded])
        ids_b = torch.cat([b["id"] for b in packed])
        assert torch.equal(ids_a, ids_b)


def _tiny_model(dropout=0.0, angular=False):
    opt = Option(terminal_count=50, path_count=40, label_count=9,
                 max_path_length=C, terminal_embed_size=6, path_embed_size=5,
                 encode_size=7, dropout_prob=dropout,
                 angular_margin_loss=angular, device=torch.device("cpu"))
    g = torch.Generator().manual_seed(0)
    return Code2VecTorch(opt, init_logical_params(opt, g))


def test_oracle_forward_packed_train_matches_padded_forward():
    """Loss and every parameter gradient of forward_packed_train equal
    those of forward on the same methods padded to C (dropout 0)."""
    data, want = _epoch_data(n=8)
    assert {1, C} <= set(want.tolist())  # lengths 1 (incl. all-pad) and C
    packed = next(iter(BatchIterator(data, 8, shuffle=False, pack=True)))
    padded = next(iter(BatchIterator(data, 8, shuffle=False)))
    w = torch.ones(9)

    grads = []
    losses = []
    for mode in ("padded", "packed"):
        model = _tiny_model()
        model.train()
        if mode == "padded":
            out, cv, attn = model(padded["starts"], padded["paths"],
                                  padded["ends"], padded["label"])
        else:
            out, cv, attn = model.forward_packed_train(
                packed["starts"], packed["paths"], packed["ends"],
                packed["lengths"], packed["label"])
            assert attn.shape == (int(packed["lengths"].sum()),)
            assert out.shape == (8, 9) and cv.shape == (8, 7)
        loss = model.loss(out, padded["label"], w)
        loss.backward()
        losses.append(loss.detach())
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    torch.testing.assert_close(losses[1], losses[0])
    assert set(grads[0]) == set(grads[1])
    for k in grads[0]:
        torch.testing.assert_close(grads[1][k], grads[0][k], msg=k)


@pytest.mark.parametrize("lengths", [[3, 0, 2], [3, -1, 3], [3, 3], [2, 2, 2]])
def test_bad_lengths_raise_value_error(lengths):
    model = _tiny_model()
    model.train()
    s = torch.ones(5, dtype=torch.int32)
    y = torch.zeros(len(lengths), dtype=torch.int64)
    with pytest.raises(ValueError):
        model.forward_packed_train(s, s, s, lengths, y)
    with pytest.raises(ValueError):
        Fn.packed_offsets(lengths, 5, torch.device("cpu"))


def test_packed_offsets_builds_and_checks():
    lens, off = Fn.packed_offsets([2, 1, 3], 6, torch.device("cpu"))
    assert lens.tolist() == [2, 1, 3]
    assert off.dtype == torch.int32 and off.tolist() == [0, 2, 3, 6]
    with pytest.raises(ValueError):  # handed-in offsets of the wrong size
        Fn.packed_offsets([2, 1, 3], 6, torch.device("cpu"),
                          offsets=torch.zeros(3, dtype=torch.int32))


def test_forward_packed_still_asserts_in_training_mode():
    model = _tiny_model()
    model.train()
    s = torch.ones(5, dtype=torch.int32)
    with pytest.raises(AssertionError):
        model.forward_packed(s, s, s, [2, 3])


def test_pack_batches_rejected_for_data_parallel():
    from code2vec_amd.engine.trainer import Trainer, TrainerConfig
    from code2vec_amd.parallel.dist import DistContext

    class A:
        max_epoch = 1; lr = 0.01; beta_min = 0.9; beta_max = 0.999
        weight_decay = 0.0; model_path = "x"; vectors_path = "x"
        test_result_path = None; env = None; print_sample_cycle = 0
        eval_method = "subtoken"; random_seed = 1; batch_size = 4
        pack_batches = True

    cfg = TrainerConfig(A)
    assert cfg.pack_batches is True
    ctx = DistContext(0, 2, 0, torch.device("cpu"))
    with pytest.raises(ValueError, match="pack_batches"):
        Trainer(cfg, None, None, None, _tiny_model(), ctx)


def test_cli_pack_batches_end_to_end(tmp_path, tiny_corpus, capsys):
    """--pack_batches trains on the torch backend: the loss goes down and
    the exported checkpoint reloads."""
    assert cli.build_parser().parse_args([]).pack_batches is False
    out_dir = tmp_path / "out"
    cli.main([
        "--corpus_path", tiny_corpus["corpus_path"],
        "--path_idx_path", tiny_corpus["path_idx_path"],
        "--terminal_idx_path", tiny_corpus["terminal_idx_path"],
        "--model_path", str(out_dir),
        "--vectors_path", str(out_dir / "code.vec"),
        "--max_epoch", "4", "--batch_size", "16",
        "--terminal_embed_size", "12", "--path_embed_size", "12",
        "--encode_size", "16", "--max_path_length", "12",
        "--dropout_prob", "0.0",
        "--no_cuda", "--print_sample_cycle", "0", "--env", "floyd",
        "--pack_batches",
    ])
    out = capsys.readouterr().out
    losses = [json.loads(line)["value"] for line in out.splitlines()
              if line.startswith('{"metric": "train_loss"')]
    assert len(losses) == 4
    assert losses[-1] < losses[0], losses
    ctx_rate = [json.loads(line)["value"] for line in out.splitlines()
                if line.startswith('{"metric": "path_contexts_per_sec"')]
    assert len(ctx_rate) == 4 and all(v > 0 for v in ctx_rate)

    sd = torch.load(out_dir / "code2vec.model", weights_only=True)
    opt = Option(terminal_count=sd["terminal_embedding.weight"].shape[0],
                 path_count=sd["path_embedding.weight"].shape[0],
                 label_count=sd["output_linear.weight"].shape[0],
                 terminal_embed_size=12, path_embed_size=12, encode_size=16)
    m = Code2VecTorch(opt, logical_from_reference_state_dict(sd, opt))
    assert torch.equal(m.input_weight.detach(), sd["input_linear.weight"])
    assert (out_dir / "code.vec").exists()
