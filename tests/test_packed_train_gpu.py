"""Training on packed batches on the GPU: forward_packed_train against the
torch oracle and against the padded HIP path, the fused table Adam, bitwise
determinism, the retire path of the forward-time grouping, bounded scratch,
pad regions, and the Trainer with pack_batches."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.data.synthetic import synthetic_batch
from code2vec_amd.engine.loader import stripped_lengths
from code2vec_amd.engine.optim import FusedAdam
from code2vec_amd.models.code2vec import (
    Code2VecHIP, Code2VecTorch, init_logical_params,
)
from code2vec_amd.ops import functional as Fn
from code2vec_amd.parallel.ddp import BucketedAllReduce
from code2vec_amd.utils.options import Option

C = 20
DIMS = [(100, 100, 100), (72, 40, 160)]   # EP = 128 (fused node), EP = 160


def relerr(a, b):
    a = a.float(); b = b.float()
    n = b.norm()
    return float((a - b).norm() / n) if float(n) > 0 else float((a - b).norm())


def make_option(dt=100, dp=100, E=100, **kw):
    d = dict(terminal_count=300, path_count=250, label_count=50,
             max_path_length=C, terminal_embed_size=dt, path_embed_size=dp,
             encode_size=E, dropout_prob=0.0, batch_size=8)
    d.update(kw)
    return Option(**d)


def make_batch(opt, B, dev, seed=0, lens=None):
    """(padded s, p, e [B, C], packed s, p, e [M], lengths, label): ragged
    methods, by default including lengths 1 and C and an all-pad row."""
    rng = np.random.default_rng(seed)
    s, p, e, y = synthetic_batch(rng, B, C, opt.terminal_count,
                                 opt.path_count, opt.label_count, full=True)
    if lens is None:
        lens = rng.integers(1, C + 1, size=B)
        lens[0], lens[1] = C, 1
        if B > 2:
            lens[2] = 0    # all pad: one PAD context once packed
    pad = np.arange(C)[None, :] >= np.asarray(lens)[:, None]
    s[pad] = 0; p[pad] = 0; e[pad] = 0
    n = stripped_lengths(s)
    real = np.arange(C)[None, :] < n[:, None]
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return ((to(s), to(p), to(e)), (to(s[real]), to(p[real]), to(e[real])),
            torch.from_numpy(n), to(y))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("dt,dp,E", DIMS)
def test_packed_loss_and_grads_match_oracle(dev, dt, dp, E):
    opt = make_option(dt, dp, E)
    logical = init_logical_params(opt, torch.Generator().manual_seed(4))
    hip = Code2VecHIP(opt, logical, device=dev).train()
    ref = Code2VecTorch(opt, logical).to(dev).train()
    _, (s, p, e), lens, y = make_batch(opt, 8, dev, seed=2)
    w = torch.ones(opt.label_count, device=dev)

    out_h, cv_h, attn_h = hip.forward_packed_train(s, p, e, lens, y)
    assert out_h.shape == (8, 50) and cv_h.shape == (8, E)
    assert attn_h.shape == (int(lens.sum()),)
    loss_h = hip.loss(out_h, y, w)
    loss_h.backward()
    out_r, _, attn_r = ref.forward_packed_train(s.long(), p.long(), e.long(),
                                                lens, y)
    loss_r = ref.loss(out_r, y, w)
    loss_r.backward()

    lh, lr = float(loss_h.detach()), float(loss_r.detach())
    assert abs(lh - lr) / lr < 2e-2
    assert relerr(hip.attention_a.grad[:E], ref.attention_a.grad) < 6e-2
    assert relerr(hip.ln_gamma.grad[:E], ref.ln_gamma.grad) < 6e-2
    assert relerr(hip.output_bias.grad, ref.output_bias.grad) < 6e-2
    assert relerr(hip.output_weight.grad[:, :E], ref.output_weight.grad) < 6e-2


@pytest.mark.parametrize("dt,dp,E", DIMS)
def test_packed_matches_padded_hip(dev, dt, dp, E):
    """Two HIP paths over the same methods at dropout 0; only summation
    orders differ (bounds of test_fused_gather_combiner_matches_unfused)."""
    opt = make_option(dt, dp, E)
    logical = init_logical_params(opt, torch.Generator().manual_seed(7))
    (s, p, e), (fs, fp, fe), lens, y = make_batch(opt, 8, dev, seed=5)
    w = torch.ones(opt.label_count, device=dev)
    res = []
    for packed in (False, True):
        m = Code2VecHIP(opt, logical, device=dev).train()
        if packed:
            out, _, _ = m.forward_packed_train(fs, fp, fe, lens, y)
        else:
            out, _, _ = m(s, p, e, y)
        loss = m.loss(out, y, w)
        loss.backward()
        res.append((float(loss), m.terminal_embedding.grad.clone(),
                    m.path_embedding.grad.clone(), m.input_weight.grad.clone(),
                    m.ln_gamma.grad.clone()))
    (l0, tg0, pg0, wg0, gg0), (l1, tg1, pg1, wg1, gg1) = res
    assert abs(l0 - l1) / abs(l0) < 1e-3
    # the PAD row included: a masked context's gradient is exactly zero, and
    # the all-pad method's C uniform rows add up to its one packed PAD row
    assert relerr(tg1, tg0) < 2e-2
    assert relerr(pg1, pg0) < 2e-2
    assert relerr(wg1, wg0) < 2e-2
    assert relerr(gg1, gg0) < 2e-2


def _steps(m, ddp, optim, batches, w, owned, cap):
    losses = []
    for (fs, fp, fe), lens, y in batches:
        ddp.zero_grad()
        out, _, _ = m.forward_packed_train(fs, fp, fe, lens, y,
                                           row_capacity=cap)
        loss = m.loss(out, y, w)
        loss.backward()
        if owned:
            ddp.finish_and_step(optim)
        else:
            ddp.finish()
            optim.step()
        losses.append(loss.detach().float().cpu())
    return losses


def test_finish_and_step_matches_plain_step_packed(dev):
    opt = make_option()
    logical = init_logical_params(opt, torch.Generator().manual_seed(21))
    w = torch.ones(opt.label_count, device=dev)
    batches = [make_batch(opt, 8, dev, seed=50 + i)[1:] for i in range(3)]
    finals = []
    for mode in ("plain", "owned"):
        m = Code2VecHIP(opt, logical, device=dev).train()
        owned = ([m.terminal_embedding, m.path_embedding]
                 if mode == "owned" else None)
        ddp = BucketedAllReduce(list(m.parameters()), 1, owned_params=owned,
                                owned_chunks=3)
        optim = FusedAdam(m.parameters(), lr=0.01)
        _steps(m, ddp, optim, batches, w, mode == "owned", 8 * C)
        finals.append({n: q.detach().float().cpu()
                       for n, q in m.named_parameters()})
        ddp.close()
    for name in finals[0]:
        assert torch.equal(finals[0][name], finals[1][name]), name


@pytest.mark.parametrize("dt,dp,E", DIMS)
def test_packed_training_bitwise_deterministic(dev, dt, dp, E):
    opt = make_option(dt, dp, E, dropout_prob=0.25)
    logical = init_logical_params(opt, torch.Generator().manual_seed(31))
    w = torch.ones(opt.label_count, device=dev)
    batches = [make_batch(opt, 8, dev, seed=60 + i)[1:] for i in range(5)]

    def run():
        Fn.reseed_dropout_rng(77)
        m = Code2VecHIP(opt, logical, device=dev).train()
        ddp = BucketedAllReduce(
            list(m.parameters()), 1,
            owned_params=[m.terminal_embedding, m.path_embedding])
        optim = FusedAdam(m.parameters(), lr=0.01)
        losses = _steps(m, ddp, optim, batches, w, True, 8 * C)
        ddp.close()
        return losses, {n: q.detach().float().cpu().clone()
                        for n, q in m.named_parameters()}

    (la, a), (lb, b) = run(), run()
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def _histograms():
    return [v for k, v in Fn._scratch_cache.items()
            if k[0] == "i32" and str(k[1]).startswith("counts_")]


def test_forward_without_backward_retires_the_grouping(dev):
    opt = make_option()
    m = Code2VecHIP(opt, device=dev).train()
    ddp = BucketedAllReduce(
        list(m.parameters()), 1,
        owned_params=[m.terminal_embedding, m.path_embedding])
    optim = FusedAdam(m.parameters(), lr=0.01)
    w = torch.ones(opt.label_count, device=dev)
    try:
        (fs, fp, fe), lens, y = make_batch(opt, 8, dev, seed=1)[1:]
        m.forward_packed_train(fs, fp, fe, lens, y, row_capacity=8 * C)
        assert Fn._group_state["outstanding"] is not None
        (fs, fp, fe), lens, y = make_batch(opt, 6, dev, seed=2)[1:]
        m.forward_packed_train(fs, fp, fe, lens, y, row_capacity=8 * C)
        Fn.retire_table_grouping()
        hist = _histograms()
        assert hist
        for h in hist:
            assert int(h.abs().sum()) == 0
        # and a full step after it still works and leaves them zero
        _steps(m, ddp, optim, [((fs, fp, fe), lens, y)], w, True, 8 * C)
        for h in _histograms():
            assert int(h.abs().sum()) == 0
    finally:
        ddp.close()


def test_scratch_cache_is_bounded_over_distinct_row_counts(dev):
    opt = make_option()
    m = Code2VecHIP(opt, device=dev).train()
    ddp = BucketedAllReduce(
        list(m.parameters()), 1,
        owned_params=[m.terminal_embedding, m.path_embedding])
    optim = FusedAdam(m.parameters(), lr=0.01)
    w = torch.ones(opt.label_count, device=dev)
    try:
        seen, sizes = set(), []
        for i in range(12):
            lens = [C] * 4 + [i + 1] + [1] * 3       # 12 distinct M
            batch = make_batch(opt, 8, dev, seed=100 + i, lens=lens)[1:]
            seen.add(int(batch[1].sum()))
            _steps(m, ddp, optim, [batch], w, True, 8 * C)
            sizes.append(len(Fn._scratch_cache))
        assert len(seen) == 12
        assert sizes[1] == sizes[11], sizes
        with pytest.raises(ValueError):   # more rows than the capacity
            (fs, fp, fe), lens, y = batch
            m.forward_packed_train(fs, fp, fe, lens, y, row_capacity=10)
    finally:
        Fn.retire_table_grouping()
        ddp.close()


@pytest.mark.parametrize("dt,dp,E", DIMS)
def test_pad_regions_stay_zero_after_packed_steps(dev, dt, dp, E):
    opt = make_option(dt, dp, E, dropout_prob=0.25)
    hip = Code2VecHIP(opt, device=dev).train()
    optim = FusedAdam(hip.parameters(), lr=0.01)
    w = torch.ones(opt.label_count, device=dev)
    for i in range(3):
        (fs, fp, fe), lens, y = make_batch(opt, 8, dev, seed=10 + i)[1:]
        optim.zero_grad()
        out, _, _ = hip.forward_packed_train(fs, fp, fe, lens, y)
        hip.loss(out, y, w).backward()
        optim.step()
    assert torch.all(hip.terminal_embedding.detach()[:, dt:].float() == 0)
    assert torch.all(hip.path_embedding.detach()[:, dp:].float() == 0)
    assert torch.all(hip.input_weight.detach()[E:, :].float() == 0)
    assert torch.all(hip.output_weight.detach()[:, E:].float() == 0)
    assert torch.all(hip.ln_gamma.detach()[E:] == 0)
    assert torch.all(hip.attention_a.detach()[E:] == 0)
    TS, PS = hip.TS, hip.PS
    assert torch.all(hip.input_weight.detach()[:, dt:TS].float() == 0)
    assert torch.all(hip.input_weight.detach()[:, TS + dp:TS + PS].float() == 0)
    for q in hip.parameters():
        assert bool(torch.isfinite(q.detach().float()).all())


def test_bad_lengths_raise_before_any_launch(dev):
    opt = make_option()
    m = Code2VecHIP(opt, device=dev).train()
    s = torch.ones(5, dtype=torch.int32, device=dev)
    y = torch.zeros(2, dtype=torch.int64, device=dev)
    for lens in ([5, 0], [6, -1], [2, 2]):
        with pytest.raises(ValueError):
            m.forward_packed_train(s, s, s, lens, y)
    assert Fn._group_state["outstanding"] is None


def test_trainer_pack_batches_epoch_gpu(dev, tmp_path):
    from code2vec_amd.data.builder import DatasetBuilder
    from code2vec_amd.data.reader import CorpusReader
    from code2vec_amd.data.synthetic import SyntheticSpec, write_synthetic_corpus
    from code2vec_amd.engine.trainer import Trainer, TrainerConfig
    from code2vec_amd.models.code2vec import build_model
    from code2vec_amd.parallel.dist import DistContext

    files = write_synthetic_corpus(
        str(tmp_path / "data"),
        SyntheticSpec(n_methods=60, n_terminals=300, n_paths=200,
                      max_contexts=20, seed=11),
    )
    reader = CorpusReader(files["corpus_path"], files["path_idx_path"],
                          files["terminal_idx_path"])
    opt = Option(terminal_count=len(reader.terminal_vocab),
                 path_count=len(reader.path_vocab),
                 label_count=len(reader.label_vocab),
                 max_path_length=16, terminal_embed_size=100,
                 path_embed_size=100, encode_size=100, dropout_prob=0.25,
                 batch_size=16, device=dev)
    builder = DatasetBuilder(reader, opt, seed=3)
    model = build_model(opt, backend="hip",
                        logical=init_logical_params(
                            opt, torch.Generator().manual_seed(2)),
                        device=dev)
    ctx = DistContext(0, 1, 0, dev)

    class A:
        max_epoch = 1; lr = 0.01; beta_min = 0.9; beta_max = 0.999
        weight_decay = 0.0; model_path = str(tmp_path / "out")
        vectors_path = str(tmp_path / "out" / "code.vec")
        test_result_path = None
        env = None; print_sample_cycle = 0
        eval_method = "subtoken"; random_seed = 3; batch_size = 16
        pack_batches = True

    trainer = Trainer(TrainerConfig(A), opt, reader, builder, model, ctx)
    try:
        losses, rows = [], []
        for epoch in range(4):
            loss, n = trainer._train_epoch(epoch)
            losses.append(loss)
            rows.append(n)
        assert losses[-1] < losses[0], losses
        # real rows, not batch_size * max_path_length per step
        n_train = len(builder.refresh_train_dataset(0))
        assert 0 < rows[0] <= n_train * 16
        loader = trainer._make_loader(train=False, epoch=0)
        stats = trainer.evaluate(loader)   # evaluation stays padded
        assert np.isfinite(stats[0])
    finally:
        pending = trainer._next_train
        if pending is not None:
            pending[1].result()
            trainer._next_train = None
        trainer._build_pool.shutdown(wait=True)
        trainer.ddp.close()
