"""Row-gathering table Adam (adam_table_bf16 + embed_scatter_heavy) and the
deferred table-gradient flow, checked BITWISE against the dense path
(embed_scatter_sorted + cast_clear_rows + adam_step_bf16).

Where the dense path has no fixed fp32 addition order (runs over more than
two 16-entry chunks of the sorted order: boundary partials meet in atomics)
the gradients are small integers, exact in bf16 and in any fp32 summation
order, so both paths must still agree bit for bit.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import ext
from code2vec_amd.ops import functional as Fn

T_ROWS = 301  # not a multiple of 64
LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _indices(case, M, N, rng):
    """int32 [N] row indices of one table (N = M, or 2M for start|end)."""
    if case == "same":
        return np.full(N, 5, dtype=np.int32)
    idx = rng.integers(0, T_ROWS, size=N).astype(np.int32)
    if case == "heavy":
        # one row far above the heavy threshold, plus PAD entries
        pos = rng.permutation(N)
        idx[pos[: Fn._TABLE_ADAM_HEAVY + 36]] = 7
        idx[pos[Fn._TABLE_ADAM_HEAVY + 36: Fn._TABLE_ADAM_HEAVY + 86]] = 0
    return idx


def _gout(case, M, KP, dev, gen):
    if case == "uniform":
        return torch.randn(M, KP, generator=gen, device=dev).to(torch.bfloat16)
    g = torch.randint(-4, 5, (M, KP), generator=gen, device=dev)
    return g.to(torch.bfloat16)


@pytest.mark.parametrize("case,M", [("uniform", 701), ("heavy", 701),
                                    ("same", 701), ("sparse", 5)])
@pytest.mark.parametrize("form", ["term", "path"])
@pytest.mark.parametrize("S,KP", [(104, 320), (8, 32)])
def test_table_adam_matches_dense_path_bitwise(dev, S, KP, form, case, M):
    T = T_ROWS
    if form == "term":
        N, off0, off1 = 2 * M, 0, 2 * S
    else:
        N, off0, off1 = M, S, S
    thr = Fn._TABLE_ADAM_HEAVY
    rng = np.random.default_rng(1234)
    gen = torch.Generator(device=dev).manual_seed(99)
    for wd in (0.0, 0.01):
        p0 = (torch.randn(T, S, generator=gen, device=dev) * 0.1).to(
            torch.bfloat16)
        st = {}
        for side in ("old", "new"):
            st[side] = dict(
                p=p0.clone(), master=p0.float().view(-1).clone(),
                m=torch.zeros(T * S, device=dev),
                v=torch.zeros(T * S, device=dev),
                scratch=torch.zeros(T, S, device=dev))
        flags = torch.zeros(T, dtype=torch.uint8, device=dev)
        bc_pow = torch.ones(2, dtype=torch.float64, device=dev)
        comparable = torch.ones(T, dtype=torch.bool)
        for _ in range(2):
            idx_np = _indices(case, M, N, rng)
            cnt = np.bincount(idx_np, minlength=T)
            if case == "uniform":
                # randn grads: only runs of at most two chunks have a
                # fixed addition order on the dense path (realized
                # maximum with this seed: 15 entries, nothing excluded)
                touched = cnt > 0
                excluded = cnt > 17
                assert excluded.sum() <= 0.05 * touched.sum()
                comparable &= torch.from_numpy(~excluded)
            if case == "heavy":
                assert cnt[7] > thr
            gout = _gout(case, M, KP, dev, gen)
            idx = torch.from_numpy(idx_np).to(dev)
            sorted_idx, perm, counts, cursor = Fn._group_by_index(
                idx, T, with_cursor=True)
            ext().adam_tick(bc_pow, B1, B2)
            # dense path
            o = st["old"]
            counts_old = counts.clone()
            dense = torch.empty(T, S, dtype=torch.bfloat16, device=dev)
            ext().embed_scatter_sorted(sorted_idx, perm, gout, o["scratch"],
                                       dense, flags, M, KP, off0, off1, 16)
            ext().cast_clear_rows(o["scratch"], counts_old, flags, dense)
            Fn.adam_step(o["p"], dense, o["master"], o["m"], o["v"], bc_pow,
                         LR, B1, B2, EPS, wd)
            # row-gathering path
            n = st["new"]
            ext().embed_scatter_heavy(sorted_idx, perm, counts, gout,
                                      n["scratch"], M, KP, off0, off1, thr)
            ext().adam_table_bf16(n["p"], gout, perm, counts, cursor,
                                  n["scratch"], n["master"], n["m"], n["v"],
                                  bc_pow, M, KP, off0, off1, thr, LR, B1, B2,
                                  EPS, wd)
            assert int(counts.abs().sum()) == 0
            assert int(counts_old.abs().sum()) == 0
            assert int(flags.sum()) == 0
            assert float(n["scratch"].abs().sum()) == 0.0
            assert float(o["scratch"].abs().sum()) == 0.0
        rows = comparable.to(dev)
        for name in ("p", "master", "m", "v"):
            a = st["old"][name].view(T, S)[rows]
            b = st["new"][name].view(T, S)[rows]
            assert torch.equal(a, b), (name, wd)
        # the step did something: touched rows moved
        assert not torch.equal(st["new"]["p"], p0)


# ---------------------------------------------------------------------------
# model level

def _tiny_setup(dev, seed=55):
    from code2vec_amd.data.synthetic import synthetic_batch
    from code2vec_amd.models.code2vec import init_logical_params
    from code2vec_amd.utils.options import Option

    opt = Option(terminal_count=3000, path_count=2500, label_count=700,
                 max_path_length=40, terminal_embed_size=100,
                 path_embed_size=100, encode_size=100, dropout_prob=0.0,
                 batch_size=32)
    logical = init_logical_params(opt, torch.Generator().manual_seed(21))
    rng = np.random.default_rng(seed)
    batches = []
    for _ in range(2):
        arrs = synthetic_batch(rng, 16, opt.max_path_length,
                               opt.terminal_count, opt.path_count,
                               opt.label_count)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in arrs))
    w = torch.ones(opt.label_count, device=dev)
    return opt, logical, batches, w


def _make(opt, logical, dev, fuse):
    from code2vec_amd.engine.optim import FusedAdam
    from code2vec_amd.models.code2vec import Code2VecHIP
    from code2vec_amd.parallel.ddp import BucketedAllReduce

    m = Code2VecHIP(opt, logical, device=dev).train()
    ddp = BucketedAllReduce(
        list(m.parameters()), 1,
        owned_params=[m.terminal_embedding, m.path_embedding],
        owned_chunks=3, fuse_owned_step=fuse)
    assert ddp.fuse_owned_step == fuse
    optim = FusedAdam(m.parameters(), lr=0.01, weight_decay=0.01)
    return m, ddp, optim


def _backward(m, batch, w):
    s, p, e, y = batch
    out, _, _ = m(s, p, e, y)
    m.loss(out, y, w).backward()


def _snapshot(m, optim):
    snap = {n: q.detach().clone() for n, q in m.named_parameters()}
    for n, q in m.named_parameters():
        st = optim.state[q]
        for k in ("m", "v", "master"):
            if st[k] is not None:
                snap[f"{n}.{k}"] = st[k].clone()
    return snap


def _assert_scatter_invariants():
    """counts, flags and the fp32 scatter scratch are all-zero between
    steps, whichever path consumed them."""
    seen = 0
    for key, buf in Fn._scratch_cache.items():
        if (key[0] in ("term", "path")
                or key[0] == "flags"
                or (key[0] == "i32" and key[1].startswith("counts_"))):
            assert float(buf.float().abs().sum()) == 0.0, key
            seen += 1
    assert seen >= 2  # at least the two histograms exist after a backward


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), name


def test_fused_owned_step_matches_dense_owned_step(dev):
    opt, logical, batches, w = _tiny_setup(dev)
    snaps = []
    for fuse in (True, False):
        m, ddp, optim = _make(opt, logical, dev, fuse)
        for i in range(3):
            ddp.zero_grad()
            _backward(m, batches[i % 2], w)
            ddp.finish_and_step(optim)
        snaps.append(_snapshot(m, optim))
        ddp.close()
        _assert_scatter_invariants()
    _assert_same(snaps[0], snaps[1])


def test_finish_materializes_deferred_grad(dev):
    opt, logical, batches, w = _tiny_setup(dev)
    grads = []
    for fuse in (True, False):
        m, ddp, optim = _make(opt, logical, dev, fuse)
        ddp.zero_grad()
        _backward(m, batches[0], w)
        ddp.finish()
        grads.append((m.terminal_embedding.grad.clone(),
                      m.path_embedding.grad.clone()))
        ddp.close()
        _assert_scatter_invariants()
    assert grads[0][0].dtype == torch.bfloat16
    assert float(grads[0][0].float().abs().sum()) > 0
    assert torch.equal(grads[0][0], grads[1][0])
    assert torch.equal(grads[0][1], grads[1][1])


def test_abandoned_deferred_backward_leaves_no_trace(dev):
    opt, logical, batches, w = _tiny_setup(dev)
    snaps = []
    for abandon in (True, False):
        m, ddp, optim = _make(opt, logical, dev, True)
        if abandon:
            ddp.zero_grad()
            _backward(m, batches[1], w)
            ddp.zero_grad()  # no optimizer step for that backward
            _assert_scatter_invariants()
        ddp.zero_grad()
        _backward(m, batches[0], w)
        ddp.finish_and_step(optim)
        snaps.append(_snapshot(m, optim))
        ddp.close()
        _assert_scatter_invariants()
    _assert_same(snaps[0], snaps[1])
