"""group_tables: both embedding tables' counting sort in one chain of
launches, run at forward time (optionally on a side stream) and adopted by
the backward.

Record contents are checked against numpy, the records against
``_group_by_index`` records through the table Adam, and the forward-time
flow against the per-table chain inside backward at model level.  Wherever
runs of more than two entries meet, gradients are small integers (exact in
bf16 and in any fp32 summation order), so within-run order cannot matter
and every comparison is bitwise.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import ext, round_up
from code2vec_amd.ops import functional as Fn

LR, B1, B2, EPS, WD = 0.01, 0.9, 0.999, 1e-8, 0.01


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _group_tables(starts, paths, ends, T, P):
    """ext().group_tables on fresh buffers, on the current stream; returns
    {tag: (sorted_idx, perm, counts, cursor)}."""
    dev = starts.device
    M = starts.numel()
    out = {}
    for tag, rows, n in (("term", T + 1, 2 * M), ("path", P + 1, M)):
        out[tag] = (torch.full((n,), -7, dtype=torch.int32, device=dev),
                    torch.full((n,), -7, dtype=torch.int64, device=dev),
                    torch.zeros(rows, dtype=torch.int32, device=dev),
                    torch.full((rows,), -7, dtype=torch.int32, device=dev))
    spart = torch.empty(int(ext().group_tables_partials_len(T + 1, P + 1)),
                        dtype=torch.int32, device=dev)
    t, p = out["term"], out["path"]
    on_side = ext().group_tables(starts, paths, ends, t[2], p[2], t[3], p[3],
                                 spart, t[0], t[1], p[0], p[1], T + 1, P + 1,
                                 False)
    assert on_side is False
    return out


def _index_case(case, rng):
    """(starts, paths, ends int32 [B, C], T, P)"""
    if case == "tiny":
        B, C, T, P = 3, 5, 7, 5
    elif case == "edges":
        B, C, T, P = 7, 37, 300, 211  # M = 259, term N = 518
    elif case.startswith("scan"):
        B, C, T, P = 7, 37, int(case[4:]) - 1, 2
    elif case == "halfpad":
        B, C, T, P = 16, 40, 300, 211
    elif case == "same":
        B, C, T, P = 7, 37, 300, 211
    s = rng.integers(0, T, size=(B, C)).astype(np.int32)
    p = rng.integers(0, P, size=(B, C)).astype(np.int32)
    e = rng.integers(0, T, size=(B, C)).astype(np.int32)
    if case == "halfpad":
        # ragged batch: the second half of every row is <PAD/>, and index
        # 1 is a heavy hitter in both tables
        s[:, C // 2:] = p[:, C // 2:] = e[:, C // 2:] = 0
        s[:, :6] = 1
        e[:, 2:9] = 1
        p[:, :7] = 1
        assert (np.concatenate([s.ravel(), e.ravel()]) == 1).sum() \
            > Fn._TABLE_ADAM_HEAVY
        assert (p == 1).sum() > Fn._TABLE_ADAM_HEAVY
    if case == "same":
        s[:] = 3
        e[:] = 3
        p[:] = 3
    return s, p, e, T, P


@pytest.mark.parametrize("case", ["tiny", "edges", "scan1023", "scan1024",
                                  "scan1025", "halfpad", "same"])
def test_record_contents_match_numpy(dev, case):
    s, p, e, T, P = _index_case(case, np.random.default_rng(7))
    rec = _group_tables(*(torch.from_numpy(a).to(dev) for a in (s, p, e)),
                        T, P)
    lists = {"term": (np.concatenate([s.ravel(), e.ravel()]), T + 1),
             "path": (p.ravel(), P + 1)}
    for tag, (idx, rows) in lists.items():
        sorted_idx, perm, counts, cursor = (a.cpu().numpy() for a in rec[tag])
        N = idx.size
        cnt = np.bincount(idx, minlength=rows)
        assert np.array_equal(counts, cnt), tag
        assert np.array_equal(cursor, np.cumsum(cnt)), tag  # run END
        assert np.all(np.diff(sorted_idx) >= 0), tag
        assert np.array_equal(idx[perm], sorted_idx), tag
        assert np.array_equal(np.sort(perm), np.arange(N)), tag


def _adam_state(p0, dev):
    T, S = p0.shape
    return dict(p=p0.clone(), master=p0.float().view(-1).clone(),
                m=torch.zeros(T * S, device=dev),
                v=torch.zeros(T * S, device=dev),
                scratch=torch.zeros(T, S, device=dev))


def _step_one_table(st, rec, gout, bc_pow, M, KP, off0, off1, keep_counts):
    sorted_idx, perm, counts, cursor = rec
    op = (ext().adam_table_bf16_keep_counts if keep_counts
          else ext().adam_table_bf16)
    op(st["p"], gout, perm, counts, cursor, st["scratch"], st["master"],
       st["m"], st["v"], bc_pow, M, KP, off0, off1, Fn._TABLE_ADAM_HEAVY, LR,
       B1, B2, EPS, WD)


def test_records_match_group_by_index_through_table_adam(dev):
    """old: _group_by_index records, per-table launches; new: group_tables
    records, per-table launches; merged: group_tables records, one pre-pass
    and one clear for both tables."""
    s0, p0_, e0, T, P = _index_case("halfpad", np.random.default_rng(3))
    B, C = s0.shape
    M = B * C
    TS, PS = 104, 40
    KP = round_up(2 * TS + PS, 32)
    rows = {"term": T, "path": P}
    width = {"term": TS, "path": PS}
    offs = {"term": (0, TS + PS), "path": (TS, TS)}
    thr = Fn._TABLE_ADAM_HEAVY
    gen = torch.Generator(device=dev).manual_seed(5)
    rng = np.random.default_rng(11)
    init = {tag: (torch.randn(rows[tag], width[tag], generator=gen,
                              device=dev) * 0.1).to(torch.bfloat16)
            for tag in rows}
    sides = {side: {tag: _adam_state(init[tag], dev) for tag in rows}
             for side in ("old", "new", "merged")}
    bc_pow = torch.ones(2, dtype=torch.float64, device=dev)
    for step in range(2):
        s, p, e = (rng.permutation(a.ravel()).reshape(a.shape)
                   for a in (s0, p0_, e0))
        st_, pt_, et_ = (torch.from_numpy(a).to(dev) for a in (s, p, e))
        gout = torch.randint(-4, 5, (M, KP), generator=gen,
                             device=dev).to(torch.bfloat16)
        ext().adam_tick(bc_pow, B1, B2)
        lists = {"term": torch.cat([st_.view(-1), et_.view(-1)]),
                 "path": pt_.view(-1)}
        # old
        for tag in rows:
            rec = Fn._group_by_index(lists[tag], rows[tag], with_cursor=True)
            st = sides["old"][tag]
            ext().embed_scatter_heavy(rec[0], rec[1], rec[2], gout,
                                      st["scratch"], M, KP, *offs[tag], thr)
            _step_one_table(st, rec, gout, bc_pow, M, KP, *offs[tag], False)
            assert int(rec[2].abs().sum()) == 0
        # new records, per-table launches
        recs = _group_tables(st_, pt_, et_, T, P)
        for tag in rows:
            rec = recs[tag]
            st = sides["new"][tag]
            ext().embed_scatter_heavy(rec[0], rec[1], rec[2], gout,
                                      st["scratch"], M, KP, *offs[tag], thr)
            _step_one_table(st, rec, gout, bc_pow, M, KP, *offs[tag], False)
            assert int(rec[2].abs().sum()) == 0
        # new records, merged pre-pass and merged clear
        recs = _group_tables(st_, pt_, et_, T, P)
        t, q = recs["term"], recs["path"]
        mt, mp = sides["merged"]["term"], sides["merged"]["path"]
        ext().embed_scatter_heavy_pair(t[0], t[1], t[2], mt["scratch"], q[0],
                                       q[1], q[2], mp["scratch"], gout, M, KP,
                                       thr)
        _step_one_table(mt, t, gout, bc_pow, M, KP, *offs["term"], True)
        _step_one_table(mp, q, gout, bc_pow, M, KP, *offs["path"], True)
        assert int(t[2].sum()) == 2 * M and int(q[2].sum()) == M
        ext().clear_i32_pair(t[2], q[2])
        assert int(t[2].abs().sum()) == 0 and int(q[2].abs().sum()) == 0
        for side in sides.values():
            for st in side.values():
                assert float(st["scratch"].abs().sum()) == 0.0
    for tag in rows:
        for name in ("p", "master", "m", "v"):
            assert torch.equal(sides["old"][tag][name],
                               sides["new"][tag][name]), (tag, name)
            assert torch.equal(sides["old"][tag][name],
                               sides["merged"][tag][name]), (tag, name)
        assert not torch.equal(sides["merged"][tag]["p"], init[tag])


# ---------------------------------------------------------------------------
# model level

def _rows_at_most_twice(rng, n, count):
    """n indices in [1, count), no value more than twice."""
    pool = np.concatenate([np.arange(1, count), np.arange(1, count)])
    return rng.permutation(pool)[:n].astype(np.int32)


@pytest.fixture(scope="module")
def tiny(dev):
    from code2vec_amd.models.code2vec import init_logical_params
    from code2vec_amd.utils.options import Option

    opt = Option(terminal_count=3000, path_count=2500, label_count=700,
                 max_path_length=40, terminal_embed_size=100,
                 path_embed_size=100, encode_size=100, dropout_prob=0.0,
                 batch_size=32)
    logical = init_logical_params(opt, torch.Generator().manual_seed(21))
    rng = np.random.default_rng(55)
    B, C = 16, opt.max_path_length
    batches = []
    for _ in range(4):
        # two-term fp32 sums commute: with no non-PAD row more than twice
        # per table (starts and ends together) every grouping order gives
        # the same bits
        se = _rows_at_most_twice(rng, 2 * B * C, opt.terminal_count)
        s = se[: B * C].reshape(B, C).copy()
        e = se[B * C:].reshape(B, C).copy()
        p = _rows_at_most_twice(rng, B * C, opt.path_count).reshape(B, C)
        p = p.copy()
        # ragged tails: all-PAD contexts
        lens = rng.integers(C // 2, C + 1, size=B)
        pad = np.arange(C)[None, :] >= lens[:, None]
        assert pad.any()
        s[pad] = p[pad] = e[pad] = 0
        y = rng.integers(0, opt.label_count, size=B).astype(np.int64)
        batches.append(tuple(torch.from_numpy(a).to(dev)
                             for a in (s, p, e, y)))
    w = torch.ones(opt.label_count, device=dev)
    return opt, logical, batches, w


def _make(opt, logical, dev):
    from code2vec_amd.engine.optim import FusedAdam
    from code2vec_amd.models.code2vec import Code2VecHIP
    from code2vec_amd.parallel.ddp import BucketedAllReduce

    m = Code2VecHIP(opt, logical, device=dev).train()
    ddp = BucketedAllReduce(
        list(m.parameters()), 1,
        owned_params=[m.terminal_embedding, m.path_embedding],
        owned_chunks=3, fuse_owned_step=True)
    assert ddp.fuse_owned_step
    optim = FusedAdam(m.parameters(), lr=0.01, weight_decay=0.01)
    return m, ddp, optim


def _forward(m, batch, w):
    s, p, e, y = batch
    out, _, _ = m(s, p, e, y)
    return m.loss(out, y, w)


def _full_step(m, ddp, optim, batch, w):
    ddp.zero_grad()
    _forward(m, batch, w).backward()
    ddp.finish_and_step(optim)


def _snapshot(m, optim):
    snap = {n: q.detach().clone() for n, q in m.named_parameters()}
    for n, q in m.named_parameters():
        st = optim.state[q]
        for k in ("m", "v", "master"):
            if st[k] is not None:
                snap[f"{n}.{k}"] = st[k].clone()
    return snap


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), name


def _assert_invariants():
    """histograms, flags and the fp32 scatter scratch all-zero, and no
    grouping left outstanding"""
    torch.cuda.synchronize()
    seen = 0
    for key, buf in Fn._scratch_cache.items():
        if (key[0] in ("term", "path") or key[0] == "flags"
                or (key[0] == "i32" and key[1].startswith("counts_"))):
            assert float(buf.float().abs().sum()) == 0.0, key
            seen += 1
    assert seen >= 2
    assert Fn._group_state["outstanding"] is None


MODES = {"per_table": (False, False), "inline": (True, False),
         "side": (True, True)}


def _set_mode(monkeypatch, mode):
    tables, stream = MODES[mode]
    monkeypatch.setattr(Fn, "_GROUP_TABLES", tables)
    monkeypatch.setattr(Fn, "_GROUP_STREAM", stream)


def _train(tiny, dev, monkeypatch, mode, steps):
    opt, logical, batches, w = tiny
    _set_mode(monkeypatch, mode)
    tickets0 = Fn._group_state["next_ticket"]
    m, ddp, optim = _make(opt, logical, dev)
    for i in range(steps):
        _full_step(m, ddp, optim, batches[i % len(batches)], w)
    snap = _snapshot(m, optim)
    ddp.close()
    _assert_invariants()
    # the mode under test is the one that ran
    launched = Fn._group_state["next_ticket"] - tickets0
    assert launched == (steps if MODES[mode][0] else 0)
    return snap


def test_model_steps_equal_across_modes(tiny, dev, monkeypatch):
    snaps = {mode: _train(tiny, dev, monkeypatch, mode, 3) for mode in MODES}
    _assert_same(snaps["per_table"], snaps["inline"])
    _assert_same(snaps["per_table"], snaps["side"])


def test_side_stream_matches_inline_over_20_steps(tiny, dev, monkeypatch):
    """a missing wait between the streams shows up as a stale or
    half-written grouping within a few steps"""
    _assert_same(_train(tiny, dev, monkeypatch, "inline", 20),
                 _train(tiny, dev, monkeypatch, "side", 20))


@pytest.mark.parametrize("mode", ["inline", "side"])
@pytest.mark.parametrize("disturbance", ["forward_only", "two_forwards",
                                         "backward_no_step"])
def test_unadopted_grouping_is_retired(tiny, dev, monkeypatch, mode,
                                       disturbance):
    opt, logical, batches, w = tiny
    _set_mode(monkeypatch, mode)
    snaps = []
    for disturb in (True, False):
        m, ddp, optim = _make(opt, logical, dev)
        if disturb:
            ddp.zero_grad()
            if disturbance == "forward_only":
                _forward(m, batches[1], w)
                assert Fn._group_state["outstanding"] is not None
            elif disturbance == "two_forwards":
                _forward(m, batches[1], w)
                _forward(m, batches[2], w).backward()
            else:
                _forward(m, batches[1], w).backward()
                ddp.zero_grad()  # no optimizer step for that backward
                _assert_invariants()
        _full_step(m, ddp, optim, batches[0], w)
        snaps.append(_snapshot(m, optim))
        ddp.close()
        _assert_invariants()
    _assert_same(snaps[0], snaps[1])


def test_no_grouping_without_a_backward_to_come(tiny, dev, monkeypatch):
    opt, logical, batches, w = tiny
    _set_mode(monkeypatch, "side")
    m, ddp, optim = _make(opt, logical, dev)
    tickets0 = Fn._group_state["next_ticket"]
    with torch.no_grad():
        _forward(m, batches[0], w)
    m.eval()
    _forward(m, batches[0], w)
    m.train()
    assert Fn._group_state["next_ticket"] == tickets0
    assert Fn._group_state["outstanding"] is None
    _forward(m, batches[0], w)
    assert Fn._group_state["next_ticket"] == tickets0 + 1
    ddp.close()  # retires it
    _assert_invariants()
