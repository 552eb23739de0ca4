"""group_tables' two-level sort by LDS buckets (index_group.hip: count,
offsets, partition, finish) against numpy and against the global-atomic
chain it replaced (C2V_GROUP_SORT=0).

Every comparison is exact.  Shapes are the smallest that reach each path:
table sizes around the bucket size R, entry counts around the tile of the
count/partition kernels, one bucket looping over several tiles, one hot
row, a ragged batch, indices out of range, every value of the sweep
switches, and the packed path's capacity-sized scratch.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import ext
from code2vec_amd.ops import functional as Fn

R = 2048      # shipped rows per bucket (C2V_GROUP_R)
TILE = 4096   # shipped entries per count/partition block (C2V_GROUP_TILE)
GUARD = 16    # guard elements on both sides of every output buffer
FILL = -7
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _guarded(n, dtype, fill, dev):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n]


def _run(s, p, e, rows_t, rows_p, dev, tmp="own"):
    """ext().group_tables on guarded buffers; {tag: (sorted_idx, perm,
    counts, cursor)} as numpy, after checking that no guard changed.
    ``tmp``: "own" passes a guarded scratch, None lets the binding
    allocate."""
    st, pt, et = (torch.from_numpy(a).to(dev) for a in (s, p, e))
    M = s.size
    whole, view = {}, {}
    for tag, rows, n in (("term", rows_t, 2 * M), ("path", rows_p, M)):
        bufs = (_guarded(n, torch.int32, FILL, dev),
                _guarded(n, torch.int64, FILL, dev),
                _guarded(rows, torch.int32, 0, dev),
                _guarded(rows, torch.int32, FILL, dev))
        whole[tag] = [b[0] for b in bufs]
        view[tag] = [b[1] for b in bufs]
    spart = torch.empty(int(ext().group_tables_partials_len(rows_t, rows_p)),
                        dtype=torch.int32, device=dev)
    t, q = view["term"], view["path"]
    args = (st, pt, et, t[2], q[2], t[3], q[3], spart, t[0], t[1], q[0], q[1],
            rows_t, rows_p, False)
    if tmp == "own":
        n = int(ext().group_tables_tmp_len(M, rows_t, rows_p))
        gw, gv = _guarded(n, torch.int32, FILL, dev)
        assert ext().group_tables(*args, gv) is False
        g = gw.cpu().numpy()
        assert np.all(g[:GUARD] == FILL) and np.all(g[-GUARD:] == FILL)
    else:
        assert ext().group_tables(*args) is False
    out = {}
    for tag in whole:
        for k, (w, fill) in enumerate(zip(whole[tag], (FILL, FILL, 0, FILL))):
            a = w.cpu().numpy()
            assert np.all(a[:GUARD] == fill), (tag, k)
            assert np.all(a[-GUARD:] == fill), (tag, k)
        out[tag] = tuple(v.cpu().numpy() for v in view[tag])
    return out


def _check(rec, s, p, e, rows_t, rows_p):
    lists = {"term": (np.concatenate([s, e]).astype(np.int64), rows_t),
             "path": (p.astype(np.int64), rows_p)}
    for tag, (idx, rows) in lists.items():
        sorted_idx, perm, counts, cursor = rec[tag]
        kept = (idx >= 0) & (idx < rows)
        K = int(kept.sum())
        cnt = np.bincount(idx[kept], minlength=rows)
        assert np.array_equal(counts, cnt), tag
        assert np.array_equal(cursor, np.cumsum(cnt)), tag  # run END
        assert np.all(np.diff(sorted_idx[:K]) >= 0), tag
        assert np.array_equal(idx[perm[:K]], sorted_idx[:K]), tag
        assert np.array_equal(np.sort(perm[:K]), np.nonzero(kept)[0]), tag
        # dropped entries leave the tail untouched
        assert np.all(sorted_idx[K:] == FILL), tag
        assert np.all(perm[K:] == FILL), tag


def _same_records(a, b):
    for tag in a:
        for k in (0, 2, 3):
            assert np.array_equal(a[tag][k], b[tag][k]), (tag, k)
        # perm: the same set of entries in every run
        for rec in (a, b):
            assert np.array_equal(rec[tag][0] >= 0, rec[tag][1] >= 0)
        oa = np.lexsort((a[tag][1], a[tag][0]))
        ob = np.lexsort((b[tag][1], b[tag][0]))
        assert np.array_equal(a[tag][1][oa], b[tag][1][ob]), tag


def _both_chains(monkeypatch, s, p, e, rows_t, rows_p, dev):
    monkeypatch.delenv("C2V_GROUP_SORT", raising=False)
    new = _run(s, p, e, rows_t, rows_p, dev)
    _check(new, s, p, e, rows_t, rows_p)
    monkeypatch.setenv("C2V_GROUP_SORT", "0")
    old = _run(s, p, e, rows_t, rows_p, dev)
    _check(old, s, p, e, rows_t, rows_p)
    monkeypatch.delenv("C2V_GROUP_SORT")
    _same_records(new, old)
    return new


def _uniform(rng, M, rows_t, rows_p):
    return (rng.integers(0, rows_t, M).astype(np.int32),
            rng.integers(0, rows_p, M).astype(np.int32),
            rng.integers(0, rows_t, M).astype(np.int32))


def _ragged(rng, M, rows_t, rows_p):
    """half of all entries index 0, a few hundred index 1, the rest
    uniform; starts and ends differ, so entry numbers on both sides of M
    land in every kind of run"""
    s, p, e = _uniform(rng, M, rows_t, rows_p)
    for a in (s, p, e):
        where = rng.permutation(M)
        a[where[:M // 2]] = 0
        a[where[M // 2:M // 2 + 300]] = 1
    return s, p, e


@pytest.mark.parametrize("rows_t,rows_p", [(R - 1, 3), (R, R + 1),
                                           (R + 1, 2 * R + 1), (2 * R + 1, R),
                                           (3, R - 1)])
def test_table_sizes_around_the_bucket(dev, monkeypatch, rows_t, rows_p):
    """bucket edges, a last partial bucket, a table smaller than one bucket
    and, with a few hundred entries over thousands of rows, empty buckets"""
    s, p, e = _uniform(np.random.default_rng(rows_t), 150, rows_t, rows_p)
    # the rows on both sides of every bucket edge are hit
    s[:4] = [0, 1, 2, rows_t - 1]
    e[:3] = [min(R - 1, rows_t - 1), min(R, rows_t - 1), rows_t - 1]
    p[:4] = [0, min(R - 1, rows_p - 1), min(R, rows_p - 1), rows_p - 1]
    _both_chains(monkeypatch, s, p, e, rows_t, rows_p, dev)


@pytest.mark.parametrize("where", ["one_bucket", "one_row"])
@pytest.mark.parametrize("M", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_entry_counts_around_the_tile(dev, monkeypatch, M, where):
    """the path list has M entries and the term list 2M: both sides of a
    tile edge, and one bucket (or one row, index 3) taking all of them so
    that its finish block loops over several tiles"""
    rows_t, rows_p = 2 * R + 1, 3 * R
    rng = np.random.default_rng(M)
    if where == "one_bucket":
        s, p, e = (rng.integers(R, 2 * R, M).astype(np.int32)
                   for _ in range(3))
    else:
        s, p, e = (np.full(M, 3, dtype=np.int32) for _ in range(3))
    _both_chains(monkeypatch, s, p, e, rows_t, rows_p, dev)


def test_ragged_batch(dev, monkeypatch):
    M, rows_t, rows_p = 3000, 2 * R + 1, R + 5
    s, p, e = _ragged(np.random.default_rng(1), M, rows_t, rows_p)
    rec = _both_chains(monkeypatch, s, p, e, rows_t, rows_p, dev)
    perm0 = rec["term"][1][:rec["term"][2][0]]  # row 0's run
    assert (perm0 < M).any() and (perm0 >= M).any()


def test_out_of_range_indices_are_dropped(dev, monkeypatch):
    M, rows_t, rows_p = 1500, R + 1, 2 * R + 1
    rng = np.random.default_rng(2)
    s, p, e = _ragged(rng, M, rows_t, rows_p)
    for a, rows in ((s, rows_t), (p, rows_p), (e, rows_t)):
        where = rng.permutation(M)
        a[where[:40]] = -1
        a[where[40:80]] = rows
        a[where[80:120]] = INT_MAX
        a[where[120:130]] = -INT_MAX - 1
    _both_chains(monkeypatch, s, p, e, rows_t, rows_p, dev)


@pytest.mark.parametrize("tile", [1024, 2048, 4096])
@pytest.mark.parametrize("r", [1024, 2048, 4096])
def test_every_sweep_setting(dev, monkeypatch, r, tile):
    M, rows_t, rows_p = 4100, 2 * 4096 + 1, 4096 + 1
    s, p, e = _ragged(np.random.default_rng(3), M, rows_t, rows_p)
    s[:3] = [r - 1, r, rows_t - 1]
    monkeypatch.setenv("C2V_GROUP_R", str(r))
    monkeypatch.setenv("C2V_GROUP_TILE", str(tile))
    _check(_run(s, p, e, rows_t, rows_p, dev), s, p, e, rows_t, rows_p)


def test_binding_allocates_without_scratch(dev):
    M, rows_t, rows_p = 700, R + 1, 2 * R + 1
    s, p, e = _ragged(np.random.default_rng(4), M, rows_t, rows_p)
    _check(_run(s, p, e, rows_t, rows_p, dev, tmp=None), s, p, e, rows_t,
           rows_p)


def test_packed_capacity_scratch_serves_two_row_counts(dev, monkeypatch):
    """_launch_table_grouping with a row capacity: one capacity-sized
    scratch, handed over as views, for two different M in a row"""
    T, P, cap = 2 * R + 40, R + 7, 3 * TILE
    term_w = torch.zeros(T, 8, dtype=torch.bfloat16, device=dev,
                         requires_grad=True)
    path_w = torch.zeros(P, 8, dtype=torch.bfloat16, device=dev,
                         requires_grad=True)
    monkeypatch.setattr(Fn, "_grouping_applies", lambda *a: True)
    monkeypatch.setattr(Fn, "_GROUP_TABLES", True)
    monkeypatch.setattr(Fn, "_GROUP_STREAM", False)
    rng = np.random.default_rng(5)
    try:
        for M in (2 * TILE + 3, TILE - 9):
            s, p, e = _ragged(rng, M, T + 1, P + 1)
            st, pt, et = (torch.from_numpy(a).to(dev) for a in (s, p, e))
            assert Fn._launch_table_grouping(st, pt, et, term_w, path_w,
                                             row_capacity=cap) is not None
            g = Fn._group_state["outstanding"]
            rec = {}
            for tag, n in (("term", 2 * M), ("path", M)):
                sorted_idx, perm, counts, cursor = g.tables[tag]
                assert sorted_idx.numel() == n and perm.numel() == n
                rec[tag] = (sorted_idx.cpu().numpy(), perm.cpu().numpy(),
                            counts.cpu().numpy(), cursor.cpu().numpy())
            lists = {"term": (np.concatenate([s, e]), T + 1),
                     "path": (p, P + 1)}
            for tag, (idx, rows) in lists.items():
                sorted_idx, perm, counts, cursor = rec[tag]
                cnt = np.bincount(idx, minlength=rows)
                assert np.array_equal(counts, cnt), tag
                assert np.array_equal(cursor, np.cumsum(cnt)), tag
                assert np.all(np.diff(sorted_idx) >= 0), tag
                assert np.array_equal(idx[perm], sorted_idx), tag
                assert np.array_equal(np.sort(perm), np.arange(idx.size)), tag
            Fn.retire_table_grouping()
        keys = [k for k in Fn._scratch_cache
                if k[0] == "i32" and k[1] == "gtmp_cap"]
        assert len(keys) == 1
    finally:
        Fn.retire_table_grouping()
