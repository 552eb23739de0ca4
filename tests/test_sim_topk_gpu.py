"""K20 sim_topk (fused similarity + top-k) on the GPU.

Random data cannot be compared index by index: the kernel's fp32 summation
order inside MFMA is not torch's, so where two scores nearly tie either
order is right.  The rule instead compares against fp64 scores
S = q.double() @ db.double().T of the same bf16 inputs with

    tol = EP * 2^-23 * max_i |q_i| * max_j |db_j|

the (n-1)*u bound for fp32 accumulation of exact products (bf16 x bf16 is
exact in fp32), u doubled to 2^-23 to cover a truncating adder; about
1.5e-5 at EP = 128 for unit rows.  For every query:
  1. indices distinct, in [0, N), not the excluded row;
  2. |vals[j] - S[i, idx[j]]| <= tol;
  3. vals non-increasing, equal values with ascending indices;
  4. |vals[j] - sortdesc(S[i])[j]| <= tol (nothing better was missed).
Integer-valued data (entries in [-3, 3]: exact in bf16, sums <= 1152 exact
in fp32) must equal the oracle ops/reference.py::sim_topk bit for bit; it
is tie-rich, so it pins the smallest-row rule.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.engine.similar import CodeVectorIndex
from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


_CASES = {}


def unit_case(nq, N, EP, dev):
    """Seeded unit-norm rows -> bf16 (q, db) on the device plus their fp64
    score matrix on the CPU; computed once per shape, shared read-only."""
    key = (nq, N, EP)
    if key not in _CASES:
        g = torch.Generator().manual_seed(100000 * nq + 7 * N + EP)
        q = torch.randn(nq, EP, generator=g)
        db = torch.randn(N, EP, generator=g)
        q = (q / q.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        db = (db / db.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        S = q.double() @ db.double().t()
        tol = EP * 2.0 ** -23 * float(q.double().norm(dim=1).max()) \
            * float(db.double().norm(dim=1).max())
        _CASES[key] = (q.to(dev), db.to(dev), S, tol)
    return _CASES[key]


def int_case(nq, N, EP, dev, seed=0):
    g = torch.Generator().manual_seed(seed + nq + N + EP)
    q = torch.randint(-3, 4, (nq, EP), generator=g).to(torch.bfloat16)
    db = torch.randint(-3, 4, (N, EP), generator=g).to(torch.bfloat16)
    return q.to(dev), db.to(dev)


def check_rule(vals, idx, S, tol, k, exclude=None, tag=""):
    """The four-point tolerance rule of the module docstring; returns the
    largest |vals - S[idx]|."""
    nq, N = S.shape
    assert vals.dtype == torch.float32 and vals.shape == (nq, k)
    assert idx.dtype == torch.int64 and idx.shape == (nq, k)
    vals = vals.cpu().double()
    idx = idx.cpu()
    S = S.clone()
    assert bool(((idx >= 0) & (idx < N)).all())
    assert bool((torch.sort(idx, dim=1).values.diff(dim=1) > 0).all()) \
        or k == 1
    if exclude is not None:
        ex = exclude.cpu()
        assert not bool((idx == ex[:, None]).any())
        rows = torch.nonzero(ex >= 0).flatten()
        S[rows, ex[rows]] = float("-inf")
    err = (vals - S.gather(1, idx)).abs().max().item()
    best = torch.sort(S, dim=1, descending=True).values[:, :k]
    miss = (vals - best).abs().max().item()
    print(f"sim_topk {tag} nq={nq} N={N} k={k}: max |val - fp64| = "
          f"{err:.3e}, max |val - best_j| = {miss:.3e}, tol = {tol:.3e}")
    assert err <= tol
    d = vals.diff(dim=1)
    assert bool((d <= 0).all())
    assert bool((idx.diff(dim=1)[d == 0] > 0).all())
    assert miss <= tol
    return err


# (37, 1000): query tail + row tail; (64, 20011): default nsplit > 1, odd
# N; (5, 533, 320): generic EP; (3, 16, 32): k == N, one tile, smallest EP
RULE_SHAPES = [(37, 1000, 128, 16), (64, 20011, 128, 16), (5, 533, 320, 5),
               (3, 16, 32, 16), (1, 17, 128, 1)]


@pytest.mark.parametrize("nq,N,EP,k", RULE_SHAPES)
def test_tolerance_rule(dev, nq, N, EP, k):
    q, db, S, tol = unit_case(nq, N, EP, dev)
    if (nq, N) == (64, 20011):
        assert Fn.sim_topk_default_nsplit(nq, N) > 1
    vals, idx = Fn.sim_topk(q, db, k)
    check_rule(vals, idx, S, tol, k, tag=f"EP={EP}")


@pytest.mark.parametrize("nq,N,EP,k,nsplit", [
    (37, 1000, 128, 16, None), (64, 20011, 128, 16, None),
    (5, 533, 320, 5, 2), (3, 16, 32, 16, None), (20, 300, 512, 7, 4),
    (33, 4099, 128, 10, 1)])
def test_integer_data_equals_oracle(dev, nq, N, EP, k, nsplit):
    q, db = int_case(nq, N, EP, dev)
    vals, idx = Fn.sim_topk(q, db, k, nsplit=nsplit)
    rv, ri = R.sim_topk(q, db, k)
    assert torch.equal(idx, ri)
    assert torch.equal(vals, rv)


@pytest.mark.parametrize("EP", [128, 64])
def test_identical_rows_return_arange(dev, EP):
    N, k = 5000, 16
    row = torch.randint(-3, 4, (EP,),
                        generator=torch.Generator().manual_seed(1))
    db = row.to(torch.bfloat16).repeat(N, 1).contiguous().to(dev)
    q = db[:3].contiguous()
    for nsplit in (None, 1, 5):
        vals, idx = Fn.sim_topk(q, db, k, nsplit=nsplit)
        assert torch.equal(idx, torch.arange(k, device=dev).repeat(3, 1))
        assert bool((vals == float((row * row).sum())).all())


@pytest.mark.parametrize("EP", [128, 96])
def test_duplicates_across_slice_boundaries(dev, EP):
    N, nsplit = 1000, 3
    rows = Fn.sim_topk_slice_rows(N, nsplit)
    assert rows % Fn.SIM_ROW_TILE == 0 and 2 * rows < N <= 3 * rows
    q, db = int_case(2, N, EP, dev, seed=9)
    planted = [0, rows - 1, rows, 2 * rows - 1, 2 * rows, N - 1]
    db[planted] = 3.0  # the best possible partner of an all-3 query
    q[0] = 3.0
    q[1] = -3.0
    vals, idx = Fn.sim_topk(q, db, len(planted), nsplit=nsplit)
    assert idx[0].tolist() == planted
    assert vals[0].tolist() == [9.0 * EP] * len(planted)
    rv, ri = R.sim_topk(q, db, 16)
    vals, idx = Fn.sim_topk(q, db, 16, nsplit=nsplit)
    assert torch.equal(idx, ri) and torch.equal(vals, rv)


@pytest.mark.parametrize("nq,N,EP", [(37, 1000, 128), (5, 533, 320),
                                     (1, 17, 128)])
def test_nsplit_does_not_change_bits(dev, nq, N, EP):
    q, db, _, _ = unit_case(nq, N, EP, dev)
    k = min(16, N)
    base = Fn.sim_topk(q, db, k, nsplit=1)
    for nsplit in (2, 7, None):
        got = Fn.sim_topk(q, db, k, nsplit=nsplit)
        assert torch.equal(got[0].view(torch.int32),
                           base[0].view(torch.int32))
        assert torch.equal(got[1], base[1])


@pytest.mark.parametrize("EP,nsplit", [(128, None), (320, 3)])
def test_exclude(dev, EP, nsplit):
    N, k = 700, 16
    _, db = int_case(1, N, EP, dev, seed=3)
    rows = torch.tensor([0, 5, 335, 336, 698, 699, 17, 250], device=dev)
    q = db[rows].contiguous()
    vals, idx = Fn.sim_topk(q, db, k, rows, nsplit=nsplit)
    rv, ri = R.sim_topk(q, db, k, rows)
    assert torch.equal(idx, ri) and torch.equal(vals, rv)
    assert not bool((idx == rows[:, None]).any())
    # without exclusion every query finds itself (or an equal row before it)
    v0, i0 = Fn.sim_topk(q, db, k, nsplit=nsplit)
    assert bool((i0 == rows[:, None]).any(dim=1).all())
    # -1 excludes nothing
    none = torch.full_like(rows, -1)
    v1, i1 = Fn.sim_topk(q, db, k, none, nsplit=nsplit)
    assert torch.equal(i1, i0) and torch.equal(v1, v0)
    # mixed: only the flagged queries lose their row
    mixed = torch.where(torch.arange(len(rows), device=dev) % 2 == 0, rows,
                        none)
    v2, i2 = Fn.sim_topk(q, db, k, mixed, nsplit=nsplit)
    r2 = R.sim_topk(q, db, k, mixed)
    assert torch.equal(i2, r2[1]) and torch.equal(v2, r2[0])


def test_exclude_tolerance_rule(dev):
    q, db, S, tol = unit_case(37, 1000, 128, dev)
    g = torch.Generator().manual_seed(11)
    ex = torch.randint(-1, 1000, (37,), generator=g)
    ex[0] = int(S[0].argmax())  # the best row itself is excluded
    vals, idx = Fn.sim_topk(q, db, 16, ex.to(dev))
    check_rule(vals, idx, S, tol, 16, exclude=ex, tag="exclude")


def test_bitwise_deterministic(dev):
    q, db, _, _ = unit_case(64, 20011, 128, dev)
    a = Fn.sim_topk(q, db, 16)
    b = Fn.sim_topk(q, db, 16)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1], b[1])


def test_hipgraph_capture_replay(dev):
    q, db, _, _ = unit_case(64, 20011, 128, dev)
    sq, sdb = q.clone(), db.clone()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        Fn.sim_topk(sq, sdb, 16)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = Fn.sim_topk(sq, sdb, 16)
    g = torch.Generator().manual_seed(77)
    fq = torch.randn(64, 128, generator=g).to(torch.bfloat16).to(dev)
    fdb = torch.randn(20011, 128, generator=g).to(torch.bfloat16).to(dev)
    sq.copy_(fq)
    sdb.copy_(fdb)
    graph.replay()
    torch.cuda.synchronize()
    eager = Fn.sim_topk(fq, fdb, 16)
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    assert not torch.equal(out[1], Fn.sim_topk(q, db, 16)[1])


@pytest.mark.parametrize("nq,N,EP,k", [(37, 1000, 128, 16),
                                       (5, 533, 320, 5)])
def test_fused_and_composed_agree(dev, nq, N, EP, k, monkeypatch):
    q, db, S, tol = unit_case(nq, N, EP, dev)
    fv, fi = Fn.sim_topk(q, db, k)
    cv, ci = Fn.sim_topk_composed(q, db, k)
    check_rule(cv, ci, S, tol, k, tag="composed")
    # both lie within tol of the same sorted fp64 scores
    assert float((fv - cv).abs().max()) <= 2 * tol
    # C2V_SIM_FUSED=0 routes the public op to the composed path
    monkeypatch.setattr(Fn, "_SIM_FUSED", False)
    rv, ri = Fn.sim_topk(q, db, k)
    assert torch.equal(rv, cv) and torch.equal(ri, ci)


def test_argument_errors(dev):
    q = torch.zeros(4, 64, dtype=torch.bfloat16, device=dev)
    db = torch.zeros(32, 64, dtype=torch.bfloat16, device=dev)
    err = (ValueError, RuntimeError)
    for k in (0, 17):
        with pytest.raises(err):
            Fn.sim_topk(q, db, k)
    with pytest.raises(err):
        Fn.sim_topk(q, db[:8].contiguous(), 9)  # k > N
    ex = torch.full((4,), -1, dtype=torch.int64, device=dev)
    with pytest.raises(err):
        Fn.sim_topk(q, db[:8].contiguous(), 8, ex)  # k == N with exclude
    with pytest.raises(err):
        Fn.sim_topk(q, db, 2, ex[:3])  # one exclude per query
    with pytest.raises(err):
        Fn.sim_topk(q[:, :48].contiguous(), db[:, :48].contiguous(), 2)
    with pytest.raises(err):
        Fn.sim_topk(q[:, :32], db[:, :32].contiguous(), 2)  # non-contiguous
    with pytest.raises(err):
        Fn.sim_topk(q, db[::2], 2)  # non-contiguous
    with pytest.raises(err):
        Fn.sim_topk(q.float(), db.float(), 2)  # fp32 on device
    with pytest.raises(err):
        Fn.sim_topk(q, db[:, :32].contiguous(), 2)  # mismatched EP
    with pytest.raises(err):
        Fn.sim_topk(q, db, 2, nsplit=0)
    with pytest.raises(err):
        Fn.sim_topk_composed(q.float(), db.float(), 2)


def test_code_vector_index_cuda_matches_cpu(dev):
    N, E, k = 3000, 100, 10  # EP = 128: 28 pad columns
    g = torch.Generator().manual_seed(21)
    v = torch.randn(N, E, generator=g)
    names = [f"m{i}" for i in range(N)]
    gpu = CodeVectorIndex(v, names, dev)
    cpu = CodeVectorIndex(v, names, "cpu")
    assert gpu.EP == 128 and gpu.matrix.is_cuda
    assert torch.equal(gpu.matrix.cpu(), cpu.matrix)
    assert bool((gpu.matrix[:, E:] == 0).all())
    queries = torch.randn(21, E, generator=g)
    qb = cpu._prepare(queries, "queries")
    S = qb.double() @ cpu.matrix.double().t()
    tol = gpu.EP * 2.0 ** -23 * float(qb.double().norm(dim=1).max()) \
        * float(cpu.matrix.double().norm(dim=1).max())
    scores, rows = gpu.search(queries, k)
    check_rule(scores, rows, S, tol, k, tag="index")
    cs, cr = cpu.search(queries, k)
    check_rule(cs, cr, S, tol, k, tag="index-cpu")
    assert float((scores.cpu() - cs).abs().max()) <= 2 * tol

    # a scaled copy of an index row finds that row first
    picks = [0, 1234, N - 1]
    s, r = gpu.search(v[picks] * 2.5, 3)
    assert r[:, 0].tolist() == picks and bool((s[:, 0] > 0.99).all())
    # de-duplication use: rows as queries never return themselves, and
    # otherwise see what a query with the row's own bits sees (scaling by
    # a power of two normalizes to the same bf16 row)
    s, r = gpu.search(v[picks] * 4.0, 3)
    assert r[:, 0].tolist() == picks
    s2, r2 = gpu.neighbors_of_rows(picks, 3)
    assert not bool((r2.cpu() == torch.tensor(picks)[:, None]).any())
    assert torch.equal(r2[:, :2], r[:, 1:]) \
        and torch.equal(s2[:, :2], s[:, 1:])
