"""Seeded cases and the rule of the K24 (sim_range) tests; not a test file.

Integer data (entries in [-3, 3]: exact in bf16, sums <= 9 * 512 exact in
fp32) must equal the oracle ops/reference.py::sim_range bit for bit,
scores equal to the threshold included.

Random unit rows cannot be compared pair by pair where a score sits next
to the threshold: the kernel's fp32 summation order inside MFMA is not
torch's.  The rule compares against fp64 scores S = q.double() @
db.double().T of the same bf16 inputs with K20's tolerance

    tol = EP * 2^-23 * max_i |q_i| * max_j |db_j|

(tests/test_sim_topk_gpu.py derives it).  With t32 = fp32(t):
  1. the CSR is well formed: offsets[0] == 0, non-decreasing,
     offsets[-1] == len(rows) == len(scores);
  2. within a segment rows are strictly ascending, in [0, N), never
     exclude[i], always > after[i];
  3. |score - S[i, row]| <= tol and score >= t32;
  4. every allowed row with S >= t + tol is reported, and no reported row
     has S < t - tol.
Pairs with |S - t| < tol are open either way; BEFORE looking at the
kernel's output the helper asserts on the fp64 reference that at most 1 %
of the pairs with S >= t are such borderline pairs (a condition on the
case, not a measurement of the kernel).
"""

import torch

# nq, N, EP, threshold (exact in fp32).  Pairs with S >= t / borderline
# pairs of these seeded cases: 638 / 1, 2606 / 5, 32 / 0, 26 / 0, 10 / 0,
# 117 / 0, all 5100 / 0.
UNIT_SHAPES = [
    (37, 1000, 128, 0.1875),   # query tail + row tail
    (64, 20011, 128, 0.25),    # default nsplit > 1, odd N
    (5, 533, 320, 0.125),      # generic EP
    (3, 16, 32, 0.0),          # one tile, smallest EP
    (1, 17, 128, 0.0),         # one query, one row past a tile
    (20, 300, 512, 0.09375),   # largest EP
    (17, 300, 128, -2.0),      # every row of every query
]

# K20's integer shapes (tests/test_sim_topk_gpu.py) with a threshold each
INT_SHAPES = [
    (37, 1000, 128, 40.0), (64, 20011, 128, 96.0), (5, 533, 320, 60.0),
    (3, 16, 32, 0.0), (20, 300, 512, 100.0), (33, 4099, 128, 96.0),
]

_CASES = {}


def unit_case(nq, N, EP, dev="cpu"):
    """tests/test_sim_topk_gpu.py::unit_case's recipe: seeded unit-norm
    rows -> bf16 (q, db) on ``dev`` plus their fp64 score matrix on the
    CPU; computed once per shape, shared read-only."""
    key = (nq, N, EP, str(dev))
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


def int_case(nq, N, EP, dev="cpu", seed=0):
    g = torch.Generator().manual_seed(seed + nq + N + EP)
    q = torch.randint(-3, 4, (nq, EP), generator=g).to(torch.bfloat16)
    db = torch.randint(-3, 4, (N, EP), generator=g).to(torch.bfloat16)
    return q.to(dev), db.to(dev)


def allowed_mask(nq, N, exclude=None, after=None):
    cols = torch.arange(N).view(1, -1)
    ok = torch.ones(nq, N, dtype=torch.bool)
    if exclude is not None:
        ok &= cols != exclude.cpu().view(-1, 1)
    if after is not None:
        ok &= cols > after.cpu().view(-1, 1)
    return ok


def check_csr(offsets, rows, scores, nq, N, exclude=None, after=None):
    """Points 1 and 2 of the rule; returns the CPU triple and the query of
    every entry."""
    assert offsets.dtype == torch.int64 and offsets.shape == (nq + 1,)
    assert rows.dtype == torch.int64 and rows.dim() == 1
    assert scores.dtype == torch.float32 and scores.shape == rows.shape
    offsets, rows, scores = offsets.cpu(), rows.cpu(), scores.cpu()
    assert int(offsets[0]) == 0
    counts = offsets.diff()
    assert bool((counts >= 0).all())
    assert int(offsets[-1]) == rows.shape[0]
    qi = torch.repeat_interleave(torch.arange(nq), counts)
    assert bool(((rows >= 0) & (rows < N)).all())
    same = qi[1:] == qi[:-1]
    assert bool((rows.diff()[same] > 0).all())
    if exclude is not None:
        assert not bool((rows == exclude.cpu()[qi]).any())
    if after is not None:
        assert bool((rows > after.cpu()[qi]).all())
    return offsets, rows, scores, qi


def borderline_condition(S, tol, t, exclude=None, after=None):
    """The condition on the case: at most 1 % of the pairs with S >= t lie
    within tol of t.  Returns (pairs, borderline)."""
    ok = allowed_mask(*S.shape, exclude, after)
    pairs = int(((S >= t) & ok).sum())
    border = int((((S - t).abs() < tol) & ok).sum())
    assert border <= 0.01 * pairs, (pairs, border)
    return pairs, border


def check_range_rule(offsets, rows, scores, S, tol, t, exclude=None,
                     after=None, tag=""):
    """The rule of the module docstring; returns the largest
    |score - S[i, row]|."""
    nq, N = S.shape
    t32 = float(torch.tensor(t, dtype=torch.float32))
    pairs, border = borderline_condition(S, tol, t32, exclude, after)
    offsets, rows, scores, qi = check_csr(offsets, rows, scores, nq, N,
                                          exclude, after)
    ref = S[qi, rows]
    err = float((scores.double() - ref).abs().max()) if rows.numel() else 0.0
    print(f"sim_range {tag} nq={nq} N={N} t={t}: {pairs} pairs with S >= t, "
          f"{border} borderline, {rows.numel()} reported, max |score - fp64| "
          f"= {err:.3e}, tol = {tol:.3e}")
    assert err <= tol
    assert bool((scores >= t32).all())
    assert not bool((ref < t32 - tol).any())
    got = torch.zeros(nq, N, dtype=torch.bool)
    got[qi, rows] = True
    must = (S >= t32 + tol) & allowed_mask(nq, N, exclude, after)
    assert not bool((must & ~got).any())
    return err


def assert_csr_equal(a, b):
    """Two CSR triples agree bit for bit (scores compared as integers)."""
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype
    assert torch.equal(a[0].cpu(), b[0].cpu())
    assert torch.equal(a[1].cpu(), b[1].cpu())
    assert torch.equal(a[2].cpu().view(torch.int32),
                       b[2].cpu().view(torch.int32))


def clustered_int_index():
    """Integer vectors for a ``dot`` index of 96 rows, width 40 (EP = 64),
    with every score known by construction.  At threshold 120:
      - the family: rows 5, 9, 13, ..., 81 (20 rows) are identical,
        [2, -2] * 20 with self score 160 — more than any k <= 16 lists;
      - the pair: rows 30 and 90 are identical, all 2 (160), orthogonal to
        the family;
      - the chain: B = [2, 2, -2, -2] * 10 (row 50), A = B with columns
        0..7 zeroed (row 2), C = B with columns 8..15 zeroed (row 91), so
        A.B = B.C = 128 and A.C = 96 < 120; all three are orthogonal to
        the family and the pair;
      - every other row holds a single +-3 and scores at most 9 to
        anything.
    Returns (vectors f32 [96, 40], threshold, family, pair, chain)."""
    N, E = 96, 40
    v = torch.zeros(N, E)
    for r in range(N):
        v[r, r % E] = 3.0 if r % 2 else -3.0
    family = list(range(5, 82, 4))
    v[family] = torch.tensor([2.0, -2.0] * 20)
    pair = [30, 90]
    v[pair] = torch.full((E,), 2.0)
    B = torch.tensor([2.0, 2.0, -2.0, -2.0] * 10)
    A = B.clone()
    A[:8] = 0.0
    C = B.clone()
    C[8:16] = 0.0
    chain = [2, 50, 91]
    v[2], v[50], v[91] = A, B, C
    return v, 120.0, family, pair, chain
