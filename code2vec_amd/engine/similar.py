"""Nearest-neighbour search over exported code vectors.

``CodeVectorIndex`` holds one code vector per method as a bf16 matrix on
the search device and answers "which methods are most like this one?"
with the K20 ``sim_topk`` kernel (ops/csrc/sim_topk.hip): the queries are
scored against the whole index and the k best rows selected without the
[nq, N] score matrix ever being written.  On the CPU the same call goes
through ops/reference.py::sim_topk.

The index is built from a ``code.vec`` file (engine/export.py's format),
from any [N, E] float matrix, or from a file written by ``save``.
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from ..ops import functional as Fn
from ..ops import reference as R

METRICS = ("cosine", "dot")
MAX_K = R.ROW_TOPK_MAX_K
DEFAULT_MAX_PAIRS = R.SIM_RANGE_MAX_PAIRS
_EPS = 1e-12  # keeps a zero vector zero under cosine normalization
_FORMAT = "code2vec_amd.CodeVectorIndex.v1"


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def read_code_vec(path: str) -> Tuple[List[str], torch.Tensor]:
    """Parse a ``code.vec`` file into (names, vectors f32 [N, E]).

    The header is ``count\\tencode_size``; the count is NOT a reliable
    number of rows that follow (the format's quirk, kept by
    engine/export.py: it is the corpus size, whatever is appended after
    it), so the rows are counted.  Each row is
    ``name\\tv0 v1 ...``; a row whose width differs from the header's
    encode_size is a ValueError naming the line."""
    names: List[str] = []
    rows: List[List[float]] = []
    with open(path, encoding="utf-8") as f:
        header = f.readline().rstrip("\n").split("\t")
        try:
            E = int(header[1])
        except (IndexError, ValueError):
            raise ValueError(
                f"{path}: line 1 is not a 'count\\tencode_size' header")
        if E < 1:
            raise ValueError(f"{path}: line 1 gives encode_size {E}")
        for lineno, line in enumerate(f, start=2):
            line = line.rstrip("\n")
            if not line.strip():
                continue
            name, sep, rest = line.partition("\t")
            if not sep:
                raise ValueError(
                    f"{path}: line {lineno} has no tab between name and "
                    f"vector")
            try:
                vec = [float(t) for t in rest.split()]
            except ValueError:
                raise ValueError(
                    f"{path}: line {lineno} has a non-numeric component")
            if len(vec) != E:
                raise ValueError(
                    f"{path}: line {lineno} has {len(vec)} components, the "
                    f"header says {E}")
            names.append(name)
            rows.append(vec)
    vectors = (torch.tensor(rows, dtype=torch.float32) if rows
               else torch.zeros(0, E, dtype=torch.float32))
    return names, vectors


class CodeVectorIndex:
    """A searchable set of code vectors.

    vectors: [N, E] float; names: N strings; metric ``cosine`` L2-normalizes
    rows in fp32 (a zero vector stays zero), ``dot`` stores them as given.
    Rows are zero-padded to EP = round_up(E, 32) and kept as bf16 on
    ``device``.  Queries get the same treatment, so a score is the fp32 dot
    product of two bf16 rows."""

    def __init__(self, vectors: torch.Tensor, names: Sequence[str],
                 device, metric: str = "cosine"):
        if metric not in METRICS:
            raise ValueError(
                f"metric must be one of {METRICS}, got {metric!r}")
        vectors = torch.as_tensor(vectors)
        if vectors.dim() != 2 or not vectors.is_floating_point():
            raise ValueError(
                f"vectors must be a float [N, E] matrix, got "
                f"{tuple(vectors.shape)} {vectors.dtype}")
        N, E = vectors.shape
        if N < 1 or E < 1:
            raise ValueError(f"empty index: vectors are {N} x {E}")
        if len(names) != N:
            raise ValueError(
                f"{len(names)} names for {N} vectors")
        if _round_up(E, 32) > R.SIM_TOPK_MAX_EP:
            raise ValueError(
                f"vector width {E} exceeds the supported "
                f"{R.SIM_TOPK_MAX_EP}")
        self.metric = metric
        self.device = torch.device(device)
        self.E = int(E)
        self.EP = _round_up(self.E, 32)
        self.names = list(names)
        self.matrix = self._prepare(vectors, "vectors")

    # -- construction ------------------------------------------------------
    def _prepare(self, x: torch.Tensor, what: str) -> torch.Tensor:
        """[n, E] float -> normalized, padded bf16 [n, EP] on the device.

        The arithmetic runs where ``x`` lives and only the finished bf16
        rows move, so vectors read from a file give the same bits whatever
        the search device."""
        x = torch.as_tensor(x)
        if x.dim() != 2 or x.shape[1] != self.E:
            raise ValueError(
                f"{what} must be [n, {self.E}], got {tuple(x.shape)}")
        x = x.to(torch.float32)
        if not bool(torch.isfinite(x).all()):
            raise ValueError(f"{what} contain non-finite values")
        if self.metric == "cosine":
            x = x / x.norm(dim=1, keepdim=True).clamp_min(_EPS)
        out = torch.zeros(x.shape[0], self.EP, dtype=torch.bfloat16,
                          device=x.device)
        out[:, :self.E] = x.to(torch.bfloat16)
        return out.to(self.device)

    @classmethod
    def from_code_vec(cls, path: str, device, metric: str = "cosine"):
        names, vectors = read_code_vec(path)
        if not names:
            raise ValueError(f"{path}: no vector rows")
        return cls(vectors, names, device, metric=metric)

    def save(self, path: str) -> None:
        """One torch.save file: the prepared bf16 matrix, names, E, metric."""
        torch.save({"format": _FORMAT, "matrix": self.matrix.cpu(),
                    "names": self.names, "E": self.E,
                    "metric": self.metric}, path)

    @classmethod
    def load(cls, path: str, device):
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or d.get("format") != _FORMAT:
            raise ValueError(f"{path}: not a saved CodeVectorIndex")
        m = d["matrix"]
        E = int(d["E"])
        if m.dim() != 2 or m.dtype != torch.bfloat16 \
                or m.shape[1] != _round_up(E, 32) \
                or len(d["names"]) != m.shape[0] \
                or d["metric"] not in METRICS:
            raise ValueError(f"{path}: inconsistent saved CodeVectorIndex")
        self = cls.__new__(cls)
        self.metric = d["metric"]
        self.device = torch.device(device)
        self.E = E
        self.EP = int(m.shape[1])
        self.names = list(d["names"])
        self.matrix = m.to(self.device).contiguous()
        return self

    def __len__(self) -> int:
        return self.matrix.shape[0]

    # -- search --------------------------------------------------------------
    def _check_k(self, k: int, excluding: bool) -> int:
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
        limit = len(self) - (1 if excluding else 0)
        if k > limit:
            raise ValueError(
                f"k = {k} exceeds the {limit} rows available in an index "
                f"of {len(self)}" + (" minus the query's own" if excluding
                                     else ""))
        return k

    def _search_prepared(self, q: torch.Tensor, k: int,
                         exclude: Optional[torch.Tensor]):
        if exclude is not None:
            exclude = torch.as_tensor(exclude).to(
                self.device, torch.int64).contiguous()
            if exclude.dim() != 1 or exclude.shape[0] != q.shape[0]:
                raise ValueError("exclude_rows must hold one row per query")
        return Fn.sim_topk(q, self.matrix, k, exclude)

    def search(self, queries: torch.Tensor, k: int, exclude_rows=None):
        """queries [nq, E] float -> (scores f32 [nq, k], rows i64 [nq, k]),
        best first, ties to the smallest row.  exclude_rows [nq]: one index
        row per query that must not come back (-1: none)."""
        k = self._check_k(k, exclude_rows is not None)
        return self._search_prepared(self._prepare(queries, "queries"), k,
                                     exclude_rows)

    def neighbors_of_rows(self, rows, k: int):
        """Index rows as queries, each excluding itself (de-duplication)."""
        k = self._check_k(k, True)
        rows = torch.as_tensor(rows, dtype=torch.int64).to(self.device)
        if rows.dim() != 1:
            raise ValueError("rows must be a 1-D list of index rows")
        if rows.numel() and (int(rows.min()) < 0
                             or int(rows.max()) >= len(self)):
            raise ValueError(
                f"rows must be in [0, {len(self)})")
        q = self.matrix.index_select(0, rows).contiguous()
        return self._search_prepared(q, k, rows)

    # -- range search (K24) --------------------------------------------------
    def _check_rows(self, rows) -> torch.Tensor:
        rows = torch.as_tensor(rows, dtype=torch.int64).to(self.device)
        if rows.dim() != 1:
            raise ValueError("rows must be a 1-D list of index rows")
        if rows.numel() and (int(rows.min()) < 0
                             or int(rows.max()) >= len(self)):
            raise ValueError(f"rows must be in [0, {len(self)})")
        return rows.contiguous()

    def range_search(self, queries: torch.Tensor, threshold: float,
                     exclude_rows=None, max_pairs: int = DEFAULT_MAX_PAIRS):
        """queries [nq, E] float -> CSR (offsets i64 [nq + 1], rows i64
        [nnz], scores f32 [nnz]): query i owns
        rows[offsets[i]:offsets[i + 1]], EVERY index row with a score of at
        least ``threshold``, in ascending row order.  exclude_rows [nq]: one
        index row per query that must not come back (-1: none).  More than
        ``max_pairs`` results raise a ValueError."""
        q = self._prepare(queries, "queries")
        if exclude_rows is not None:
            exclude_rows = torch.as_tensor(exclude_rows).to(
                self.device, torch.int64).contiguous()
            if exclude_rows.dim() != 1 \
                    or exclude_rows.shape[0] != q.shape[0]:
                raise ValueError("exclude_rows must hold one row per query")
        return Fn.sim_range(q, self.matrix, threshold, exclude=exclude_rows,
                            max_pairs=max_pairs)

    def neighbors_within(self, rows, threshold: float,
                         max_pairs: int = DEFAULT_MAX_PAIRS):
        """Index rows as queries, each excluding itself: the range-search
        counterpart of neighbors_of_rows.  Returns range_search's CSR."""
        rows = self._check_rows(rows)
        q = self.matrix.index_select(0, rows).contiguous()
        return Fn.sim_range(q, self.matrix, threshold, exclude=rows,
                            max_pairs=max_pairs)

    def duplicate_pairs(self, threshold: float, query_chunk: int = 16384,
                        max_pairs: int = DEFAULT_MAX_PAIRS):
        """The self-join: every unordered pair of index rows with a score of
        at least ``threshold``, once.  Returns CPU tensors (i i64, j i64,
        score f32) with i < j, sorted by (i, j).  The index is its own
        query set, ``query_chunk`` rows per range search, each row looking
        only at the rows after it; the result does not depend on
        ``query_chunk``.  ``max_pairs`` bounds the total."""
        query_chunk = int(query_chunk)
        if query_chunk < 1:
            raise ValueError(
                f"query_chunk must be >= 1, got {query_chunk}")
        R.check_sim_range_args(self.matrix[:0], self.matrix, threshold,
                               max_pairs=max_pairs)
        N = len(self)
        out_i, out_j, out_s = [], [], []
        total = 0
        for a in range(0, N, query_chunk):
            b = min(N, a + query_chunk)
            own = torch.arange(a, b, dtype=torch.int64, device=self.device)
            try:
                offsets, rows, scores = Fn.sim_range(
                    self.matrix[a:b], self.matrix, threshold, after=own,
                    max_pairs=max_pairs - total)
            except R.TooManyPairs as e:
                raise R.TooManyPairs(total + e.total, e.threshold,
                                     max_pairs) from None
            total += rows.shape[0]
            out_i.append(torch.repeat_interleave(
                own, offsets.diff()).cpu())
            out_j.append(rows.cpu())
            out_s.append(scores.cpu())
        return torch.cat(out_i), torch.cat(out_j), torch.cat(out_s)

    def duplicate_groups(self, threshold: float, query_chunk: int = 16384,
                         max_pairs: int = DEFAULT_MAX_PAIRS):
        """Groups of near-duplicates: the connected components of the graph
        whose edges are duplicate_pairs(threshold).  This is single
        linkage: similarity above a threshold is not transitive, so a group
        may hold two members that score BELOW the threshold to each other
        (A ~ B and B ~ C put A and C together).  Returns a list of row
        lists, each ascending, ordered by their smallest member (the
        group's representative); rows without a partner are omitted."""
        i, j, _ = self.duplicate_pairs(threshold, query_chunk, max_pairs)
        return _components(i, j, len(self))


def _components(i: torch.Tensor, j: torch.Tensor, n: int) -> List[List[int]]:
    """Connected components of the edges (i, j) over n nodes by min-label
    propagation to a fixed point: every node ends with the smallest node of
    its component.  Components of one node are left out."""
    if i.numel() == 0:
        return []
    label = torch.arange(n, dtype=torch.int64)
    while True:
        m = torch.minimum(label[i], label[j])
        new = label.scatter_reduce(0, i, m, "amin")
        new = new.scatter_reduce(0, j, m, "amin")
        new = new[new]  # pointer jumping: a label's own label is no larger
        if torch.equal(new, label):
            break
        label = new
    members = torch.unique(torch.cat((i, j)))  # ascending
    lab = label[members]
    order = torch.sort(lab, stable=True).indices
    members, lab = members[order], lab[order]
    sizes = torch.unique_consecutive(lab, return_counts=True)[1].tolist()
    return [g.tolist() for g in torch.split(members, sizes)]
