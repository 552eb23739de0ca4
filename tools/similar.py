#!/usr/bin/env python3
"""Find the methods most similar to a query among exported code vectors.

The index is a code.vec written by main.py (--vectors) or an index saved
earlier with --save_index (--index).  Exactly one query source:

  --query_vectors other.vec        every row of another code.vec
  --query_predictions preds.jsonl  the output of tools/predict.py
                                   --with_vector ("vector", "expected"/"id")
  --self                           every index row against the rest
                                   (clone / near-duplicate detection)

One JSON object per query, in input order:

    {"query": i, "name": ..., "neighbors": [{"row", "name", "score"}]}

--k K lists the K best rows (at most 16); --threshold T lists EVERY row
that scores at least T instead, best first, however many there are.  With
--self --threshold T, --groups writes the groups of near-duplicates (the
connected components of the pairs scoring at least T), one per line:

    {"group": g, "size": n, "representative": {"row", "name"},
     "members": [{"row", "name"}, ...]}

    python tools/similar.py --vectors output/code.vec --self --k 5
    python tools/similar.py --vectors output/code.vec --self \\
        --threshold 0.95 --groups
    python tools/predict.py ... --with_vector --out preds.jsonl
    python tools/similar.py --vectors output/code.vec \\
        --query_predictions preds.jsonl
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_K = 16
DEFAULT_K = 5
# queries per search call: bounds the host-side result handling, the
# kernel itself takes any number
QUERY_CHUNK = 4096


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--vectors", type=str, default=None,
                   help="code.vec to search (header 'count\\tencode_size', "
                        "rows 'name\\tv0 v1 ...')")
    p.add_argument("--index", type=str, default=None,
                   help="index saved with --save_index (instead of --vectors)")
    p.add_argument("--query_vectors", type=str, default=None,
                   help="code.vec whose rows are the queries")
    p.add_argument("--query_predictions", type=str, default=None,
                   help="JSON lines of tools/predict.py --with_vector")
    p.add_argument("--self", dest="self_search", action="store_true",
                   default=False,
                   help="every index row against all the others")
    p.add_argument("--k", type=int, default=None,
                   help=f"neighbours per query (1..{MAX_K}; default "
                        f"{DEFAULT_K} unless --threshold is given)")
    p.add_argument("--threshold", type=float, default=None,
                   help="list every row scoring at least this instead of "
                        "the --k best")
    p.add_argument("--groups", action="store_true", default=False,
                   help="with --self --threshold: write groups of "
                        "near-duplicates instead of per-query lists")
    p.add_argument("--max_pairs", type=int, default=None,
                   help="with --threshold: give up beyond this many "
                        "results per search call, or pairs in all with "
                        "--groups (default 2^24)")
    p.add_argument("--metric", type=str, default=None,
                   choices=["cosine", "dot"],
                   help="default: cosine for --vectors, the saved one for "
                        "--index")
    p.add_argument("--save_index", type=str, default=None,
                   help="write the prepared index here for later --index")
    p.add_argument("--out", type=str, default=None,
                   help="output file (default: stdout)")
    p.add_argument("--no_cuda", action="store_true", default=False)
    p.add_argument("--gpu", type=str, default="cuda:0")
    return p


def _read_predictions(path):
    """(names, vectors) from predict.py's JSON lines."""
    names, vecs = [], []
    with open(path, encoding="utf-8") as f:
        for lineno, line in enumerate(f, start=1):
            if not line.strip():
                continue
            try:
                row = json.loads(line)
            except json.JSONDecodeError:
                raise SystemExit(
                    f"similar: {path}: line {lineno} is not JSON")
            if "vector" not in row:
                raise SystemExit(
                    f"similar: {path}: line {lineno} has no \"vector\" "
                    f"(run tools/predict.py with --with_vector)")
            name = row.get("expected")
            if name is None:
                name = row.get("id")
            names.append("" if name is None else str(name))
            vecs.append(row["vector"])
    if not vecs:
        raise SystemExit(f"similar: {path}: no queries")
    width = len(vecs[0])
    for i, v in enumerate(vecs):
        if len(v) != width:
            raise SystemExit(
                f"similar: {path}: query {i} has {len(v)} components, "
                f"query 0 has {width}")
    return names, vecs


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.threshold is not None and args.k is not None:
        raise SystemExit(
            "similar: --k and --threshold are mutually exclusive")
    if args.groups and not (args.self_search and args.threshold is not None):
        raise SystemExit("similar: --groups needs --self and --threshold")
    if args.max_pairs is not None and args.threshold is None:
        raise SystemExit("similar: --max_pairs needs --threshold")
    if args.max_pairs is not None and args.max_pairs < 0:
        raise SystemExit(
            f"similar: --max_pairs must be >= 0, got {args.max_pairs}")
    if args.threshold is not None and not math.isfinite(args.threshold):
        raise SystemExit(
            f"similar: --threshold must be finite, got {args.threshold}")
    ranged = args.threshold is not None
    if not ranged and args.k is None:
        args.k = DEFAULT_K
    if not ranged and not 1 <= args.k <= MAX_K:
        raise SystemExit(f"similar: --k must be in 1..{MAX_K}, got {args.k}")
    if (args.vectors is None) == (args.index is None):
        raise SystemExit(
            "similar: give exactly one of --vectors and --index")
    sources = [s for s, on in (
        ("--query_vectors", args.query_vectors is not None),
        ("--query_predictions", args.query_predictions is not None),
        ("--self", args.self_search)) if on]
    if len(sources) != 1:
        raise SystemExit(
            "similar: give exactly one query source (--query_vectors, "
            "--query_predictions or --self), got "
            + (" and ".join(sources) if sources else "none"))

    import torch

    from code2vec_amd.engine.similar import CodeVectorIndex, read_code_vec

    use_cuda = not args.no_cuda and torch.cuda.is_available()
    device = torch.device(args.gpu if use_cuda else "cpu")
    if use_cuda:
        torch.cuda.set_device(device)

    try:
        if args.index is not None:
            index = CodeVectorIndex.load(args.index, device)
            if args.metric is not None and index.metric != args.metric:
                raise SystemExit(
                    f"similar: --index was saved with metric "
                    f"{index.metric}, --metric asks for {args.metric}")
        else:
            index = CodeVectorIndex.from_code_vec(
                args.vectors, device, metric=args.metric or "cosine")
    except (ValueError, OSError) as e:
        raise SystemExit(f"similar: {e}") from e
    if args.save_index:
        index.save(args.save_index)

    N = len(index)
    range_kw = {} if args.max_pairs is None else {"max_pairs": args.max_pairs}
    if args.self_search:
        if not ranged and args.k >= N:
            raise SystemExit(
                f"similar: --self needs --k below the index's {N} rows, "
                f"got {args.k}")
        q_names, q_vecs = index.names, None
        nq = N
    else:
        if not ranged and args.k > N:
            raise SystemExit(
                f"similar: --k {args.k} exceeds the index's {N} rows")
        try:
            if args.query_vectors is not None:
                q_names, q_vecs = read_code_vec(args.query_vectors)
                if not q_names:
                    raise SystemExit(
                        f"similar: {args.query_vectors}: no queries")
            else:
                q_names, rows = _read_predictions(args.query_predictions)
                q_vecs = torch.tensor(rows, dtype=torch.float32)
        except (ValueError, OSError) as e:
            raise SystemExit(f"similar: {e}") from e
        if q_vecs.shape[1] != index.E:
            raise SystemExit(
                f"similar: dimension mismatch: queries have "
                f"{q_vecs.shape[1]} components, the index has {index.E}")
        nq = q_vecs.shape[0]

    out = open(args.out, "w", encoding="utf-8") if args.out else sys.stdout
    try:
        if args.groups:
            try:
                groups = index.duplicate_groups(args.threshold, **range_kw)
            except ValueError as e:
                raise SystemExit(f"similar: {e}") from e
            for g, members in enumerate(groups):
                out.write(json.dumps({
                    "group": g,
                    "size": len(members),
                    "representative": {"row": members[0],
                                       "name": index.names[members[0]]},
                    "members": [{"row": r, "name": index.names[r]}
                                for r in members],
                }) + "\n")
            extra = sum(len(m) - 1 for m in groups)
            print(f"similar: {N} methods, {len(groups)} groups, {extra} "
                  f"rows that are not a representative", file=sys.stderr)
            return 0
        for a in range(0, nq, QUERY_CHUNK):
            b = min(nq, a + QUERY_CHUNK)
            if ranged:
                try:
                    if q_vecs is None:
                        csr = index.neighbors_within(
                            torch.arange(a, b), args.threshold, **range_kw)
                    else:
                        csr = index.range_search(
                            q_vecs[a:b], args.threshold, **range_kw)
                except ValueError as e:
                    raise SystemExit(f"similar: {e}") from e
                offsets, rows, scores = (t.cpu() for t in csr)
                offsets = offsets.tolist()
                for i in range(b - a):
                    r = rows[offsets[i]:offsets[i + 1]]
                    s = scores[offsets[i]:offsets[i + 1]]
                    # best first; rows come ascending, so a stable sort
                    # leaves equal scores by ascending row
                    order = torch.sort(s, descending=True,
                                       stable=True).indices
                    out.write(json.dumps({
                        "query": a + i,
                        "name": q_names[a + i],
                        "neighbors": [
                            {"row": rr, "name": index.names[rr], "score": ss}
                            for rr, ss in zip(r[order].tolist(),
                                              s[order].tolist())],
                    }) + "\n")
                continue
            try:
                if q_vecs is None:
                    scores, rows = index.neighbors_of_rows(
                        torch.arange(a, b), args.k)
                else:
                    scores, rows = index.search(q_vecs[a:b], args.k)
            except ValueError as e:
                raise SystemExit(f"similar: {e}") from e
            scores = scores.cpu().tolist()
            rows = rows.cpu().tolist()
            for i in range(b - a):
                out.write(json.dumps({
                    "query": a + i,
                    "name": q_names[a + i],
                    "neighbors": [
                        {"row": r, "name": index.names[r], "score": s}
                        for r, s in zip(rows[i], scores[i])],
                }) + "\n")
    finally:
        if args.out:
            out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
