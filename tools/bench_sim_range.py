#!/usr/bin/env python3
"""Time the similarity range search (K24 sim_range) against the composed
path (fp32 matmul, >=, nonzero) and against K20 (sim_topk, k = 16) on one
GPU.

The index is seeded and clustered: random unit-norm bf16 rows, with clone
families planted at random rows (every member a noisy copy of the family's
base vector).  The queries are the index's first nq rows; the "self" case
is duplicate_pairs' inner call, a chunk of rows against the whole index
with after = own row.  A threshold per target number of hits per query is
read off the fp32 scores of the first 64 queries (0 hits: just above their
largest score), so "hits" is a target, and the measured mean is printed.

Per case, on the SAME tensors and alternating within each round, every
timing bracketed by device events after a warm-up: the count pass, the fill
pass (given the count pass's cursors), the whole fused call (both passes,
the scan and the host sync), the composed call and K20; median and minimum
over the rounds.  --full_join T also times CodeVectorIndex.duplicate_pairs
over the whole index at threshold T (every chunk, the copies to the host)
and the grouping of its pairs, by the host clock.

    python tools/bench_sim_range.py --full_join 0.8
    python tools/bench_sim_range.py --nq 64 --hits 10 --json out.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--N", type=int, default=605945, help="index rows")
    p.add_argument("--EP", type=int, default=128)
    p.add_argument("--nq", type=str, default="64,1024",
                   help="comma list of query counts")
    p.add_argument("--self_chunk", type=int, default=16384,
                   help="rows of the self-join chunk (0: skip that case)")
    p.add_argument("--hits", type=str, default="0,10,100",
                   help="comma list of target hits per query")
    p.add_argument("--families", type=int, default=2000,
                   help="planted clone families")
    p.add_argument("--family_size", type=int, default=24)
    p.add_argument("--noise", type=float, default=0.25,
                   help="norm of the noise added to a unit base vector")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--budget_ms", type=float, default=300.0,
                   help="device time one timing loop aims for (sets the "
                        "iteration count from a probe run)")
    p.add_argument("--nsplit", type=str, default=None,
                   help="force the fused kernel's slice count; a comma "
                        "list times each value")
    p.add_argument("--no_composed", action="store_true", default=False)
    p.add_argument("--full_join", type=str, default=None,
                   help="comma list of thresholds: also time "
                        "CodeVectorIndex.duplicate_pairs over the whole "
                        "index at each (host clock, results on the CPU)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--gpu", type=str, default="cuda:0")
    p.add_argument("--json", type=str, default=None,
                   help="also write the rows as JSON here")
    return p


def clustered_index(torch, N, EP, families, family_size, noise, seed, dev):
    """Seeded unit rows with planted clone families -> bf16 [N, EP]."""
    g = torch.Generator(device=dev).manual_seed(seed)
    db = torch.randn(N, EP, generator=g, device=dev)
    db = db / db.norm(dim=1, keepdim=True)
    n_planted = min(N, families * family_size)
    if n_planted:
        rows = torch.randperm(N, generator=g, device=dev)[:n_planted]
        base = db[rows[::family_size]].repeat_interleave(family_size, 0)
        eps = torch.randn(n_planted, EP, generator=g, device=dev)
        eps = eps / eps.norm(dim=1, keepdim=True) * noise
        member = base[:n_planted] + eps
        db[rows] = member / member.norm(dim=1, keepdim=True)
    return db.to(torch.bfloat16)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)

    import torch

    from code2vec_amd.ops import functional as Fn

    if not torch.cuda.is_available():
        raise SystemExit("bench_sim_range: needs a GPU")
    dev = torch.device(args.gpu)
    torch.cuda.set_device(dev)

    def timed(fn, iters):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters * 1000.0  # us

    def iters_for(fn):
        fn()
        fn()
        t = timed(fn, 2)
        return max(2, min(200, int(args.budget_ms * 1000.0 / max(t, 1.0))))

    N, EP = args.N, args.EP
    db = clustered_index(torch, N, EP, args.families, args.family_size,
                         args.noise, args.seed, dev)
    # thresholds from the fp32 scores of the first 64 queries
    sample = (db[:64].float() @ db.float().t()).flatten()
    hits = [int(h) for h in args.hits.split(",")]
    thresholds = {}
    for h in hits:
        if h == 0:
            thresholds[h] = float(sample.max()) + 0.01
        else:
            thresholds[h] = float(torch.topk(sample, h * 64).values[-1])
    del sample

    cases = [("rows", int(v)) for v in args.nq.split(",") if v]
    if args.self_chunk:
        cases.append(("self", args.self_chunk))
    rows = []
    print("| case | nq | N | EP | target hits | threshold | hits/query | "
          "nsplit | count med us | fill med us | fused med us | fused min us "
          "| composed med us | composed min us | composed/fused | "
          "K20 k=16 med us |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for kind, nq in cases:
        nq = min(nq, N)
        q = db[:nq]
        own = torch.arange(nq, dtype=torch.int64, device=dev)
        after = own if kind == "self" else None
        nsplits = ([int(v) for v in args.nsplit.split(",")] if args.nsplit
                   else [Fn.sim_range_default_nsplit(nq, N)])
        max_pairs = 1 << 28
        for h, nsplit in ((h, ns) for h in hits for ns in nsplits):
            t = thresholds[h]
            cur, _ = Fn.sim_range_count(q, db, t, None, after, nsplit)
            total = int(cur[-1])
            if total > max_pairs:
                print(f"| {kind} | {nq} | {N} | {EP} | {h} | {t:.4f} | "
                      f"{total / nq:.1f} | skipped: more than {max_pairs} "
                      f"pairs |", flush=True)
                continue

            def count():
                return Fn.sim_range_count(q, db, t, None, after, nsplit)

            def fill():
                return Fn.sim_range_fill(q, db, t, cur, nsplit, total, None,
                                         after)

            def fused():
                return Fn.sim_range(q, db, t, after=after,
                                    max_pairs=max_pairs, nsplit=nsplit)

            def composed():
                return Fn.sim_range_composed(q, db, t, after=after,
                                             max_pairs=max_pairs)

            def k20():
                return Fn.sim_topk(q, db, 16, own if kind == "self" else None)

            fns = [("count", count), ("fill", fill), ("fused", fused),
                   ("k20", k20)]
            if not args.no_composed:
                fns.append(("composed", composed))
                got, want = fused(), composed()
                same = (torch.equal(got[0], want[0])
                        and torch.equal(got[1], want[1]))
            else:
                same = None
            iters = {name: iters_for(fn) for name, fn in fns}
            times = {name: [] for name, _ in fns}
            for _ in range(args.rounds):
                for name, fn in fns:
                    times[name].append(timed(fn, iters[name]))
            med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
            mn = {k: min(v) for k, v in times.items()}
            row = {"case": kind, "nq": nq, "N": N, "EP": EP,
                   "target_hits": h, "threshold": t,
                   "hits_per_query": total / nq, "nsplit": nsplit,
                   "median_us": med, "min_us": mn, "iters": iters,
                   "rows_equal_composed": same}
            rows.append(row)
            c_med = med.get("composed", float("nan"))
            c_min = mn.get("composed", float("nan"))
            print(f"| {kind} | {nq} | {N} | {EP} | {h} | {t:.4f} | "
                  f"{total / nq:.2f} | {nsplit} | {med['count']:.1f} | "
                  f"{med['fill']:.1f} | {med['fused']:.1f} | "
                  f"{mn['fused']:.1f} | {c_med:.1f} | {c_min:.1f} | "
                  f"{c_med / med['fused']:.2f} | {med['k20']:.1f} |",
                  flush=True)
            if same is False:
                print(f"  note: fused and composed report different rows at "
                      f"{kind} nq={nq} t={t} (scores next to the threshold "
                      f"differ by summation order)", flush=True)
    if args.full_join:
        # CodeVectorIndex.duplicate_pairs over the WHOLE index: every chunk,
        # the device-to-host copies and the host-side concatenation, by the
        # host clock around a call that ends with everything on the CPU
        import time

        from code2vec_amd.engine.similar import CodeVectorIndex

        index = CodeVectorIndex.__new__(CodeVectorIndex)
        index.metric, index.device = "dot", dev
        index.E = index.EP = EP
        index.names = None  # not used by the join
        index.matrix = db
        print("\n| full self-join | N | threshold | pairs | groups | "
              "duplicate_pairs med ms | min ms | components ms |")
        print("|---|---|---|---|---|---|---|---|")
        for t in (float(v) for v in args.full_join.split(",")):
            index.duplicate_pairs(t, max_pairs=1 << 28)  # warm-up
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                i, j, _ = index.duplicate_pairs(t, max_pairs=1 << 28)
                ts.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            from code2vec_amd.engine.similar import _components
            groups = _components(i, j, N)
            tc = (time.perf_counter() - t0) * 1e3
            ts.sort()
            rows.append({"case": "full_join", "N": N, "threshold": t,
                         "pairs": int(i.numel()), "groups": len(groups),
                         "duplicate_pairs_ms": ts, "components_ms": tc})
            print(f"| duplicate_pairs | {N} | {t} | {i.numel()} | "
                  f"{len(groups)} | {ts[1]:.1f} | {ts[0]:.1f} | {tc:.1f} |",
                  flush=True)
    if args.json:
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
