#!/usr/bin/env python3
"""Time the fused similarity + top-k kernel (K20 sim_topk) against the
composed path (fp32 matmul + K19 row_topk) on one GPU.

Per shape: unit-norm random bf16 rows, both paths on the SAME tensors,
alternating within each round, every timing bracketed by device events
after a warm-up; the median and minimum over the rounds are printed, plus
the index bytes the fused kernel streams per second
(ceil(nq / query_tile) * N * EP * 2 / t) and the largest score difference
between the two paths.

    python tools/bench_sim.py
    python tools/bench_sim.py --shapes 64x605945x128 --k 10 --json out.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_SHAPES = ("1x605945x128,64x605945x128,1024x605945x128,"
                  "1x4194304x128,64x4194304x128,1024x4194304x128,"
                  "64x605945x320")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", type=str, default=DEFAULT_SHAPES,
                   help="comma list of nq x N x EP")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--budget_ms", type=float, default=400.0,
                   help="device time one timing loop aims for (sets the "
                        "iteration count from a probe run)")
    p.add_argument("--nsplit", type=str, default=None,
                   help="force the fused kernel's slice count; a comma "
                        "list times each value")
    p.add_argument("--fused_only", action="store_true", default=False,
                   help="skip the composed path (for nsplit sweeps)")
    p.add_argument("--gpu", type=str, default="cuda:0")
    p.add_argument("--json", type=str, default=None,
                   help="also write the rows as JSON here")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)

    import torch

    from code2vec_amd.ops import functional as Fn

    if not torch.cuda.is_available():
        raise SystemExit("bench_sim: needs a GPU")
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

    nsplits = ([int(v) for v in args.nsplit.split(",")]
               if args.nsplit else [None])
    rows = []
    print("| nq | N | EP | k | nsplit | fused med us | fused min us | "
          "composed med us | composed min us | composed/fused | "
          "index TB/s | max score diff |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for spec in args.shapes.split(","):
        nq, N, EP = (int(v) for v in spec.lower().split("x"))
        g = torch.Generator(device=dev).manual_seed(nq + N + EP)
        db = torch.randn(N, EP, generator=g, device=dev)
        db = (db / db.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        q = torch.randn(nq, EP, generator=g, device=dev)
        q = (q / q.norm(dim=1, keepdim=True)).to(torch.bfloat16)
        for nsplit in nsplits:
            if nsplit is None:
                nsplit = Fn.sim_topk_default_nsplit(nq, N)

            def fused():
                return Fn.sim_topk(q, db, args.k, nsplit=nsplit)

            def composed():
                return Fn.sim_topk_composed(q, db, args.k)

            if args.fused_only:
                diff = float("nan")
                it_f, it_c = iters_for(fused), 0
            else:
                diff = float((fused()[0] - composed()[0]).abs().max())
                it_f, it_c = iters_for(fused), iters_for(composed)
            tf, tc = [], []
            for _ in range(args.rounds):
                tf.append(timed(fused, it_f))
                tc.append(timed(composed, it_c) if it_c else float("nan"))
            tf.sort()
            tc.sort()
            med_f, med_c = tf[len(tf) // 2], tc[len(tc) // 2]
            passes = -(-nq // Fn.SIM_QUERY_TILE)
            tbs = passes * N * EP * 2 / (med_f * 1e-6) / 1e12
            row = {"nq": nq, "N": N, "EP": EP, "k": args.k, "nsplit": nsplit,
                   "fused_med_us": med_f, "fused_min_us": tf[0],
                   "composed_med_us": med_c, "composed_min_us": tc[0],
                   "ratio": med_c / med_f, "index_TBps": tbs,
                   "max_score_diff": diff, "iters": [it_f, it_c]}
            rows.append(row)
            print(f"| {nq} | {N} | {EP} | {args.k} | {nsplit} | {med_f:.1f} | "
                  f"{tf[0]:.1f} | {med_c:.1f} | {tc[0]:.1f} | "
                  f"{med_c / med_f:.2f} | {tbs:.2f} | {diff:.2e} |", flush=True)
        del db, q
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
