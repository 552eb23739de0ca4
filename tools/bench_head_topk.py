#!/usr/bin/env python3
"""Time the fused head + top-k kernel (K23 head_topk) against the composed
paths on one GPU, and report each path's peak memory.

Three paths on the SAME seeded tensors per shape (default head: bf16 code
vectors, weight and an fp32 bias, scale 1):
  fused     Fn.head_topk (no [nq, L] tensor)
  composed  Fn.head_topk_composed: fp32 matmul in query chunks + K19
  logits    Fn.head_topk_composed(bf16_logits=True): the prediction path
            without K23 — OutputHead's bf16 [nq, L] logits, then K19
They alternate within each round; every timing is bracketed by device
events after a warm-up, with an iteration count that fills about
--budget_ms; median (min) over the rounds in microseconds.  Peak memory is
torch.cuda.max_memory_allocated over one call above the level before it,
reset before each path.

    python tools/bench_head_topk.py
    python tools/bench_head_topk.py --shapes 1x72416x128 --nsplit 17,35,70 \\
        --fused_only
    python tools/bench_head_topk.py --device cpu --tiny
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEFAULT_SHAPES = ",".join(f"{nq}x{L}x128" for L in (72416, 261245)
                          for nq in (1, 16, 64, 1024))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shapes", type=str, default=DEFAULT_SHAPES,
                   help="comma list of nq x L x EP")
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--budget_ms", type=float, default=400.0,
                   help="device time one timing loop aims for (sets the "
                        "iteration count from a probe run)")
    p.add_argument("--nsplit", type=str, default=None,
                   help="force the fused kernel's slice count; a comma "
                        "list times each value")
    p.add_argument("--fused_only", action="store_true", default=False,
                   help="skip the composed paths (for nsplit sweeps)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--tiny", action="store_true", default=False,
                   help="one toy shape, one round (with --device cpu: the "
                        "oracle, a smoke test of this tool)")
    p.add_argument("--json", type=str, default=None,
                   help="also write the rows as JSON here")
    return p


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)

    import time

    import torch

    from code2vec_amd.ops import functional as Fn

    dev = torch.device(args.device)
    on_gpu = dev.type == "cuda"
    if on_gpu:
        if not torch.cuda.is_available():
            raise SystemExit("bench_head_topk: needs a GPU (or --device cpu "
                             "--tiny)")
        torch.cuda.set_device(dev)
    elif not args.tiny:
        raise SystemExit("bench_head_topk: --device cpu only runs --tiny")
    if args.tiny:
        args.shapes, args.rounds, args.budget_ms = "3x200x64", 1, 1.0

    def timed(fn, iters):
        if not on_gpu:
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            return (time.perf_counter() - t0) / iters * 1e6
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
        return max(2, min(500, int(args.budget_ms * 1000.0 / max(t, 1.0))))

    def peak_mib(fn):
        if not on_gpu:
            return float("nan")
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        del out
        return peak / 2.0 ** 20

    nsplits = ([int(v) for v in args.nsplit.split(",")]
               if args.nsplit else [None])
    names = ("fused",) if args.fused_only else ("fused", "composed", "logits")
    rows = []
    head = "| nq | L | EP | k | nsplit |"
    for n in names:
        head += f" {n} med (min) us | {n} peak MiB |"
    if not args.fused_only:
        head += " composed/fused | logits/fused | max val diff |"
    print(head)
    print("|" + "---|" * (head.count("|") - 1))
    for spec in args.shapes.split(","):
        nq, L, EP = (int(v) for v in spec.lower().split("x"))
        g = torch.Generator().manual_seed(nq + L + EP)
        dt = torch.bfloat16 if on_gpu else torch.float32
        w = (0.3 * torch.randn(L, EP, generator=g)).to(dt).to(dev)
        q = (0.3 * torch.randn(nq, EP, generator=g)).to(dt).to(dev)
        bias = torch.randn(L, generator=g).to(dev)
        for nsplit in nsplits:
            if nsplit is None:
                nsplit = Fn.head_topk_default_nsplit(L, EP)
            fns = {
                "fused": lambda: Fn.head_topk(q, w, args.k, bias,
                                              nsplit=nsplit),
                "composed": lambda: Fn.head_topk_composed(q, w, args.k, bias),
                "logits": lambda: Fn.head_topk_composed(
                    q, w, args.k, bias, bf16_logits=on_gpu),
            }
            diff = float("nan")
            if not args.fused_only:
                diff = float((fns["fused"]()[0]
                              - fns["composed"]()[0]).abs().max())
            peaks = {n: peak_mib(fns[n]) for n in names}
            iters = {n: iters_for(fns[n]) for n in names}
            times = {n: [] for n in names}
            for _ in range(args.rounds):
                for n in names:
                    times[n].append(timed(fns[n], iters[n]))
            row = {"nq": nq, "L": L, "EP": EP, "k": args.k, "nsplit": nsplit,
                   "max_val_diff": diff, "iters": iters}
            line = f"| {nq} | {L} | {EP} | {args.k} | {nsplit} |"
            for n in names:
                t = sorted(times[n])
                row[f"{n}_med_us"], row[f"{n}_min_us"] = t[len(t) // 2], t[0]
                row[f"{n}_peak_mib"] = peaks[n]
                line += (f" {t[len(t) // 2]:.1f} ({t[0]:.1f}) | "
                         f"{peaks[n]:.1f} |")
            if not args.fused_only:
                f = row["fused_med_us"]
                line += (f" {row['composed_med_us'] / f:.2f} | "
                         f"{row['logits_med_us'] / f:.2f} | {diff:.2e} |")
            rows.append(row)
            print(line, flush=True)
        del w, q, bias
        if on_gpu:
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
