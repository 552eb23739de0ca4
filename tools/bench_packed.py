#!/usr/bin/env python3
"""Time prediction forwards on one GPU: the padded [B, C] layout (eager, and
the hipGraph replay the Predictor uses) against the packed variable-length
layout (Code2VecHIP.forward_packed, K21), at the top11 model shape
(E = 100, L = 72,416, C = 200, 1,024 methods per batch).

Three seeded length distributions over the 1,024 methods:

    full      every method has C contexts
    short     geometric-like, mean 40, clipped to 1..C
    longtail  short, with 1% of the methods at 10 * C contexts (the padded
              path subsamples those to C, the packed path keeps them)

The three paths run on the same methods, alternating within each round,
every timing bracketed by device events after a warm-up of every shape; the
median and minimum over the rounds are printed as ms per 1,024 methods and
methods/s.  The packed forward is timed as a caller sees it, host-side
length check and offsets upload included; the graph replay likewise with
its input copies.

    python tools/bench_packed.py
    python tools/bench_packed.py --dists short,longtail --json out.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTS = ("full", "short", "longtail")
SHORT_MEAN = 40
LONG_FRACTION = 0.01
LONG_FACTOR = 10


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--dists", type=str, default=",".join(DISTS),
                   help="comma list of " + ", ".join(DISTS))
    p.add_argument("--methods", type=int, default=1024,
                   help="methods per batch")
    p.add_argument("--contexts", type=int, default=200,
                   help="C = max_path_length of the padded path")
    p.add_argument("--encode", type=int, default=100)
    p.add_argument("--embed", type=int, default=100)
    p.add_argument("--labels", type=int, default=72416)
    p.add_argument("--terminals", type=int, default=360632)
    p.add_argument("--paths", type=int, default=342846)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--budget_ms", type=float, default=400.0,
                   help="device time one timing loop aims for (sets the "
                        "iteration count from a probe run)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--gpu", type=str, default="cuda:0")
    p.add_argument("--json", type=str, default=None,
                   help="also write the rows as JSON here")
    return p


def draw_lengths(dist: str, n: int, C: int, rng):
    """Seeded context counts of ``n`` methods."""
    import numpy as np

    if dist == "full":
        return np.full(n, C, dtype=np.int64)
    lens = np.clip(rng.geometric(1.0 / SHORT_MEAN, n), 1, C).astype(np.int64)
    if dist == "longtail":
        k = max(1, int(round(n * LONG_FRACTION)))
        lens[rng.choice(n, k, replace=False)] = LONG_FACTOR * C
    return lens


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    dists = args.dists.split(",")
    for dname in dists:
        if dname not in DISTS:
            raise SystemExit(f"bench_packed: unknown distribution {dname!r}")

    import numpy as np
    import torch

    from code2vec_amd.engine.infer import GraphedInference
    from code2vec_amd.models.code2vec import Code2VecHIP, init_logical_params
    from code2vec_amd.utils.options import Option

    if not torch.cuda.is_available():
        raise SystemExit("bench_packed: needs a GPU")
    dev = torch.device(args.gpu)
    torch.cuda.set_device(dev)
    B, C = args.methods, args.contexts

    opt = Option(terminal_count=args.terminals, path_count=args.paths,
                 label_count=args.labels, max_path_length=C,
                 terminal_embed_size=args.embed, path_embed_size=args.embed,
                 encode_size=args.encode, dropout_prob=0.0, batch_size=B,
                 device=dev)
    model = Code2VecHIP(
        opt, init_logical_params(opt, torch.Generator().manual_seed(1)),
        device=dev).eval()
    graphed = GraphedInference(model, B, dev)
    label = torch.zeros(B, dtype=torch.int64, device=dev)

    def timed(fn, iters):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters  # ms

    def iters_for(fn):
        for _ in range(3):
            fn()
        t = timed(fn, 3)
        return max(3, min(500, int(args.budget_ms / max(t, 1e-3))))

    rows = []
    print("| lengths | rows packed | rows padded | path | med ms / "
          f"{B} methods | min ms | methods/s | vs graph replay |")
    print("|---|---|---|---|---|---|---|---|")
    for dname in dists:
        rng = np.random.default_rng([args.seed, DISTS.index(dname)])
        lens = draw_lengths(dname, B, C, rng)
        M = int(lens.sum())
        flat = [rng.integers(1, hi, M).astype(np.int32)
                for hi in (args.terminals, args.paths, args.terminals)]
        # the padded layout of the same methods: at most C contexts each
        # (a longer bag subsampled, as DatasetBuilder.build_data does)
        padded = [np.zeros((B, C), dtype=np.int32) for _ in range(3)]
        lo = 0
        for i, n in enumerate(lens.tolist()):
            sel = (np.arange(n) if n <= C
                   else np.sort(rng.permutation(n)[:C])) + lo
            for dst, src in zip(padded, flat):
                dst[i, :len(sel)] = src[sel]
            lo += n
        f_s, f_p, f_e = (torch.from_numpy(x).to(dev) for x in flat)
        p_s, p_p, p_e = (torch.from_numpy(x).to(dev) for x in padded)
        lens_t = torch.from_numpy(lens)

        def eager():
            with torch.no_grad():
                return model(p_s, p_p, p_e, label)

        def replay():
            return graphed.run(p_s, p_p, p_e, label)

        def packed():
            return model.forward_packed(f_s, f_p, f_e, lens_t)

        paths = (("padded eager", eager), ("padded graph replay", replay),
                 ("packed", packed))
        iters = {name: iters_for(fn) for name, fn in paths}
        times = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                times[name].append(timed(fn, iters[name]))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for name, _ in paths:
            t = med[name]
            ratio = med["padded graph replay"] / t
            row = {"dist": dname, "methods": B, "rows_packed": M,
                   "rows_padded": B * C, "path": name, "med_ms": t,
                   "min_ms": min(times[name]), "methods_per_s": B / t * 1e3,
                   "speedup_vs_graph_replay": ratio, "iters": iters[name],
                   "rounds": args.rounds,
                   "mean_len": float(lens.mean()), "max_len": int(lens.max())}
            rows.append(row)
            print(f"| {dname} | {M} | {B * C} | {name} | {t:.3f} | "
                  f"{min(times[name]):.3f} | {B / t * 1e3:,.0f} | "
                  f"{ratio:.2f}x |", flush=True)
        del f_s, f_p, f_e, p_s, p_p, p_e
    if args.json:
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
