#!/usr/bin/env python3
"""Time a full eager training step on one GPU: the padded [B, C] rectangle
(Code2VecHIP.forward) against packed batches (forward_packed_train, K21 +
K22), at the top11 model shape (E = 100, L = 72,416, B = 1,024, C = 200).

A step is built as bench.py's: zero_grad, forward, loss, backward and
finish_and_step (fused table Adam), dropout 0.25, on batches staged on the
device beforehand.  The packed step is timed as the trainer runs it: the
host-side length check included, the device offsets arriving with the batch
as the loader delivers them.

Seeded length distributions over the B methods (those of bench_packed.py,
plus the F1 corpus's mean):

    full      every method has C contexts
    short     geometric-like, mean 40, clipped to 1..C
    f1        geometric-like, mean 32, clipped to 1..C

Both paths run on the same methods, alternating within each round, every
timing bracketed by device events after a warm-up of every batch shape; the
median and minimum over the rounds are printed as ms per step.  The padded
path counts B * C contexts per step, the packed path its real rows.
torch.cuda.memory_reserved() and the size of the persistent scratch cache
are printed after the warm-up and at the end.

    python tools/bench_packed_train.py
    python tools/bench_packed_train.py --dists f1 --json out.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DISTS = ("full", "short", "f1")
MEANS = {"short": 40, "f1": 32}


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--dists", type=str, default=",".join(DISTS),
                   help="comma list of " + ", ".join(DISTS))
    p.add_argument("--methods", type=int, default=1024,
                   help="B, methods per batch")
    p.add_argument("--contexts", type=int, default=200,
                   help="C = max_path_length")
    p.add_argument("--encode", type=int, default=100)
    p.add_argument("--embed", type=int, default=100)
    p.add_argument("--labels", type=int, default=72416)
    p.add_argument("--terminals", type=int, default=360632)
    p.add_argument("--paths", type=int, default=342846)
    p.add_argument("--pool", type=int, default=4,
                   help="distinct batches per distribution (distinct row "
                        "counts on the packed path)")
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
    return np.clip(rng.geometric(1.0 / MEANS[dist], n), 1, C).astype(np.int64)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    dists = args.dists.split(",")
    for dname in dists:
        if dname not in DISTS:
            raise SystemExit(
                f"bench_packed_train: unknown distribution {dname!r}")

    import numpy as np
    import torch

    from code2vec_amd.engine.optim import FusedAdam
    from code2vec_amd.models.code2vec import Code2VecHIP, init_logical_params
    from code2vec_amd.ops import functional as Fn
    from code2vec_amd.parallel.ddp import BucketedAllReduce
    from code2vec_amd.utils.options import Option

    if not torch.cuda.is_available():
        raise SystemExit("bench_packed_train: needs a GPU")
    dev = torch.device(args.gpu)
    torch.cuda.set_device(dev)
    torch.manual_seed(123)
    B, C = args.methods, args.contexts
    cap = B * C

    opt = Option(terminal_count=args.terminals, path_count=args.paths,
                 label_count=args.labels, max_path_length=C,
                 terminal_embed_size=args.embed, path_embed_size=args.embed,
                 encode_size=args.encode, dropout_prob=0.25, batch_size=B,
                 device=dev)
    model = Code2VecHIP(
        opt, init_logical_params(opt, torch.Generator().manual_seed(123)),
        device=dev).train()
    optim = FusedAdam(model.parameters(), lr=0.01, betas=(0.9, 0.999))
    ddp = BucketedAllReduce(
        list(model.parameters()), 1,
        owned_params=[model.terminal_embedding, model.path_embedding])
    class_weight = torch.ones(args.labels, device=dev)

    def finish(outputs, y):
        loss = model.loss(outputs, y, class_weight)
        loss.backward()
        ddp.finish_and_step(optim)

    def padded_step(b):
        s, p, e, y = b["padded"]
        ddp.zero_grad()
        outputs, _, _ = model(s, p, e, y)
        finish(outputs, y)

    def packed_step(b):
        s, p, e, y = b["packed"]
        ddp.zero_grad()
        outputs, _, _ = model.forward_packed_train(
            s, p, e, b["lengths"], y, offsets=b["offsets"], row_capacity=cap)
        finish(outputs, y)

    def timed(fn, pool, iters):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for i in range(iters):
            fn(pool[i % len(pool)])
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / iters  # ms

    def memory(tag):
        print(f"[{tag}] memory_reserved = "
              f"{torch.cuda.memory_reserved(dev) / 2**20:.1f} MiB, "
              f"len(_scratch_cache) = {len(Fn._scratch_cache)}", flush=True)

    # every batch of every distribution, staged before anything is timed
    pools = {}
    for dname in dists:
        rng = np.random.default_rng([args.seed, DISTS.index(dname)])
        pool = []
        for _ in range(args.pool):
            lens = draw_lengths(dname, B, C, rng)
            real = np.arange(C)[None, :] < lens[:, None]
            padded = []
            for hi in (args.terminals, args.paths, args.terminals):
                a = rng.integers(1, hi, (B, C)).astype(np.int32)
                a[~real] = 0
                padded.append(a)
            y = torch.from_numpy(
                rng.integers(0, args.labels, B).astype(np.int64)).to(dev)
            off = np.zeros(B + 1, dtype=np.int32)
            np.cumsum(lens, out=off[1:])
            pool.append({
                "padded": tuple(torch.from_numpy(a).to(dev)
                                for a in padded) + (y,),
                "packed": tuple(torch.from_numpy(a[real]).to(dev)
                                for a in padded) + (y,),
                "lengths": torch.from_numpy(lens),
                "offsets": torch.from_numpy(off).to(dev),
                "rows": int(lens.sum()),
            })
        pools[dname] = pool

    # warm-up of every shape on both paths
    for dname in dists:
        for b in pools[dname]:
            for _ in range(2):
                padded_step(b)
                packed_step(b)
    torch.cuda.synchronize()
    memory("after warm-up")

    rows = []
    print("| lengths | mean rows packed | rows padded | path | med ms/step | "
          "min ms/step | contexts/s (own count) | methods/s | vs padded |")
    print("|---|---|---|---|---|---|---|---|---|")
    for dname in dists:
        pool = pools[dname]
        mean_rows = sum(b["rows"] for b in pool) / len(pool)
        paths = (("padded", padded_step), ("packed", packed_step))
        iters = {}
        for name, fn in paths:
            t = timed(fn, pool, len(pool))
            n = int(args.budget_ms / max(t, 1e-3))
            iters[name] = max(len(pool), min(500, n // len(pool) * len(pool)))
        times = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                times[name].append(timed(fn, pool, iters[name]))
        med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
        for name, _ in paths:
            t = med[name]
            ctx = (B * C if name == "padded" else mean_rows) / t * 1e3
            ratio = med["padded"] / t
            rows.append({
                "dist": dname, "methods": B, "rows_packed_mean": mean_rows,
                "rows_padded": B * C, "path": name, "med_ms": t,
                "min_ms": min(times[name]), "contexts_per_s": ctx,
                "methods_per_s": B / t * 1e3, "speedup_vs_padded": ratio,
                "iters": iters[name], "rounds": args.rounds,
                "pool": len(pool)})
            print(f"| {dname} | {mean_rows:,.0f} | {B * C:,} | {name} | "
                  f"{t:.3f} | {min(times[name]):.3f} | {ctx:,.0f} | "
                  f"{B / t * 1e3:,.0f} | {ratio:.2f}x |", flush=True)
    memory("at the end")
    ddp.close()
    if args.json:
        with open(args.json, "w", encoding="utf-8") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
