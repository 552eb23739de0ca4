#!/usr/bin/env python3
"""Flagship benchmark — the driver contract.

Measures the headline metric of BASELINE.json: whole-node
path-contexts/sec of code2vec training on the top11-shaped config
(terminal vocab 360,631(+question), path vocab 342,845(+pad), batch 1024,
200 contexts/method, embed/encode 100, bf16) with synthetic dense data and
random-init weights.  One process per GPU (torchrun), RCCL data parallelism,
weak scaling (per-GPU batch fixed at 1024).

A timed step = forward + fused loss + backward + bucketed gradient
all-reduce + fused Adam — the full training step.  label_count for top11 is
not published by the reference; 72,416 is DERIVED from its real data via a
Heaps-law fit to methods.txt's unique-name curve (tools/derive_label_vocab.py)
and stated in config.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--config top11]
                       [--dump-outputs DIR] [--full]
For N>1 the driver launches via torch.distributed.run.

A plain run sets up, warms up, times the K steps and prints one JSON result
line.  --dump-outputs DIR additionally writes what the last timed step
returned (and the parameters it updated) as DIR/<name>.npy, float32, so two
builds can be compared output for output.  Model init, batches and the
dropout RNG are seeded, and that last step is run from the seeded initial
model and optimizer state (put back with the clock stopped), so what it
computes is a function of the arguments alone and repeats from run to run.
--full is where any measurement beyond the headline figure belongs; the
benchmark has none today (other modes and configs are runs of their own,
selected with --mode / --config / --real-pipeline), so it changes nothing.
"""

from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time

# hipBLASLt/rocBLAS GEMM autotuning for the plain dgrad/wgrad GEMMs — the
# tuning happens on first use of each shape, inside the untimed warmup steps.
os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME",
                      os.path.join(os.environ.get("TMPDIR", "/tmp"),
                                   "c2v_tunableop_%d.csv"))

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from code2vec_amd.data.synthetic import synthetic_batch
from code2vec_amd.engine.optim import FusedAdam
from code2vec_amd.models.code2vec import Code2VecHIP, init_logical_params
from code2vec_amd.parallel.ddp import BucketedAllReduce
from code2vec_amd.parallel.dist import init_distributed
from code2vec_amd.utils.options import Option

CONFIGS = {
    # BASELINE.json config 2/3: top11-shaped (top11_dataset/params.txt:7-9).
    # label_count DERIVED from real reference data: Heaps' law
    # V(n)=1.01*n^0.840 fit to the prefix-unique normalized-name curve of
    # the reference's dataset/methods.txt (9,916 real methods, 2,280
    # unique) gives V(605,945)=72,415; the synthetic generator's
    # calibrated name process reproduces it (72,539 simulated) —
    # tools/derive_label_vocab.py.  72,416 = fit rounded to the kernel
    # 8-granule.
    "top11": dict(terminal_count=360632, path_count=342846, label_count=72416,
                  embed=100, encode=100, batch=1024, contexts=200),
    # BASELINE.json config 4: java-large-scale synthetic
    "java-large": dict(terminal_count=1_100_000, path_count=1_300_000,
                       label_count=261_000, embed=128, encode=128,
                       batch=1024, contexts=200),
    # tiny CPU-shaped plumbing config
    "tiny": dict(terminal_count=12000, path_count=10000, label_count=5000,
                 embed=100, encode=100, batch=32, contexts=200),
}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", type=str, default="top11", choices=CONFIGS)
    ap.add_argument("--pool", type=int, default=8, help="synthetic batch pool size")
    ap.add_argument("--mode", type=str, default="train", choices=["train", "infer"],
                    help="train: full step (the driver contract); infer: "
                         "hipGraph-captured batched code-vector export "
                         "(BASELINE config 5)")
    ap.add_argument("--real-pipeline", action="store_true",
                    help="route batches through the REAL input pipeline "
                         "(SyntheticReader -> native epoch builder -> "
                         "pinned-staged BatchIterator async H2D) instead "
                         "of a pre-staged device pool")
    ap.add_argument("--methods", type=int, default=605945,
                    help="--real-pipeline corpus size (default: top11's "
                         "method count)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write the last step's "
                         "results as DIR/<name>.npy (float32; large arrays "
                         "as a fixed seeded sample of rows/columns)")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement; a plain run "
                         "does only what the headline figure needs (there "
                         "are no secondary measurements at present)")
    args = ap.parse_args()
    assert args.steps >= 1, "--steps must be at least 1"

    cfg = CONFIGS[args.config]
    ctx = init_distributed("cuda" if torch.cuda.is_available() else "cpu")
    world = ctx.world_size
    assert world == args.gpus or world == 1, (
        f"WORLD_SIZE={world} but --gpus={args.gpus}"
    )
    device = ctx.device
    on_gpu = device.type == "cuda"
    # dropout draws from the global seed (torch's default one differs from
    # process to process); fix it so every run sees the same masks
    torch.manual_seed(123 + ctx.rank)

    opt = Option(
        terminal_count=cfg["terminal_count"], path_count=cfg["path_count"],
        label_count=cfg["label_count"], max_path_length=cfg["contexts"],
        terminal_embed_size=cfg["embed"], path_embed_size=cfg["embed"],
        encode_size=cfg["encode"], dropout_prob=0.25,
        batch_size=cfg["batch"], device=device,
    )
    g = torch.Generator().manual_seed(123)
    if on_gpu:
        model = Code2VecHIP(opt, init_logical_params(opt, g), device=device)
        optim = FusedAdam(model.parameters(), lr=0.01, betas=(0.9, 0.999))
    else:
        from code2vec_amd.models.code2vec import Code2VecTorch

        model = Code2VecTorch(opt, init_logical_params(opt, g))
        optim = torch.optim.Adam(model.parameters(), lr=0.01)

    owned = (
        [model.terminal_embedding, model.path_embedding] if on_gpu else None
    )
    ddp = BucketedAllReduce(list(model.parameters()), world,
                            owned_params=owned)
    ddp.broadcast_parameters()

    B, C = cfg["batch"], cfg["contexts"]
    rng = np.random.default_rng(1000 + ctx.rank)
    pool = []
    if not (args.real_pipeline and args.mode == "train"):
        for _ in range(args.pool):
            s, p, e, y = synthetic_batch(rng, B, C, cfg["terminal_count"],
                                         cfg["path_count"],
                                         cfg["label_count"])
            pool.append(tuple(
                torch.from_numpy(a).to(device) for a in (s, p, e, y)
            ))
    class_weight = torch.ones(cfg["label_count"], device=device)

    if args.mode == "infer":
        run_infer(args, cfg, ctx, model, pool)
        return

    model.train()

    batch_iter = None
    if args.real_pipeline:
        from code2vec_amd.data.builder import DatasetBuilder
        from code2vec_amd.data.synthetic import SyntheticReader
        from code2vec_amd.engine.loader import BatchIterator

        reader = SyntheticReader(
            args.methods, cfg["terminal_count"], cfg["path_count"],
            cfg["label_count"], max_contexts=2 * C, seed=7,
        )
        builder = DatasetBuilder(reader, opt, seed=123, rank=ctx.rank,
                                 world_size=world)
        loader = BatchIterator(builder.refresh_train_dataset(0), B,
                               shuffle=True, seed=5, device=device)

        def cycle():
            while True:
                for hb in loader:
                    if hb["starts"].shape[0] == B:
                        yield hb

        batch_iter = cycle()

    last = {}  # what the last timed step returned (--dump-outputs)

    def step(i: int, keep: bool = False) -> None:
        if batch_iter is not None:
            hb = next(batch_iter)
            s, p, e, y = (hb["starts"], hb["paths"], hb["ends"], hb["label"])
        else:
            s, p, e, y = pool[i % len(pool)]
        ddp.zero_grad()
        outputs, cv, attn = model(s, p, e, y)
        loss = model.loss(outputs, y, class_weight)
        loss.backward()
        if on_gpu:
            ddp.finish_and_step(optim)
        else:
            ddp.finish()
            optim.step()
        if keep:
            last.update(loss=loss, outputs=outputs, code_vector=cv,
                        attention=attn)

    # hipGraph-captured whole training step (N=1 pool mode) — opt-in
    # EXPERIMENT (C2V_GRAPH_STEP=1): capture works and replays bitwise-
    # correctly (the dropout RNG offset and Adam beta^t live in device
    # memory precisely so replays advance them), but MEASURED SLIGHTLY
    # SLOWER than eager (1.441 vs 1.429 ms/step at top11): the eager
    # loop already pipelines enqueue across steps, so graph launch saves
    # nothing here and the per-batch copy into static buffers adds a
    # little.  Kept as validated infrastructure (test
    # test_graph_captured_step_matches_eager).
    graph_note = ""
    if (on_gpu and world == 1 and args.mode == "train"
            and not args.real_pipeline
            and os.environ.get("C2V_GRAPH_STEP", "0") == "1"):
        try:
            static = tuple(t.clone() for t in pool[0])

            def graph_body():
                s, p, e, y = static
                ddp.zero_grad()
                outputs, cv, attn = model(s, p, e, y)
                loss = model.loss(outputs, y, class_weight)
                loss.backward()
                ddp.finish_and_step(optim)
                # static graph memory: holds the latest replay's results
                last.update(loss=loss, outputs=outputs, code_vector=cv,
                            attention=attn)

            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):  # allocator/TunableOp warmup
                    graph_body()
            torch.cuda.current_stream().wait_stream(side)
            # capture records kernels without executing them, so beta^t
            # must already hold the real step count when replay begins
            optim.bc_pow.fill_(1.0)
            for _ in range(optim.step_count):
                optim.bc_pow[0] *= optim.beta1
                optim.bc_pow[1] *= optim.beta2
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                graph_body()

            def graphed_step(i: int, keep: bool = False) -> None:
                for dst, src in zip(static, pool[i % len(pool)]):
                    dst.copy_(src, non_blocking=True)
                graph.replay()

            step = graphed_step
            graph_note = "; step captured in a hipGraph (replayed per batch)"
        except Exception as exc:  # noqa: BLE001 - eager fallback
            if ctx.is_rank0:
                print(f"# hipGraph capture unavailable, eager step: {exc}",
                      file=sys.stderr)

    # --dump-outputs: keep the seeded starting point.  Over many steps the
    # trajectory is not bit-reproducible (the table-grad scatter sums each
    # row's contributions in atomic-placement order, and one flipped bf16
    # rounding then grows with training), so the step whose results are
    # dumped is run from this state: its inputs are the same in every run.
    initial = snapshot_state(model, optim) if args.dump_outputs else None

    for i in range(args.warmup):
        step(i)

    if ctx.initialized:
        torch.distributed.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep_at = args.steps - 1 if args.dump_outputs else -1
    paused = 0.0
    for i in range(args.steps):
        if i == keep_at:
            # the dumped step starts from the seeded initial state; putting
            # it back is not part of a step, so the clock stops meanwhile
            if on_gpu:
                torch.cuda.synchronize()
            t_pause = time.perf_counter()
            restore_state(initial)
            if on_gpu:
                torch.cuda.synchronize()
            paused = time.perf_counter() - t_pause
        step(i, i == keep_at)
    if on_gpu:
        torch.cuda.synchronize()
    if ctx.initialized:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0 - paused

    # MAX over ranks
    if ctx.initialized:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    contexts_per_step = world * B * C
    value = contexts_per_step * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if args.dump_outputs and ctx.is_rank0:
        arrays = {k: v.detach() for k, v in last.items()}
        arrays.update(
            ("param_" + n, p.detach()) for n, p in model.named_parameters())
        dump_outputs(args.dump_outputs, arrays)

    if ctx.is_rank0:
        print(json.dumps({
            "metric": "path_contexts_per_sec",
            "value": value,
            "unit": "path-contexts/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if on_gpu else "fp32",
            "data": ("synthetic (random indices, random-init weights); "
                     "REAL input pipeline: native epoch builder -> pinned "
                     "staging -> async H2D per batch"
                     if args.real_pipeline else
                     "synthetic (dense 200 contexts/method, random indices, "
                     "random-init weights)"),
            "config": {
                "model": f"code2vec-{args.config}",
                "global_batch": world * B,
                "seq_len": C,
                "parallelism": f"dp{world}",
                "terminal_vocab": cfg["terminal_count"],
                "path_vocab": cfg["path_count"],
                "label_vocab": cfg["label_count"],
                "embed": cfg["embed"],
                "encode": cfg["encode"],
                "note": ("step = fwd + fused log-softmax/NLL loss + bwd + bucketed RCCL all-reduce + fused Adam"
                        + ("; top11 label vocab 72,416 derived via Heaps-law fit "
                           "to the reference's real methods.txt name curve "
                           "(tools/derive_label_vocab.py)" if args.config == "top11" else "")
                        + graph_note),
            },
        }))


def snapshot_state(model, optim):
    """Copies of everything a training step reads and updates: parameters,
    optimizer state and the host RNG (the dropout counter restarts at 0)."""
    live = [p.data for p in model.parameters()]
    if isinstance(optim, FusedAdam):
        for st in optim.state.values():
            live += [t for t in st.values() if t is not None]
        live.append(optim.bc_pow)
        host = optim.step_count
    else:
        host = copy.deepcopy(optim.state_dict())
    return (optim, live, [t.clone() for t in live], host,
            torch.get_rng_state())


def restore_state(snap) -> None:
    from code2vec_amd.ops import functional as Fn

    optim, live, saved, host, rng_state = snap
    with torch.no_grad():
        for t, c in zip(live, saved):
            t.copy_(c)
    if isinstance(optim, FusedAdam):
        optim.step_count = host
    else:
        optim.load_state_dict(copy.deepcopy(host))
    torch.set_rng_state(rng_state)
    Fn.reseed_dropout_rng(torch.initial_seed())


DUMP_LIMIT_BYTES = 64 * 1000 * 1000
DUMP_MAX_ROWS = 16384  # rows kept of a 2-D array (the big tables)
DUMP_MAX_COLS = 2048  # columns kept of a 2-D array (the logits)


def dump_outputs(out_dir: str, arrays) -> None:
    """Write each tensor as out_dir/<name>.npy in float32.

    Arrays too large to keep whole are cut to a fixed sample: DUMP_MAX_ROWS
    sorted row indices (DUMP_MAX_COLS column indices for the wide logits),
    drawn by a generator seeded with the axis length, so the same indices
    are chosen by every run and every build.
    """
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        if t.dim() == 2:
            for dim, cap in ((0, DUMP_MAX_ROWS), (1, DUMP_MAX_COLS)):
                n = t.shape[dim]
                if n > cap:
                    idx = np.sort(np.random.default_rng(n).choice(
                        n, size=cap, replace=False))
                    t = t.index_select(
                        dim, torch.from_numpy(idx).to(t.device))
        a = t.float().cpu().numpy()
        total += a.nbytes
        assert total <= DUMP_LIMIT_BYTES, (name, total)
        np.save(os.path.join(out_dir, name + ".npy"), a)


def run_infer(args, cfg, ctx, model, pool) -> None:
    """Inference-only: hipGraph-captured forward, code-vector batches/s."""
    from code2vec_amd.engine.infer import GraphedInference

    device = ctx.device
    B, C = cfg["batch"], cfg["contexts"]
    model.eval()
    graphed = None
    if device.type == "cuda":
        graphed = GraphedInference(model, B, device)

    def step(i: int):
        s, p, e, y = pool[i % len(pool)]
        if graphed is not None:
            return graphed.run(s.int(), p.int(), e.int(), y)
        with torch.no_grad():
            return model(s, p, e, y)

    for i in range(args.warmup):
        step(i)
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = step(i)
    if device.type == "cuda":
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    value = ctx.world_size * B * C * args.steps / elapsed
    if args.dump_outputs and ctx.is_rank0:
        dump_outputs(args.dump_outputs, dict(
            zip(("outputs", "code_vector", "attention"), out)))
    if ctx.is_rank0:
        print(json.dumps({
            "metric": "infer_path_contexts_per_sec",
            "value": value,
            "unit": "path-contexts/s",
            "n_gpus": ctx.world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if device.type == "cuda" else "fp32",
            "data": "synthetic",
            "config": {
                "model": f"code2vec-{args.config}", "global_batch": B,
                "seq_len": C, "parallelism": "dp1",
                "note": "hipGraph-captured batched code-vector export (BASELINE config 5)",
            },
        }))


if __name__ == "__main__":
    main()
