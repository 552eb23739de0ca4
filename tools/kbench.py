#!/usr/bin/env python3
"""Per-op GPU micro-benchmarks (within-process A/B, CUDA events).

Times each framework op at the top11 flagship shape; variants switch via
env vars read by ops/functional.py.  Usage (on a GPU box):
    python tools/kbench.py [op ...]
``row_topk`` (K19 vs torch.topk + torch.logsumexp), ``table_adam``
(scatter + cast_clear + adam_bf16 vs the row-gathering table Adam) and
``bwd_fusions`` (one-launch reductions, compact attention backward and
recomputing combiner backward vs what they replace) and ``group_tables``
(both tables' counting sort: the global-atomic chain vs the LDS buckets) and
``attn_stream`` (streaming attention forward/backward and the combiner's
score-emitting flush vs the tiled kernels) and ``head_bwd_pipe`` (the
pipelined head backward and wgrad kernels vs the ones they replace) are
not in the default set; asked for alone they skip building the model-shaped
operands.
"""

from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import round_up


def timeit(fn, iters=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1000  # us


def bench_row_topk(dev, results, rounds=5):
    """K19 row_topk vs the stock torch.topk + torch.logsumexp pair on the
    SAME tensor, alternating the two within each round (median / min over
    rounds).  Shapes: the prediction head at B = 1024, k = 10 for each L
    in C2V_KBENCH_TOPK_L (bf16 logits), plus the attention shape
    (1024, 200) fp32."""
    B, k = 1024, 10
    Ls = [int(v) for v in os.environ.get(
        "C2V_KBENCH_TOPK_L", "72416,261245").split(",")]
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = [(L, torch.bfloat16) for L in Ls] + [(200, torch.float32)]
    for L, dtype in shapes:
        x = torch.randn(B, L, generator=g, device=dev)
        if dtype == torch.float32:
            x = torch.softmax(x, dim=1)
        x = x.to(dtype).contiguous()
        tag = f"L={L},{'bf16' if dtype == torch.bfloat16 else 'f32'}"

        def ours():
            return Fn.row_topk(x, k)

        def pair():
            return torch.topk(x, k, dim=1), torch.logsumexp(x, dim=1)

        iters = 20 if L > 1000 else 200
        t_ours, t_pair = [], []
        for _ in range(rounds):
            t_ours.append(timeit(ours, iters=iters))
            t_pair.append(timeit(pair, iters=iters))
        t_ours.sort()
        t_pair.sort()
        results[f"row_topk({tag}) med"] = t_ours[rounds // 2]
        results[f"row_topk({tag}) min"] = t_ours[0]
        results[f"topk+lse({tag}) med"] = t_pair[rounds // 2]
        results[f"topk+lse({tag}) min"] = t_pair[0]
        gbs = x.numel() * x.element_size() / (t_ours[rounds // 2] * 1e-6) / 1e9
        print(f"# row_topk {tag}: {gbs:.0f} GB/s of input read (median)")
        del x


def bench_table_adam(dev, results, rounds=5):
    """Table optimizer step from one grouped gradient, old against new on
    the SAME buffers, alternating within each round (median / min):
      old: embed_scatter_sorted + cast_clear_rows + adam_step_bf16
      new: embed_scatter_heavy + adam_table_bf16 (+ its counts clear)
    at the top11 table shapes (term: 2M entries, two offsets; path: M
    entries) with uniform indices over [1, rows).  The counting sort runs
    once outside the timed region; each timed call first restores the
    histogram it consumes (a 1.4-MB copy, in both variants)."""
    from code2vec_amd.ops import ext

    S, KP, M = 104, 320, 1024 * 200  # M = B * C contexts
    thr = Fn._TABLE_ADAM_HEAVY
    g = torch.Generator(device=dev).manual_seed(0)
    gout = torch.randn(M, KP, generator=g, device=dev).to(torch.bfloat16)
    for tag, T, N, off0, off1 in (("term", 360632, 2 * M, 0, 2 * S),
                                  ("path", 342846, M, S, S)):
        idx = torch.randint(1, T, (N,), generator=g, device=dev,
                            dtype=torch.int32)
        sorted_idx, perm, counts0, cursor = Fn._group_by_index(
            idx, T, with_cursor=True)
        counts = counts0.clone()
        p = (torch.randn(T, S, generator=g, device=dev) * 0.1).to(
            torch.bfloat16)
        master = p.float().view(-1).clone()
        m = torch.zeros(T * S, device=dev)
        v = torch.zeros(T * S, device=dev)
        scratch = torch.zeros(T, S, device=dev)
        flags = torch.zeros(T, dtype=torch.uint8, device=dev)
        dense = torch.empty(T, S, dtype=torch.bfloat16, device=dev)
        bc_pow = torch.full((2,), 0.5, dtype=torch.float64, device=dev)
        hp = (0.01, 0.9, 0.999, 1e-8, 0.0)

        def old():
            counts.copy_(counts0)
            ext().embed_scatter_sorted(sorted_idx, perm, gout, scratch,
                                       dense, flags, M, KP, off0, off1, 16)
            ext().cast_clear_rows(scratch, counts, flags, dense)
            Fn.adam_step(p, dense, master, m, v, bc_pow, *hp)

        def new():
            counts.copy_(counts0)
            ext().embed_scatter_heavy(sorted_idx, perm, counts, gout,
                                      scratch, M, KP, off0, off1, thr)
            ext().adam_table_bf16(p, gout, perm, counts, cursor, scratch,
                                  master, m, v, bc_pow, M, KP, off0, off1,
                                  thr, *hp)

        def dense_only():  # the streaming floor the new kernel is set against
            Fn.adam_step(p, dense, master, m, v, bc_pow, *hp)

        t = {"old": [], "new": [], "adam_bf16 alone": []}
        for _ in range(rounds):
            t["old"].append(timeit(old, iters=20))
            t["new"].append(timeit(new, iters=20))
            t["adam_bf16 alone"].append(timeit(dense_only, iters=20))
        for name, vals in t.items():
            vals.sort()
            results[f"table_adam({tag}) {name} med"] = vals[rounds // 2]
            results[f"table_adam({tag}) {name} min"] = vals[0]
        # bytes the new path has to move: 28 B/param of state traffic,
        # the gathered gradient rows, and the run metadata
        nbytes = T * S * 28 + N * S * 2 + N * 8 + (T + 1) * 12
        gbs = nbytes / (t["new"][rounds // 2] * 1e-6) / 1e9
        print(f"# table_adam {tag}: {gbs:.0f} GB/s effective (median, new)")


def bench_group_tables(dev, results, rounds=5):
    """Counting sort of both tables' index lists: the global-atomic chain
    (C2V_GROUP_SORT=0: count, scan partials, scan apply, group) against the
    two-level sort by LDS buckets, on the SAME persistent buffers,
    alternating within each round (median / min).  Both are followed by the
    clear_i32_pair the table Adam pays afterwards, so both leave the
    histograms zero.  Top11 shapes; inputs: uniform indices over [1, rows),
    a ragged batch (half <PAD/>), and a hot row (25 % of all entries on one
    index >= 2).  C2V_KBENCH_GROUP_SWEEP=1 adds the R x tile sweep of the
    new chain (the launcher reads the switches on every call)."""
    from code2vec_amd.ops import ext

    M, T, P = 1024 * 200, 360632, 342846
    g = torch.Generator(device=dev).manual_seed(0)
    switches = ("C2V_GROUP_SORT", "C2V_GROUP_R", "C2V_GROUP_TILE")
    saved = {k: os.environ.pop(k, None) for k in switches}
    sweep = [(r, t) for r in (1024, 2048, 4096) for t in (1024, 2048, 4096)] \
        if os.environ.get("C2V_KBENCH_GROUP_SWEEP") == "1" else []
    for tag in ("uniform", "half-pad", "hot-row"):
        starts = torch.randint(1, T, (1024, 200), generator=g, device=dev,
                               dtype=torch.int32)
        paths = torch.randint(1, P, (1024, 200), generator=g, device=dev,
                              dtype=torch.int32)
        ends = torch.randint(1, T, (1024, 200), generator=g, device=dev,
                             dtype=torch.int32)
        if tag == "half-pad":
            for t in (starts, paths, ends):
                t[:, 100:] = 0
        if tag == "hot-row":
            for t in (starts, paths, ends):
                hot = torch.rand(t.shape, generator=g, device=dev) < 0.25
                t[hot] = 12345
        bufs = {}
        for name, rows, n in (("term", T + 1, 2 * M), ("path", P + 1, M)):
            bufs[name] = (
                Fn._scratch_i32(f"gsorted_{name}", n, dev, zero=False),
                Fn._scratch_i64(f"gperm_{name}", n, dev),
                Fn._scratch_i32(f"counts_{name}", rows, dev),
                Fn._scratch_i32(f"cursor_{name}", rows, dev, zero=False))
        spart = Fn._scratch_i32(
            "gscanp", int(ext().group_tables_partials_len(T + 1, P + 1)),
            dev, zero=False)
        gtmp = Fn._scratch_i32(
            "gtmp", int(ext().group_tables_tmp_len(M, T + 1, P + 1)), dev,
            zero=False)
        bt, bp = bufs["term"], bufs["path"]

        def chain():
            ext().group_tables(starts, paths, ends, bt[2], bp[2], bt[3],
                               bp[3], spart, bt[0], bt[1], bp[0], bp[1],
                               T + 1, P + 1, False, gtmp)
            ext().clear_i32_pair(bt[2], bp[2])

        def run(env):
            for k in switches:
                os.environ.pop(k, None)
            os.environ.update(env)
            return timeit(chain, iters=50)

        variants = {"old": {"C2V_GROUP_SORT": "0"}, "new": {}}
        for r, tl in sweep:
            variants[f"new R={r} tile={tl}"] = {"C2V_GROUP_R": str(r),
                                                "C2V_GROUP_TILE": str(tl)}
        t = {name: [] for name in variants}
        for _ in range(rounds):
            for name, env in variants.items():
                t[name].append(run(env))
        for name, vals in t.items():
            vals.sort()
            results[f"group_tables({tag}) {name} med"] = vals[rounds // 2]
            results[f"group_tables({tag}) {name} min"] = vals[0]
    for k in switches:
        os.environ.pop(k, None)
        if saved[k] is not None:
            os.environ[k] = saved[k]


def bench_bwd_fusions(dev, results, rounds=5):
    """The one-launch reductions against what they replace on the SAME
    buffers, alternating within each round (median / min), at top11 shapes:
      wgrad_reduce [256, 320, 128] f32 -> [128, 320] bf16
        vs torch sum -> .t().contiguous() -> .to(bf16)
      slab_sum_bf16 [71, 1024*128]: 8 loads in flight per chain vs 1 (the
        launcher reads C2V_SLAB_U8 once per process: run this case a second
        time with C2V_SLAB_U8=0 for the old kernel's number)
      dcv/attn/ds-recomputing combiner_bwd vs the dout-reading one, and
      compact vs dense attention_bwd."""
    from code2vec_amd.ops import ext

    g = torch.Generator(device=dev).manual_seed(0)
    S, KP, EP = 256, 320, 128
    part = torch.randn(S, KP, EP, generator=g, device=dev)
    dw = torch.empty(EP, KP, dtype=torch.bfloat16, device=dev)
    slabs = torch.randn(71, 1024 * 128, generator=g, device=dev)
    dcv_o = torch.empty(1024, 128, dtype=torch.bfloat16, device=dev)

    B, C, E = 1024, 200, 100
    M = B * C
    ccv = torch.tanh(torch.randn(B, C, EP, generator=g, device=dev)).to(
        torch.bfloat16)
    ccv[:, :, E:] = 0
    a = torch.randn(EP, generator=g, device=dev) * 0.2
    a[E:] = 0
    starts = torch.randint(1, 1000, (B, C), generator=g, device=dev,
                           dtype=torch.int32)
    cv = torch.empty(B, EP, device=dev)
    attn = torch.empty(B, C, device=dev)
    ext().attention_fwd(ccv, a, starts, cv, attn, E)
    dcvb = (torch.randn(B, EP, generator=g, device=dev) * 0.1).to(
        torch.bfloat16)
    dcv32 = dcvb.float()
    dccv = torch.empty_like(ccv)
    ds = torch.empty(M, device=dev)
    da_p = torch.empty(B, EP, device=dev)
    none = torch.empty(0, device=dev)
    z = torch.randn(M, EP, generator=g, device=dev).to(torch.bfloat16)
    mean = torch.zeros(M, device=dev)
    rstd = torch.ones(M, device=dev)
    gamma = torch.rand(EP, generator=g, device=dev) + 0.5
    beta = torch.zeros(EP, device=dev)
    dz = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
    dg_p = torch.empty(1024, EP, device=dev)
    db_p = torch.empty(1024, EP, device=dev)
    out2 = ccv.view(M, EP)

    cases = {
        "wgrad_reduce new": lambda: ext().wgrad_reduce(part, dw),
        "wgrad_reduce torch chain": lambda: part.sum(dim=0).t().contiguous()
        .to(torch.bfloat16),
        "slab_sum_bf16 [71,131072]": lambda: ext().slab_sum_bf16(slabs,
                                                                 dcv_o),
        "attention_bwd dense": lambda: ext().attention_bwd(
            dcv32, none, ccv, a, starts, attn, dccv, da_p, E, False),
        "attention_bwd compact": lambda: ext().attention_bwd_compact(
            dcvb, none, ccv, a, starts, attn, ds, da_p, E, False),
        "combiner_bwd dout": lambda: ext().combiner_bwd(
            dccv.view(M, EP), z, out2, mean, rstd, gamma, beta, dz, dg_p,
            db_p, E, 0.25),
        "combiner_bwd recompute": lambda: ext().combiner_bwd_recompute(
            attn.view(-1), ds, dcvb, a, C, z, out2, mean, rstd, gamma, beta,
            dz, dg_p, db_p, E, 0.25),
    }
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            t[k].append(timeit(fn, iters=20))
    for k, vals in t.items():
        vals.sort()
        results[f"{k} med"] = vals[rounds // 2]
        results[f"{k} min"] = vals[0]


def bench_attn_stream(dev, results, rounds=5):
    """The streaming attention pool against the tiled kernels on the SAME
    buffers, alternating within each round (median / min), at the top11
    shape B=1024, C=200, KP=320 with 30% of the contexts masked:
      attention forward: tiled (scores + pool from the LDS tile) vs
        attention_fwd_scores (scores given, rows prefetched to registers)
      compact attention backward: tiled vs rows-in-registers
      combiner_fwd without and with the score-emitting flush."""
    from code2vec_amd.ops import ext

    g = torch.Generator(device=dev).manual_seed(0)
    B, C, E, EP, KP = 1024, 200, 100, 128, 320
    M = B * C
    x = torch.randn(M, KP, generator=g, device=dev).to(torch.bfloat16)
    w = torch.zeros(EP, KP, device=dev)
    w[:E] = torch.randn(E, KP, generator=g, device=dev) * (0.4 / KP ** 0.5)
    w = w.to(torch.bfloat16)
    gamma = torch.zeros(EP, device=dev)
    gamma[:E] = torch.rand(E, generator=g, device=dev) + 0.5
    beta = torch.zeros(EP, device=dev)
    a = torch.zeros(EP, device=dev)
    a[:E] = torch.randn(E, generator=g, device=dev) * 0.2
    starts = torch.randint(1, 1000, (B, C), generator=g, device=dev,
                           dtype=torch.int32)
    starts[torch.rand(B, C, generator=g, device=dev) < 0.3] = 0
    out = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
    z = torch.empty_like(out)
    mean = torch.empty(M, device=dev)
    rstd = torch.empty(M, device=dev)
    raw = torch.empty(M, device=dev)
    Fn.reseed_dropout_rng(1234)
    seed, off_t = Fn._philox_state(dev)
    cv = torch.empty(B, EP, device=dev)
    cvb = torch.empty(B, EP, dtype=torch.bfloat16, device=dev)
    attn = torch.empty(B, C, device=dev)
    assert ext().combiner_fwd_scores(x, w, gamma, beta, a, out, z, mean,
                                     rstd, raw, E, 0.25, seed, off_t, 1)
    ccv = out.view(B, C, EP)
    ext().attention_fwd_cvb(ccv, a, starts, cv, cvb, attn, E)
    dcvb = (torch.randn(B, EP, generator=g, device=dev) * 0.1).to(
        torch.bfloat16)
    ds = torch.empty(M, device=dev)
    da_p = torch.empty(B, EP, device=dev)
    none = torch.empty(0, device=dev)

    cases = {
        "attention_fwd tiled": lambda: ext().attention_fwd_cvb(
            ccv, a, starts, cv, cvb, attn, E),
        "attention_fwd_scores": lambda: ext().attention_fwd_scores(
            ccv, raw, starts, cv, cvb, attn, E),
        "attention_bwd compact tiled": lambda: ext().attention_bwd_compact(
            dcvb, none, ccv, a, starts, attn, ds, da_p, E, False),
        "attention_bwd compact reg": lambda: ext().attention_bwd_compact_reg(
            dcvb, none, ccv, starts, attn, ds, da_p, E, False),
        "combiner_fwd": lambda: ext().combiner_fwd(
            x, w, gamma, beta, out, z, mean, rstd, E, 0.25, seed, off_t, 1),
        "combiner_fwd + scores": lambda: ext().combiner_fwd_scores(
            x, w, gamma, beta, a, out, z, mean, rstd, raw, E, 0.25, seed,
            off_t, 1),
    }
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            t[k].append(timeit(fn, iters=20))
    for k, vals in t.items():
        vals.sort()
        results[f"{k} med"] = vals[rounds // 2]
        results[f"{k} min"] = vals[0]


def bench_head_bwd_pipe(dev, results, rounds=5):
    """The pipelined head backward and wgrad kernels against the ones they
    replace on the SAME buffers, alternating within each round (median /
    min), at the top11 shapes: head B=1024, L=72,416 (dw + dbias, dcv
    slabs at chunk 1024) and wgrad M=204,800, KP=320, EP=128, 256 slabs.
    Every depth / buffering instantiation is timed (the sweep), and with
    C2V_KBENCH_HBDW_VARIANTS=1 also the phase-isolation variants of the old
    and the new dw kernel (4 = no logits loads, 2 = no B loads, 16 = no
    MFMA)."""
    from code2vec_amd.ops import ext

    g = torch.Generator(device=dev).manual_seed(0)
    B, L, EP = 1024, 72416, 128
    logits = (torch.randn(B, L, generator=g, device=dev) * 3.0).to(
        torch.bfloat16)
    label = torch.randint(0, L, (B,), generator=g, device=dev)
    weight = torch.rand(L, generator=g, device=dev) + 0.5
    lse = torch.logsumexp(logits.float(), dim=1).contiguous()
    acc = torch.stack([torch.zeros((), device=dev), weight[label].sum()])
    coef_lse = torch.zeros(B, 4, device=dev)
    ext().head_bwd_prep(label, weight, acc, torch.ones(1, device=dev), lse,
                        coef_lse)
    cv = (torch.randn(B, EP, generator=g, device=dev) * 0.5).to(
        torch.bfloat16)
    cvimg = torch.empty((B + 63) // 64 * 2, 8, 64, 8, dtype=torch.bfloat16,
                        device=dev)
    ext().swizzle_cv(cv, cvimg)
    wout = (torch.randn(L, EP, generator=g, device=dev) * 0.05).to(
        torch.bfloat16)
    wimg = torch.empty((L + 127) // 128 * 4, 8, 64, 8, dtype=torch.bfloat16,
                       device=dev)
    ext().swizzle_cv(wout, wimg)
    dw = torch.empty(L, EP, dtype=torch.bfloat16, device=dev)
    dbias = torch.empty(L, device=dev)
    chunk = 1024
    partials = torch.empty((L + chunk - 1) // chunk, B, EP, device=dev)
    M, KP = 204800, 320
    x = torch.randn(M, KP, generator=g, device=dev).to(torch.bfloat16)
    dz = (torch.randn(M, EP, generator=g, device=dev) * 0.3).to(
        torch.bfloat16)
    wpart = torch.empty(256, KP, EP, device=dev)

    cases = {"head_bwd_dw": lambda: ext().head_bwd_dw(
        logits, cvimg, coef_lse, dw, dbias)}
    for d in (1, 2):
        cases[f"head_bwd_dw_pipe D={d}"] = (
            lambda d=d: ext().head_bwd_dw_pipe(logits, cvimg, coef_lse, dw,
                                               dbias, d))
    cases["head_bwd_dcv"] = lambda: ext().head_bwd_dcv(
        logits, wimg, coef_lse, partials, chunk)
    for b in (0, 1):
        cases[f"head_bwd_dcv_pipe dbuf={b}"] = (
            lambda b=b: ext().head_bwd_dcv_pipe(logits, wimg, coef_lse,
                                                partials, chunk, b))
    cases["wgrad"] = lambda: ext().wgrad(x, dz, wpart)
    cases["wgrad_pipe H=2"] = lambda: ext().wgrad_pipe(x, dz, wpart, 2)

    def with_variant(v, fn):
        def run():
            os.environ["C2V_HBDW_VARIANT"] = str(v)
            try:
                fn()
            finally:
                del os.environ["C2V_HBDW_VARIANT"]
        return run

    if os.environ.get("C2V_KBENCH_HBDW_VARIANTS") == "1":
        for v in (4, 2, 16):
            cases[f"head_bwd_dw variant={v}"] = with_variant(
                v, cases["head_bwd_dw"])
            cases[f"head_bwd_dw_pipe variant={v}"] = with_variant(
                v, lambda: ext().head_bwd_dw_pipe(logits, cvimg, coef_lse,
                                                  dw, dbias, 0))
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            t[k].append(timeit(fn, iters=20))
    for k, vals in t.items():
        vals.sort()
        results[f"{k} med"] = vals[rounds // 2]
        results[f"{k} min"] = vals[0]


def main():
    if "--help" in sys.argv or "-h" in sys.argv:
        print(__doc__.strip())
        return
    if not torch.cuda.is_available():
        print("kbench: needs a GPU (per-kernel timing); run under gpurun")
        return
    dev = torch.device("cuda:0")
    if sys.argv[1:] in (["row_topk"], ["table_adam"], ["bwd_fusions"],
                        ["group_tables"], ["attn_stream"],
                        ["head_bwd_pipe"]):
        # needs none of the model-shaped operands built below
        results = {}
        if sys.argv[1] == "row_topk":
            bench_row_topk(dev, results)
        elif sys.argv[1] == "attn_stream":
            bench_attn_stream(dev, results)
        elif sys.argv[1] == "head_bwd_pipe":
            bench_head_bwd_pipe(dev, results)
        elif sys.argv[1] == "bwd_fusions":
            bench_bwd_fusions(dev, results)
        elif sys.argv[1] == "group_tables":
            bench_group_tables(dev, results)
        else:
            bench_table_adam(dev, results)
        for k, vv in results.items():
            print(f"{k:40s} {vv:10.1f} us")
        return
    B, C = 1024, 200
    T, P, L = 360632, 342846, 30000
    L = int(os.environ.get("C2V_KBENCH_L", L))  # e.g. 261000 (java-large)
    T = int(os.environ.get("C2V_KBENCH_T", T))
    dt = dp = E = 100
    TS, PS, EP = round_up(dt), round_up(dp), round_up(E)
    KP = 2 * TS + PS
    M = B * C
    g = torch.Generator(device=dev).manual_seed(0)

    term = torch.randn(T, TS, generator=g, device=dev).to(torch.bfloat16)
    path = torch.randn(P, PS, generator=g, device=dev).to(torch.bfloat16)
    starts = torch.randint(1, T, (B, C), generator=g, device=dev, dtype=torch.int32)
    pth = torch.randint(1, P, (B, C), generator=g, device=dev, dtype=torch.int32)
    ends = torch.randint(1, T, (B, C), generator=g, device=dev, dtype=torch.int32)
    x = Fn.GatherConcat.apply(starts, pth, ends, term, path)
    w = (torch.randn(EP, KP, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    gamma = torch.rand(EP, generator=g, device=dev) + 0.5
    beta = torch.randn(EP, generator=g, device=dev) * 0.1
    a = torch.randn(EP, generator=g, device=dev) * 0.2
    wout = (torch.randn(L, EP, generator=g, device=dev) * 0.05).to(torch.bfloat16)
    label = torch.randint(0, L, (B,), generator=g, device=dev)
    weight = torch.ones(L, device=dev)

    ops = sys.argv[1:] or ["gather_fwd", "gather_bwd", "combiner_fwd",
                           "combiner_bwd", "attention", "lsm", "adam",
                           "wgrad"]
    results = {}

    if "gather_fwd" in ops:
        results["gather_fwd"] = timeit(
            lambda: Fn.GatherConcat.apply(starts, pth, ends, term, path))

    if "gather_bwd" in ops:
        xg = None
        def run():
            nonlocal xg
            t2 = term.detach().requires_grad_(True)
            p2 = path.detach().requires_grad_(True)
            o = Fn.GatherConcat.apply(starts, pth, ends, t2, p2)
            o.backward(x)
        results["gather_bwd(all)"] = timeit(run, iters=15)

    if "combiner_fwd" in ops:
        results["combiner_fwd"] = timeit(
            lambda: Fn.CombinerLNTanh.apply(x, w, gamma, beta, E, 0.25, True))

    if "combiner_bwd" in ops:
        def run():
            x2 = x.detach().requires_grad_(True)
            w2 = w.detach().requires_grad_(True)
            o = Fn.CombinerLNTanh.apply(x2, w2, gamma, beta, E, 0.0, False)
            o.backward(o.detach())
        results["combiner_fwd+bwd(all)"] = timeit(run, iters=15)

    ccv = Fn.CombinerLNTanh.apply(x, w, gamma, beta, E, 0.0, False).view(B, C, EP)
    if "attention" in ops:
        results["attention_fwd"] = timeit(
            lambda: Fn.AttentionPool.apply(ccv, a, starts, E))

    if "lsm" in ops:
        cv, _ = Fn.AttentionPool.apply(ccv, a, starts, E)
        logits = (cv.to(torch.bfloat16) @ wout.t()).contiguous()
        results["lsm_fwd"] = timeit(
            lambda: Fn.FusedLogSoftmaxNLL.apply(logits, label, weight))

    if "membw" in ops:
        # same-box streaming ceiling: D2D copy (read+write) of 2 GB
        src = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)
        src.fill_(1.0)
        t = timeit(lambda: dst.copy_(src), iters=10)
        results["d2d_copy(2GB r+w)"] = t
        print(f"# copy bandwidth: {2 * src.numel() * 4 / (t * 1e-6) / 1e12:.2f} TB/s")

    if "adam" in ops:
        p1 = term.clone().view(-1)
        g1 = term.clone().view(-1)
        master = p1.float()
        m = torch.zeros_like(master)
        v = torch.zeros_like(master)
        from code2vec_amd.ops import ext
        bc = torch.full((2,), 0.5, dtype=torch.float64, device=dev)
        results["adam(term)"] = timeit(
            lambda: ext().adam_step_bf16(p1, g1, master, m, v, bc, 0.01,
                                         0.9, 0.999, 1e-8, 0.0))

    if "wgrad" in ops:
        dz = ccv.view(M, EP).contiguous()
        partials = torch.empty(256, KP, EP, dtype=torch.float32, device=dev)
        from code2vec_amd.ops import ext
        results["wgrad"] = timeit(lambda: ext().wgrad(x, dz, partials))

    if "head_fwd" in ops:
        from code2vec_amd.ops import ext
        cv, _ = Fn.AttentionPool.apply(ccv, a, starts, E)
        cvb = cv.to(torch.bfloat16).contiguous()
        bias = torch.zeros(L, device=dev)
        logits = torch.empty(B, L, dtype=torch.bfloat16, device=dev)
        gx = (L + 255) // 256
        pm = torch.empty(gx, B, dtype=torch.float32, device=dev)
        ps = torch.empty_like(pm)
        nil = torch.Tensor()
        results["head_fwd(no stats)"] = timeit(
            lambda: ext().head_fwd(cvb, wout, bias, logits, nil, nil),
            iters=10)
        results["head_fwd(stats)"] = timeit(
            lambda: ext().head_fwd(cvb, wout, bias, logits, pm, ps),
            iters=10)
        lse = torch.empty(B, dtype=torch.float32, device=dev)
        acc_f = torch.empty((B + 15) // 16, 2, dtype=torch.float32, device=dev)
        results["lsm_finalize"] = timeit(
            lambda: ext().logsoftmax_nll_finalize(logits, pm, ps, label,
                                                  weight, lse, acc_f),
            iters=10)
        gx2 = (L + 16383) // 16384
        pm2 = torch.empty(gx2, B, dtype=torch.float32, device=dev)
        ps2 = torch.empty_like(pm2)
        results["lsm_partial+final"] = timeit(
            lambda: (ext().lsm_partial(logits, pm2, ps2),
                     ext().logsoftmax_nll_finalize(logits, pm2, ps2, label,
                                                   weight, lse, acc_f)),
            iters=10)
        acc_b = torch.empty(B, 2, dtype=torch.float32, device=dev)
        results["lsm_full_fwd"] = timeit(
            lambda: ext().logsoftmax_nll_fwd(logits, label, weight, lse,
                                             acc_b), iters=10)
        bias_h = bias.to(torch.bfloat16)
        results["linear(hipblaslt)"] = timeit(
            lambda: torch.nn.functional.linear(cvb, wout, bias_h), iters=10)
        wimg_a = torch.empty((L + 255) // 256 * 16, 4, 64, 8,
                             dtype=torch.bfloat16, device=dev)
        ext().swizzle_a(wout, wimg_a)
        results["swizzle_a"] = timeit(lambda: ext().swizzle_a(wout, wimg_a),
                                      iters=10)
        results["head_fwd_img(stats)"] = timeit(
            lambda: ext().head_fwd_img(cvb, wimg_a, bias, logits, pm, ps,
                                       L), iters=10)

    if "head_bwd" in ops:
        from code2vec_amd.ops import ext
        cv, _ = Fn.AttentionPool.apply(ccv, a, starts, E)
        cvb = cv.to(torch.bfloat16).contiguous()
        bias = torch.zeros(L, device=dev)
        logits = torch.empty(B, L, dtype=torch.bfloat16, device=dev)
        gx = (L + 255) // 256
        pm = torch.empty(gx, B, dtype=torch.float32, device=dev)
        ps = torch.empty_like(pm)
        ext().head_fwd(cvb, wout, bias, logits, pm, ps)
        lse = torch.empty(B, dtype=torch.float32, device=dev)
        acc_f = torch.empty((B + 15) // 16, 2, dtype=torch.float32, device=dev)
        ext().logsoftmax_nll_finalize(logits, pm, ps, label, weight, lse, acc_f)
        acc = torch.empty(2, dtype=torch.float32, device=dev)
        ext().slab_sum_f32(acc_f, acc)
        g1 = torch.ones(1, device=dev)
        coef_lse = torch.zeros(B, 4, device=dev)
        ext().head_bwd_prep(label, weight, acc, g1, lse, coef_lse)
        nchunk = (B + 63) // 64 * 2
        cvimg = torch.empty(nchunk, 8, 64, 8, dtype=torch.bfloat16, device=dev)
        ext().swizzle_cv(cvb, cvimg)
        dw = torch.empty(L, 128, dtype=torch.bfloat16, device=dev)
        dbias = torch.empty(L, dtype=torch.float32, device=dev)
        results["swizzle_cv"] = timeit(lambda: ext().swizzle_cv(cvb, cvimg))
        results["head_bwd_dw"] = timeit(
            lambda: ext().head_bwd_dw(logits, cvimg, coef_lse, dw, dbias))
        chunk = int(os.environ.get("C2V_HB_DCV_CHUNK", "0")) or (
            1024 if L <= 131072 else 4096)
        split = (L + chunk - 1) // chunk
        partials = torch.empty(split, B, 128, dtype=torch.float32, device=dev)
        wimg = torch.empty((L + 127) // 128 * 4, 8, 64, 8,
                           dtype=torch.bfloat16, device=dev)
        ext().swizzle_cv(wout, wimg)
        results["swizzle_w"] = timeit(lambda: ext().swizzle_cv(wout, wimg))
        results["head_bwd_dcv"] = timeit(
            lambda: ext().head_bwd_dcv(logits, wimg, coef_lse, partials,
                                       chunk))
        wimg_a = torch.empty((L + 255) // 256 * 16, 4, 64, 8,
                             dtype=torch.bfloat16, device=dev)
        ext().swizzle_a(wout, wimg_a)
        cvimg_a = torch.empty((B + 255) // 256 * 16, 4, 64, 8,
                              dtype=torch.bfloat16, device=dev)
        ext().swizzle_a(cvb, cvimg_a)
        results["swizzle_a(cv)"] = timeit(
            lambda: ext().swizzle_a(cvb, cvimg_a))
        results["head_bwd_dcv_rc"] = timeit(
            lambda: ext().head_bwd_dcv_rc(cvimg_a, wimg_a, wimg, bias,
                                          coef_lse, partials, B, L, chunk))

    if "row_topk" in ops:
        bench_row_topk(dev, results)
    if "table_adam" in ops:
        bench_table_adam(dev, results)
    if "group_tables" in ops:
        bench_group_tables(dev, results)

    for k, vv in results.items():
        print(f"{k:24s} {vv:10.1f} us")


if __name__ == "__main__":
    main()
