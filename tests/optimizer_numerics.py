"""Elementwise fp64 tolerance rule for the half of the training step that
writes the parameters: the embedding-gradient scatter (K13), the Adam kernels
(K16, the fp32 and multi-tensor forms) and the row-gathering table Adam (K16b).

Not a test file: the fp64 references, the bounds and the planted data of
test_optimizer_numerics_cpu.py and test_optimizer_numerics_gpu.py.  The rule
itself (``assert_within``: every element within its bound, none excluded, no
norm) and ``U = 2^-8``, ``E24 = 2^-24`` come from head_numerics.py.

Every reference is fp64 arithmetic on the tensors the kernel was given (bf16
values as stored, upcast; the optimizer state as it stood before the step),
and every later quantity is judged from what the kernel itself stored for the
earlier one.  ``mag`` is the reference with every term replaced by its
absolute value.  The counts below are first-order counts of rounded fp32
operations; every bound is multiplied by ``SECOND = 1 + 2^-20``, which covers
the second-order terms of a chain of k <= 16 roundings (k^2 u^2 / 2 <=
k u 2^-20).  No constant is fitted to an observed error.

Table gradient (embed_scatter_sorted + cast_clear_rows; the gradient that
adam_table_bf16 and embed_scatter_heavy rebuild):

  g64[r] = sum over the n_r entries o of row r of gout[o, off0 + col]
  (o < M) or gout[o - M, off1 + col] (o >= M).
  row 0 (<PAD/>)     exactly 0 whatever gout holds: embed_scatter_sorted's
                     flush, scatter_heavy_chunk (first > 0, last > 0) and
                     adam_table_bf16_kernel (row != 0) all skip index 0
  untouched rows     exactly 0
  touched rows       U|ref| + (n_r + 2) 2^-24 mag
                     (n_r - 1 fp32 additions in ANY order, which covers the
                     16-entry chunk partials and the fp32 atomics that combine
                     them: (n_r - 1) 2^-24 mag; the one rounding to bf16:
                     U|ref| plus U times the accumulation error, below
                     2 2^-24 mag for n_r <= 512, with the +1 left as slack;
                     table_grad_ref asserts n_r <= 512)

Adam (adam_update4 in adam_bf16_kernel and adam_table_bf16_kernel; the scalar
source of adam_bf16_kernel's tail, adam_f32_kernel, adam_f32_multi_kernel).
lr, b1, b2, eps, wd are the fp32-rounded values the bindings pass; 1 - b is
formed in fp32 as in the kernel (exact for b in [0.5, 1]); the bias-correction
powers are the fp64 pair read back from bc_pow.  ``p`` is what the kernel
reads as the parameter: the fp32 master for bf16 parameters.  G = g + wd p.

  m' = b1 m + (1 - b1) G        4 2^-24 mag
       (longest chain: wd p, + g, (1 - b1) G, the final add; adam_update4
       fuses the first two and, in lanes 0-1, the last two: 3 or fewer)
  v' = b2 v + (1 - b2) G^2      6 2^-24 mag in adam_update4: G is one FMA
       (1 rounding, counted twice in G^2), (1 - b2) G, times G, the final
       add: 5, +1 slack;  7 2^-24 mag in the scalar source, where G may take
       two roundings (wd p, then + g: 4 on G^2) before the same three
       operations.  This differs from a flat 6: the scalar source written out
       without contraction reaches 7 when wd != 0.
  upd = lr (m' ibc1) / (sqrt(v' ibc2) + eps),  p' = p - upd, both from the
       STORED m', v':           2^-24 |p'| + 8 2^-24 |upd|
       (float(ibc1), m' ibc1, lr *, the divide: 4; float(ibc2), v' ibc2
       halved by the square root, sqrtf, + eps: 3; 7 in all, +1 slack; the
       final subtraction: half an ulp of p').  setup.py passes no fast-math
       flag: sqrtf and the divide are correctly rounded.
  bf16 parameter                bit-equal to master'.to(bfloat16)

K16b on arbitrary gradients: the rounded bf16 gradient is not stored, so with
dg the table-gradient bound above

  m'   (1 - b1) dg + 4 2^-24 mag
  v'   (1 - b2) (2 |G| dg + dg^2) + 6 2^-24 mag
  master and parameter from the stored m', v' exactly as above.

Where the gradient is known exactly dg = 0 and the plain Adam bounds apply:
row 0 and untouched rows (g = 0), and the integer-gradient case, where every
fp32 partial sum is exact in any order and g is the one rounding to bf16 of
the exact sum.

Planted data, built by seeded generators on the CPU.

run_plan(thr, total, rows): (row, count) pairs ascending in row, so every
run's place in the sorted order is known by construction (chunk = RT = 16
entries).  In order: row 0 with 21 entries (the next run starts mid-chunk);
row 1 heavy with 194 entries over 13 chunks (an 11-entry head partial, 11
full chunks, a 7-entry tail partial); a run of exactly 16 that fills one
chunk between different neighbours; a run of 17 from a chunk edge; a run of
2 across an edge; runs of thr and thr + 1 chunk-aligned, then both again
unaligned; an aligned run of 48; a heavy run of 93 that ends exactly on a
chunk edge; two singletons; a seeded multinomial filler over rows
20 .. rows - 3; row rows - 2 untouched; row rows - 1 with the last 3 entries.
M = 1003 gives N % 16 = 6 (N = 2M) and 11 (N = M); M = 1008 gives N % 16 = 0
for both.  The tables have 1001 and 777 rows, neither a multiple of 64.
Entries go alternately to the ``starts`` and the ``ends`` half, so both feed
every planted run, and each half is shuffled.

gout is +-[0.5, 2) (a lost entry costs at least 0.5) or, in the "int" case,
integers in [-4, 4]; the columns past 2 TS + PS are NaN (never read).  The
segment a PAD entry reads is zero, as in training, except in the "padnz"
case.  Widths (TS, PS) are (8, 8), (104, 40), (136, 104); KP = round_up(2 TS +
PS, 32).

Adam state: random p, m, v >= 0, with planted elements at both ends of the
tensor (the tail ones reach the scalar tail): g = 0 with m = v = 0 (an exact
no-op at wd = 0); p = 0; |g| = 1e-9 with m = v = 0 (eps dominates the
denominator); |g| = 1024.  bc_pow is set by hand to t in {1, 2, 1000}.
"""

from __future__ import annotations

import numpy as np
import torch

from head_numerics import E24, U, assert_within, d, violations  # noqa: F401
from head_numerics import E23  # noqa: F401  (re-exported with the rule)

RT = 16
SECOND = 1.0 + 2.0 ** -20
WIDTHS = ((8, 8), (104, 40), (136, 104))
THRS = (32, 64)
M_OF = {"odd": 1003, "even": 1008}
T_ROWS, P_ROWS = 1001, 777
M_OPS, V_OPS, V_OPS_SCALAR, P_OPS = 4, 6, 7, 8
bf16 = torch.bfloat16


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ---------------------------------------------------------------------------
# worst ratios, for the README table


WORST = {}


def within(got, ref, tol, name: str, where: str) -> float:
    """assert_within that also keeps the worst ratio per output name."""
    r = assert_within(got, ref, tol, f"{name} {where}")
    if r >= WORST.get(name, (-1.0, ""))[0]:
        WORST[name] = (r, where)
    return r


def print_worst(title: str) -> None:
    for name in sorted(WORST):
        r, where = WORST[name]
        print(f"optimizer_numerics {title} worst | {name} | {r:.3f} | {where}")


# ---------------------------------------------------------------------------
# planted runs


def run_plan(thr: int, total: int, rows: int, seed: int = 0):
    """((row, count) ascending in row, {feature: row}) with ``total``
    entries over a table of ``rows`` rows (see the module docstring)."""
    named = dict(pad=0, heavy=1, fill16=3, r17=4, straddle=6, thr_al=8,
                 thr1_al=9, thr_un=11, thr1_un=12, r48=14, heavy_edge=16,
                 single_a=17, single_b=19, untouched=rows - 2, last=rows - 1)
    prefix = [(0, 21), (1, 194), (2, 9), (3, 16), (4, 17), (5, 14), (6, 2),
              (7, 15), (8, thr), (9, thr + 1), (10, 4), (11, thr),
              (12, thr + 1), (13, 10), (14, 48), (15, 3), (16, 93), (17, 1),
              (19, 1)]
    used = sum(c for _, c in prefix) + 3
    rest = total - used
    assert rest > 0 and rows > 64
    rng = np.random.default_rng(1000 * thr + total + seed)
    fill = rng.multinomial(rest, np.full(rows - 22, 1.0 / (rows - 22)))
    plan = prefix + [(20 + i, int(c)) for i, c in enumerate(fill) if c > 0]
    plan.append((rows - 1, 3))
    assert sum(c for _, c in plan) == total
    return plan, named


def plan_positions(plan):
    """{row: (first, last)} positions of each run in the sorted order."""
    pos, out = 0, {}
    for r, c in plan:
        out[r] = (pos, pos + c - 1)
        pos += c
    return out


def chunk_span(plan, rows: int) -> torch.Tensor:
    """[rows] number of RT-entry chunks each row's run touches (0 if none)."""
    span = torch.zeros(rows, dtype=torch.int64)
    for r, (a, b) in plan_positions(plan).items():
        span[r] = b // RT - a // RT + 1
    return span


class Table:
    """One table's view of a ScatterCase: the index list (N = 2M start|end
    with two offsets, or N = M), its plan and the fp64 reference."""

    def __init__(self, tag, idx, plan, named, rows, S, off0, off1, M):
        self.tag, self.idx, self.plan, self.named = tag, idx, plan, named
        self.rows, self.S, self.off0, self.off1, self.M = rows, S, off0, off1, M
        self.N = idx.numel()
        self.span = chunk_span(plan, rows)
        self.fixed_order = self.span <= 2  # at most two partials: a + b
        self.ref = None


class ScatterCase:
    """Seeded index lists and gout of one (plan, thr, widths, grad) case."""

    def __init__(self, plan: str, thr: int, TS: int, PS: int,
                 grad: str = "real"):
        M = M_OF[plan]
        g = torch.Generator().manual_seed(7919 * M + 31 * thr + TS + PS)
        self.plan, self.thr, self.TS, self.PS, self.grad = plan, thr, TS, PS, grad
        self.M, self.T, self.P = M, T_ROWS, P_ROWS
        self.KP = KP = round_up(2 * TS + PS, 32)
        tplan, tnamed = run_plan(thr, 2 * M, T_ROWS)
        pplan, pnamed = run_plan(thr, M, P_ROWS)
        tsorted = torch.tensor([r for r, c in tplan for _ in range(c)],
                               dtype=torch.int32)
        psorted = torch.tensor([r for r, c in pplan for _ in range(c)],
                               dtype=torch.int32)
        half_a, half_b = tsorted[0::2], tsorted[1::2]
        self.starts = half_a[torch.randperm(M, generator=g)].contiguous()
        self.ends = half_b[torch.randperm(M, generator=g)].contiguous()
        self.paths = psorted[torch.randperm(M, generator=g)].contiguous()
        if grad == "int":
            gout = torch.randint(-4, 5, (M, KP), generator=g).float()
        else:
            mag = 0.5 + 1.5 * torch.rand(M, KP, generator=g)
            sign = torch.randint(0, 2, (M, KP), generator=g).float() * 2 - 1
            gout = mag * sign
        gout[:, 2 * TS + PS:] = float("nan")
        if grad != "padnz":
            gout[:, :TS][self.starts == 0] = 0
            gout[:, TS:TS + PS][self.paths == 0] = 0
            gout[:, TS + PS:2 * TS + PS][self.ends == 0] = 0
        self.gout = gout.to(bf16)
        self.tables = {
            "term": Table("term", torch.cat([self.starts, self.ends]), tplan,
                          tnamed, T_ROWS, TS, 0, TS + PS, M),
            "path": Table("path", self.paths, pplan, pnamed, P_ROWS, PS, TS,
                          TS, M)}

    def name(self) -> str:
        return (f"{self.plan} thr={self.thr} ({self.TS},{self.PS}) "
                f"{self.grad}")


_CASES = {}


def scatter_case(plan, thr, TS, PS, grad="real") -> ScatterCase:
    """One ScatterCase per key, built once and shared read-only."""
    key = (plan, thr, TS, PS, grad)
    if key not in _CASES:
        _CASES[key] = ScatterCase(*key)
    return _CASES[key]


def all_scatter_keys():
    keys = [(p, t, ts, ps, "real") for p in M_OF for t in THRS
            for ts, ps in WIDTHS]
    return keys + [("odd", 64, 104, 40, "int"), ("odd", 32, 136, 104, "padnz"),
                   ("even", 64, 8, 8, "padnz")]


# ---------------------------------------------------------------------------
# table gradient: fp64 reference and bound


def entry_segments(tb: Table, gout, ends_off=None) -> torch.Tensor:
    """[N, S] the gout segment each entry of the index list reads."""
    g = gout if gout.dtype == torch.float64 else d(gout)
    a = g[:, tb.off0:tb.off0 + tb.S]
    if tb.N == tb.M:
        return a
    o1 = tb.off1 if ends_off is None else ends_off
    return torch.cat([a, g[:, o1:o1 + tb.S]])


def _sorted_order(tb: Table):
    order = torch.argsort(tb.idx.long(), stable=True)
    return order, tb.idx.long()[order]


def table_grad_ref(tb: Table, gout, mutate: str = None):
    """(g64, mag, n_r) of one table.  ``mutate`` names one of the plausible
    kernel bugs of the CPU tests."""
    seg = entry_segments(tb, gout,
                         ends_off=tb.off0 if mutate == "ends_at_off0" else None)
    order, sidx = _sorted_order(tb)
    keep = torch.ones(tb.N, dtype=torch.bool)
    pos = plan_positions(tb.plan)
    nm = tb.named
    if mutate == "drop_first":
        keep[pos[nm["heavy"]][0]] = False
    elif mutate == "drop_last":
        keep[pos[nm["r17"]][1]] = False
    elif mutate == "drop_edge":
        keep[round_up(pos[nm["heavy"]][0], RT)] = False
    elif mutate == "drop_chunk":
        c0 = round_up(pos[nm["heavy"]][0], RT) + RT
        keep[c0:c0 + RT] = False
    elif mutate == "drop_head":
        a = pos[nm["heavy"]][0]
        keep[a:round_up(a, RT)] = False
    elif mutate == "drop_tail":
        b = pos[nm["heavy"]][1]
        keep[b // RT * RT:b + 1] = False
    elif mutate == "drop_last_row":
        a, b = pos[nm["last"]]
        keep[a:b + 1] = False
    elif mutate == "drop_tail_entries":
        assert tb.N % RT
        keep[tb.N // RT * RT:] = False
    seg = seg[order]
    if mutate == "drop_cols128":
        assert tb.S > 128
        seg = seg.clone()
        seg[:, 128:] = 0
    seg = seg * keep[:, None].double()
    ref = torch.zeros(tb.rows, tb.S, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    ref.index_add_(0, sidx, seg)
    mag.index_add_(0, sidx, seg.abs())
    n_r = torch.bincount(sidx, minlength=tb.rows)
    if mutate != "pad_summed":
        ref[0] = 0
        mag[0] = 0
    assert int(n_r[1:].max()) <= 512
    return ref, mag, n_r


def table_grad_tol(ref, mag, n_r):
    return (U * ref.abs() + (n_r[:, None].double() + 2) * E24 * mag) * SECOND


def table_ref(case: ScatterCase, tag: str):
    """Cached (ref, tol, mag, n_r) of one table of a case."""
    tb = case.tables[tag]
    if tb.ref is None:
        ref, mag, n_r = table_grad_ref(tb, case.gout)
        tb.ref = (ref, table_grad_tol(ref, mag, n_r), mag, n_r)
    return tb.ref


def gather_concat_ref(starts, paths, ends, term, path, KP):
    """bf16 [M, KP] = [term[starts] | path[paths] | term[ends] | 0]."""
    M = starts.numel()
    out = torch.zeros(M, KP, dtype=bf16)
    TS, PS = term.shape[1], path.shape[1]
    out[:, :TS] = term[starts.long()]
    out[:, TS:TS + PS] = path[paths.long()]
    out[:, TS + PS:2 * TS + PS] = term[ends.long()]
    return out


# ---------------------------------------------------------------------------
# Adam: hyper-parameters, planted state, fp64 reference and bounds


def f32r(x: float) -> float:
    return float(np.float32(x))


class Hyper:
    """``args`` are the Python floats handed to the bindings; the attributes
    are what the kernels compute with (the bindings cast to float)."""

    def __init__(self, lr=0.01, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
        self.args = (lr, b1, b2, eps, wd)
        self.lr, self.b1, self.b2, self.eps, self.wd = map(f32r, self.args)
        self.omb1 = float(np.float32(1.0) - np.float32(b1))
        self.omb2 = float(np.float32(1.0) - np.float32(b2))

    def pow_at(self, t: int):
        """(b1f^t, b2f^t) as adam_tick leaves them after t ticks."""
        return (self.b1 ** t, self.b2 ** t)


def adam_state(n: int, grad_dtype, seed: int = 0):
    """dict(p fp32 (the master for bf16 parameters), g, m, v) with the
    planted elements of the module docstring."""
    gen = torch.Generator().manual_seed(104729 * (seed + 1) + n)
    p = torch.randn(n, generator=gen) * 0.1
    g = torch.randn(n, generator=gen) * 0.01
    m = torch.randn(n, generator=gen) * 0.01
    v = torch.rand(n, generator=gen) * 1e-4

    def plant(i, kind, sign):
        if kind == 0:
            g[i] = 0; m[i] = 0; v[i] = 0
        elif kind == 1:
            p[i] = 0
        elif kind == 2:
            g[i] = sign * 1e-9; m[i] = 0; v[i] = 0
        else:
            g[i] = sign * 1024.0

    for k in range(min(4, n)):
        plant(k, k, 1.0)
    if n >= 8:
        for k in range(4):
            plant(n - 1 - k, 3 - k, -1.0)
    elif n > 4:
        plant(n - 1, 2, -1.0)
    return dict(p=p, g=g.to(grad_dtype), m=m, v=v)


def adam_moments_ref(old, g64, hp: Hyper, mutate: str = None):
    """{'m': (ref, mag), 'v': (ref, mag), 'G': |G| bound pieces} from the
    state before the step and the fp64 gradient."""
    p, m, v = d(old["p"]), d(old["m"]), d(old["v"])
    wd = 0.0 if mutate == "no_wd" else hp.wd
    G = g64 + wd * p
    Gm = g64.abs() + wd * p.abs()
    mref = hp.b1 * m + hp.omb1 * G
    mmag = hp.b1 * m.abs() + hp.omb1 * Gm
    if mutate == "v_from_G":
        vref = hp.b2 * v + hp.omb2 * G
    else:
        vref = hp.b2 * v + hp.omb2 * G * G
    vmag = hp.b2 * v.abs() + hp.omb2 * Gm * Gm
    return dict(m=(mref, mmag), v=(vref, vmag), G=G, Gmag=Gm)


def adam_param_ref(old, m_stored, v_stored, pow12, hp: Hyper,
                   mutate: str = None):
    """(p', tol) from the old parameter and the STORED new moments."""
    p, ms, vs = d(old["p"]), d(m_stored), d(v_stored)
    p1, p2 = pow12
    if mutate == "bc_prev":
        p1, p2 = p1 / hp.b1, p2 / hp.b2
    ibc1, ibc2 = 1.0 / (1.0 - p1), 1.0 / (1.0 - p2)
    if mutate == "bc_swap":
        ibc1, ibc2 = ibc2, ibc1
    if mutate == "eps_in_sqrt":
        den = torch.sqrt(vs * ibc2 + hp.eps)
    else:
        den = torch.sqrt(vs * ibc2) + hp.eps
    upd = hp.lr * (ms * ibc1) / den
    ref = p - upd
    return ref, (E24 * ref.abs() + P_OPS * E24 * upd.abs()) * SECOND


def adam_check(where: str, old, new, g64, pow12, hp: Hyper, kernel: str,
               scalar_from=None, dg=None, mutate: str = None,
               count_only: bool = False):
    """The Adam rule on one step.  ``old``/``new``: dicts of p, m, v (and
    ``param``, the bf16 parameter, in ``new``).  ``scalar_from``: first flat
    index updated by the scalar source (None: none; 0: all).  ``dg``: bound
    on the unstored gradient's error (K16b).  With ``count_only`` returns the
    number of violations instead of asserting."""
    n = g64.numel()
    g64 = g64.reshape(-1)
    r = adam_moments_ref(old, g64, hp, mutate)
    v_ops = torch.full((n,), float(V_OPS), dtype=torch.float64)
    if scalar_from is not None:
        v_ops[scalar_from:] = V_OPS_SCALAR
    mtol = M_OPS * E24 * r["m"][1]
    vtol = v_ops * E24 * r["v"][1]
    if dg is not None:
        dg = dg.reshape(-1)
        mtol = mtol + hp.omb1 * dg
        vtol = vtol + hp.omb2 * (2 * r["G"].abs() * dg + dg * dg)
    mtol, vtol = mtol * SECOND, vtol * SECOND
    mref, vref = r["m"][0], r["v"][0]
    if mutate == "tail_skipped" and n % 4:
        k = n - n % 4
        mref, vref = mref.clone(), vref.clone()
        mref[k:], vref[k:] = d(old["m"])[k:], d(old["v"])[k:]
    pref, ptol = adam_param_ref(old, new["m"], new["v"], pow12, hp, mutate)
    if mutate == "tail_skipped" and n % 4:
        pref = pref.clone()
        pref[k:] = d(old["p"])[k:]
    checks = [(f"{kernel} m", new["m"], mref, mtol),
              (f"{kernel} v", new["v"], vref, vtol),
              (f"{kernel} p", new["p"], pref, ptol)]
    if count_only:
        bad = sum(int(violations(got.reshape(-1), ref, tol).sum())
                  for _, got, ref, tol in checks)
        if "param" in new and not param_bits_ok(new["param"], new["p"]):
            bad += 1
        return bad
    for name, got, ref, tol in checks:
        within(got.reshape(-1), ref, tol, name, where)
    if "param" in new:
        assert param_bits_ok(new["param"], new["p"]), \
            f"{kernel} {where}: bf16 parameter is not bf16(master')"
    return 0


def param_bits_ok(param, master) -> bool:
    """The bf16 parameter is one round-to-nearest-even of the stored master."""
    want = master.detach().cpu().reshape(-1).to(bf16)
    return torch.equal(param.detach().cpu().reshape(-1).view(torch.int16),
                       want.view(torch.int16))


def multi_concat(states, shift_state: bool = False):
    """Concatenate per-tensor state dicts into one flat dict.  With
    ``shift_state`` (the CPU tests' mutation: prefix offsets off by one) the
    first element of every tensor but the first takes the moments of the
    element before it."""
    out = {k: torch.cat([s[k].reshape(-1) for s in states])
           for k in states[0]}
    if shift_state:
        off = 0
        for s in states[:-1]:
            off += s["p"].numel()
            for k in ("m", "v"):
                out[k] = out[k].clone()
                out[k][off] = out[k][off - 1]
    return out


# ---------------------------------------------------------------------------
# torch fp32 emulations with the kernels' rounding points (CPU tests)


def emu_scatter(tb: Table, gout, order: str = "ascending", seed: int = 0):
    """bf16 [rows, S]: 16-entry chunk partials from +0 over the sorted
    order, combined per row in the given order, one rounding to bf16."""
    seg = entry_segments(tb, gout.float().double()).float()
    srt, sidx = _sorted_order(tb)
    seg = seg[srt]
    partials = {}
    for k in range(tb.N):
        key = (int(sidx[k]), k // RT)
        acc = partials.get(key)
        partials[key] = seg[k].clone() if acc is None else acc + seg[k]
    rows = {}
    for (r, c), part in partials.items():
        rows.setdefault(r, []).append((c, part))
    out = torch.zeros(tb.rows, tb.S, dtype=torch.float32)
    rng = np.random.default_rng(seed)
    for r, parts in rows.items():
        if r == 0:
            continue
        parts = [p for _, p in sorted(parts, key=lambda cp: cp[0])]
        if order == "reverse":
            parts = parts[::-1]
        elif order == "random":
            parts = [parts[i] for i in rng.permutation(len(parts))]
        tot = torch.zeros(tb.S, dtype=torch.float32)
        for part in parts:
            tot = tot + part
        out[r] = tot
    return out.to(bf16)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emu_adam(old, g, pow12, hp: Hyper, lane: str):
    """One Adam step in fp32, operation by operation.  lane 'fma' and
    'nofma' are adam_update4's elements 0-1 and 2-3; 'scalar' is the scalar
    source with every operation rounded on its own."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    lr, b1, b2, eps, wd = map(f, (hp.lr, hp.b1, hp.b2, hp.eps, hp.wd))
    omb1, omb2 = f(1.0) - b1, f(1.0) - b2
    ibc1 = f(1.0 / (1.0 - pow12[0]))
    ibc2 = f(1.0 / (1.0 - pow12[1]))
    p, m, v, g = old["p"], old["m"], old["v"], g.float()
    if lane == "scalar":
        grad = g + wd * p
        m2 = b1 * m + omb1 * grad
        v2 = b2 * v + (omb2 * grad) * grad
    else:
        grad = _fma(wd, p, g)
        gm = omb1 * grad
        gv = (omb2 * grad) * grad
        if lane == "fma":
            m2, v2 = _fma(b1, m, gm), _fma(b2, v, gv)
        else:
            m2, v2 = b1 * m + gm, b2 * v + gv
    p2 = p - (lr * (m2 * ibc1)) / (torch.sqrt(v2 * ibc2) + eps)
    return dict(p=p2, m=m2, v=v2, param=p2.to(bf16))
