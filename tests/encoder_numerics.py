"""Elementwise fp64 tolerance rule for the encoder kernels (K3-K9, K14, K15).

Not a test file: the fp64 references, the bounds and the planted data of
test_encoder_numerics_cpu.py and test_encoder_numerics_gpu.py.  The rule
itself (``assert_within``: every element satisfies |got - ref64| <= tol64)
and the constants U = 2^-8, E23 = 2^-23, E24 = 2^-24 are those of
head_numerics.py; nothing of it is copied here.

Every reference is fp64 arithmetic on the tensors the kernel was given (bf16
values as stored, upcast) and every backward reference starts from what the
forward stored (z, mean, rstd, out, attn), so each kernel is judged on its
own operation.  ``mag`` is the reference expression with every factor
replaced by its absolute value (a difference a - b becomes |a| + |b|).  The
constants are chain lengths read from the kernels; none is fitted.

combiner_fwd (combiner.hip), per row, E valid of EP columns, K = KP:
  z = bf16(x W^T)        U|ref| + dz,  dz = (KP+2) 2^-23 mag   (one 2^-23 per
                         MFMA k-element, as for the head's logits); columns
                         E..EP exactly 0
  mean (fp32)            dmean = mean_e(dz) + (E+2) 2^-24 mean_e(|z| + dz)
                         (E-term fp32 sum in any order, 1/E, the product)
  var, one pass          dvar = mean_e(2|z| dz + dz^2)          accumulators
    max(s2/E - mean^2,0)        + (E+2) 2^-24 Q                 squares, sum
                                + 2|mean| dmean + dmean^2       mean^2
                                + 2 2^-24 (Q + (|mean|+dmean)^2)
                         with Q = mean_e((|z| + dz)^2): the last term is the
                         cancellation of the one-pass form, relative to
                         var + eps it is (mean^2 + mean(z^2)) / (var + eps);
                         the clamp at 0 only moves towards the true var >= 0
  rstd (fp32)            rsqrt(max(var - dvar, 0) + eps) - rstd  (rsqrt is
                         convex and decreasing: the exact worst case, no
                         linearisation) + 2^-22 of that value (eps + var
                         rounding, a 1-ulp rsqrtf)
                         References: fp64 LayerNorm statistics of the
                         UNROUNDED fp64 x W^T.
  u = xh gamma + beta    du = |gamma| ((dz + dmean)(rstd + drstd)
                              + |z - mean| drstd)
                              + 4 2^-24 (|xh gamma| + |beta|)   (sub, two
                         products, the add)
  out = bf16(drop(tanh)) U|ref| + inv1mp (du + 8 2^-23): tanh is 1-Lipschitz;
                         fast_tanh = 1 - 2/(e^{2|u|} + 1) with a 1-ulp v_exp
                         whose argument product is rounded (relative
                         (1 + |u|) 2^-23 on e, at most 0.73 2^-23 on the
                         quotient), the add (0.5), a 2.5-ulp fast division
                         and the final subtraction (0.5): 4.5 2^-23 < 8 2^-23
                         absolute.  Dropped elements and pad columns exactly
                         0; the mask is read from ``out != 0``.
  raw scores (fp32)      (EP+16) 2^-24 mag: dot of the STORED bf16 out row
                         with a over round8(E) columns.

combiner_bwd, v1/v2/recompute, from the stored dout, z, out, mean, rstd:
  y = out (1-p), d = dy (1 - y^2) where out != 0 (dy = dout/(1-p)),
  h = d gamma, s1 = sum h / E, s2 = sum h xh / E, dz = rstd (h - s1 - xh s2)
  dz (bf16)              U|ref| + (E+16) 2^-24 mag   (the E-long reductions
                         plus about ten elementwise roundings)
  dgamma/dbeta           (M+8) 2^-24 mag, partials [blocks, EP] and sums;
                         a partial holds the rows its block's grid-stride
                         loop visits (block_of_row), so a v1/v2 mix-up or a
                         lost grid-stride tail is flagged
  recompute MODE 1/2     dout = bf16(attn dcv + ds a) is rebuilt in fp64 and
                         rounded to bf16.  The kernel rounds an fp32 value
                         that differs from the fp64 one by up to
                         dv = 2 2^-24 (|attn dcv| + |ds a|) (+ tol(ds)|a|
                         where ds came from a kernel), so where
                         bf16(v - dv) != bf16(v + dv) the two roundings may
                         legitimately differ by that one bf16 step; the step
                         is propagated through the (linear in dout) mag
                         expressions and added.  This is the reference's own
                         uncertainty, nothing else is widened.

attention (attention.hip), scores s_c = ccv_c . a over round8(E) columns,
masked exactly as the kernel does: s mask + (1 - mask) NINF, NINF = -3.4e38,
so all-pad rows are uniform 1/C and pads of mixed rows exactly 0:
  ds_c = (EP+16) 2^-24 mag_c  on valid contexts
  attn (fp32)            attn (ds_c + sum_c attn_c ds_c + (C+8) 2^-24 + 2^-20):
                         first-order softmax sensitivity (the own score,
                         and the normaliser, whose share of "2 ds" is the
                         attn-weighted mean of ds, at most the row maximum),
                         the C-term sum, __expf (its argument error
                         |s - max| 2^-24 is below ds), the division.  No
                         absolute floor: the planted scores keep every valid
                         exponential far above fp32's denormals
  cv (fp32)              sum_c tol_attn |ccv| + (C+8) 2^-24 mag
  cvb (bf16)             + U|ref|
  g_c = dcv . ccv_c (+ dattn_c), sg = sum attn g, ds = attn (g - sg) mask
  ds (fp32)              (EP+C+32) 2^-24 attn (mag g_c + sum attn mag g)
  dccv (bf16)            U|ref| + tol_ds |a| + 3 2^-24 (|attn dcv| + |ds a|)
  da partial [B, EP]     sum_c tol_ds |ccv| + (C+8) 2^-24 mag; columns >= E 0
  da                     sum of the partial bounds + (B+8) 2^-24 mag

GEMMs of exact bf16 operands (head_numerics.exact_tol):
  dgrad2 dx              K = EP
  wgrad slab (fp32)      K = rows of the slab, no output rounding; a slab
                         whose row range is empty is exactly 0
  dw after wgrad_reduce  K = M + 256

Planted data.  Dense random operands make a dropped k-step or row an O(1)
error on GEMM outputs; the rest is planted.  CombinerCase: W[:, 0] = 0.25
for every valid column, so x[r, 0] = 32 std_r moves the whole row r of z by
8 of its standard deviations ("offset" rows 1, 126, 129, M-1: the one-pass
variance); rows 2, 127,
128 have x = 0 (z = 0, var = 0, rstd = 1/sqrt(eps)); columns 3 and E-1 have
gamma = 2^-6, beta = 2^-8 (|u| small), columns 5 and E-2 gamma = 6, beta =
+-2 (saturated tanh); every beta is at least 0.05 away from 0 elsewhere so
that no kept element is 0 and the dropout mask can be read from out != 0.
AttentionCase: method 0 full length, 1 all pad, 2 length 1, the others (and
method 0 where B < 3) with pads scattered and position C-1 padded; dominant
contexts (ccv_c = 16 a / |a|^2 + n_c with n_c orthogonal to a: score 16, at
least 10 above the rest, rows that differ so that cv feels each one) at 0,
63, 64 and C-1 of method 0 and at 0, 63, 64 and the last valid position of
the scattered ones.  The dominants of one method share the score, so losing
one of k moves the others by k / (k - 1).
"""

from __future__ import annotations

import math

import numpy as np
import torch

from head_numerics import (E23, E24, U, assert_within, d, exact_tol,  # noqa
                           frobenius, violations)

LN_EPS = 1e-5
NINF = -3.4e38
bf16 = torch.bfloat16


def check(got, ref, tol, output: str, where: str) -> float:
    """assert_within under the tag 'enc <output> | <where>' (the README
    table is collected from these lines)."""
    return assert_within(got, ref, tol, f"enc {output} | {where}")


def round8(E: int) -> int:
    return (E + 7) & ~7


def to_bf16(x64: torch.Tensor) -> torch.Tensor:
    return x64.to(torch.float32).to(bf16)


# ---------------------------------------------------------------------------
# the dropout stream of common.h (rng_uniform), for mask checks


def dropout_uniform(seed: int, offset: int, M: int, EP: int) -> torch.Tensor:
    """u01[row, col] of the kernels' counter RNG at index offset + row*EP +
    col, as fp64 (the values are multiples of 2^-24, exact in fp32)."""
    idx = np.uint64(offset) + np.arange(M * EP, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    h = ((idx ^ (idx >> np.uint64(32))) & m32) * np.uint64(0x9E3779B9) & m32
    s = np.uint64(seed & 0xFFFFFFFFFFFFFFFF)
    sk = (s & m32) ^ (((s >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & m32)
    h = h ^ sk
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x7FEB352D) & m32
    h ^= h >> np.uint64(15)
    h = h * np.uint64(0x846CA68B) & m32
    h ^= h >> np.uint64(16)
    u = (h >> np.uint64(8)).astype(np.float64) / 16777216.0
    return torch.from_numpy(u).reshape(M, EP)


# ---------------------------------------------------------------------------
# planted data

OFFSET_ROWS = (1, 126, 129, -1)
ZERO_ROWS = (2, 127, 128)
OFFSET_STD = 8.0
OFFSET_W = 0.25


class CombinerCase:
    """Seeded inputs of one (M, KP, E, EP) combiner shape, on the CPU: x
    [M, KP] and w [EP, KP] bf16 (pad rows 0), gamma/beta/a [EP] fp32 (pad
    0), dout [M, EP] bf16 (pad columns 0)."""

    def __init__(self, M: int, KP: int, E: int, EP: int):
        g = torch.Generator().manual_seed(7919 * M + 31 * KP + EP + E)
        x = torch.randn(M, KP, generator=g)
        w = torch.zeros(EP, KP)
        w[:E] = torch.randn(E, KP, generator=g) * (0.4 / math.sqrt(KP))
        w[:E, 0] = OFFSET_W
        self.offset_rows = sorted({r % M for r in OFFSET_ROWS if r < M})
        self.zero_rows = sorted({r for r in ZERO_ROWS if r < M}
                                - set(self.offset_rows))
        x[self.zero_rows] = 0.0
        x, w = x.to(bf16), w.to(bf16)
        for r in self.offset_rows:      # a common shift of 8 std of the row
            x[r, 0] = 0.0
            zr = d(x[r]) @ d(w[:E]).t()
            x[r, 0] = OFFSET_STD * float(zr.std(unbiased=False)) / OFFSET_W
        gamma = torch.zeros(EP)
        beta = torch.zeros(EP)
        gamma[:E] = torch.rand(E, generator=g) + 0.5
        sign = torch.where(torch.rand(E, generator=g) < 0.5, -1.0, 1.0)
        beta[:E] = sign * (0.05 + 0.1 * torch.rand(E, generator=g))
        self.small_cols = sorted({3 % E, E - 1})
        self.sat_cols = sorted({5 % E, max(E - 2, 0)} - set(self.small_cols))
        gamma[self.small_cols] = 2.0 ** -6
        beta[self.small_cols] = 2.0 ** -8
        gamma[self.sat_cols] = 6.0
        beta[self.sat_cols] = sign[self.sat_cols] * 2.0
        a = torch.zeros(EP)
        a[:E] = torch.randn(E, generator=g) * 0.2
        dout = torch.zeros(M, EP)
        dout[:, :E] = torch.randn(M, E, generator=g) * 0.1
        self.M, self.KP, self.E, self.EP = M, KP, E, EP
        self.x, self.w = x, w
        self.gamma, self.beta, self.a = gamma, beta, a
        self.dout = dout.to(bf16)


class AttentionCase:
    """Seeded inputs of one (B, C, E, EP) attention shape, on the CPU: ccv
    [B, C, EP] bf16 (pad columns 0), a [EP] fp32, starts [B, C] int32, dcv
    [B, EP] fp32 and its bf16 rounding, dattn [B, C] fp32.  ``dominant``
    maps method -> position of its dominant context."""

    def __init__(self, B: int, C: int, E: int = 100, EP: int = 128):
        g = torch.Generator().manual_seed(104729 * B + 13 * C + EP + E)
        ccv = torch.zeros(B, C, EP)
        ccv[:, :, :E] = torch.tanh(torch.randn(B, C, E, generator=g))
        a = torch.zeros(EP)
        a[:E] = torch.randn(E, generator=g) * 0.2
        starts = torch.randint(1, 100, (B, C), generator=g, dtype=torch.int32)
        scatter = torch.rand(B, C, generator=g) < 0.3
        self.dominant = {}
        spike = 16.0 * a / float(a.double() @ a.double())
        edges = sorted({0, min(63, C - 1), min(64, C - 1)})
        for b in range(B):
            if b == 1:
                starts[b] = 0                       # length 0
                continue
            if b == 2:
                starts[b, 1:] = 0                   # length 1
                continue
            pos = set(edges)
            if b == 0 and B >= 3:                   # length C
                pos.add(C - 1)
            else:                                   # pads scattered
                starts[b][scatter[b]] = 0
                starts[b, C - 1] = 0
                starts[b, edges] = 7
                pos.add(int(torch.nonzero(starts[b] > 0).flatten()[-1]))
            for c in sorted(pos):   # same score, different rows: + n, n _|_ a
                n = torch.zeros(EP)
                n[:E] = torch.randn(E, generator=g) * 0.5
                ccv[b, c] = spike + n - float(n @ a) / float(a @ a) * a
            self.dominant[b] = sorted(pos)
        dcv = torch.zeros(B, EP)
        dcv[:, :E] = torch.randn(B, E, generator=g) * 0.1
        self.B, self.C, self.E, self.EP = B, C, E, EP
        self.ccv, self.a, self.starts = ccv.to(bf16), a, starts
        self.dcv, self.dcv16 = dcv, dcv.to(bf16)
        self.dattn = torch.randn(B, C, generator=g) * 0.1


_CASES = {}


def combiner_case(M, KP, E, EP) -> CombinerCase:
    key = ("c", M, KP, E, EP)
    if key not in _CASES:
        _CASES[key] = CombinerCase(M, KP, E, EP)
    return _CASES[key]


def attention_case(B, C, E=100, EP=128) -> AttentionCase:
    key = ("a", B, C, E, EP)
    if key not in _CASES:
        _CASES[key] = AttentionCase(B, C, E, EP)
    return _CASES[key]


def gemm_case(M: int, K: int, N: int, seed: int = 0):
    """Dense random bf16 operands: a [M, K] and b [M, N] (two matrices that
    share their row dimension), b scaled like a gradient."""
    g = torch.Generator().manual_seed(seed + 65537 * M + 257 * K + N)
    return (torch.randn(M, K, generator=g).to(bf16),
            (torch.randn(M, N, generator=g) * 0.1).to(bf16))


# contexts per method for the recompute modes at the tests' row counts
# (M must be a multiple of C)
RECOMPUTE_C = {5: 5, 129: 43, 300: 100, 8193: 3}


def recompute_inputs(M: int, C: int, EP: int, dcv_bf16: bool):
    """(attn [M], ds [M], dcv [M / C, EP], C) for the dout-recomputing
    combiner backward: softmax rows and a ds of the size attention gives."""
    g = torch.Generator().manual_seed(M + C)
    attn = torch.softmax(torch.randn(M // C, C, generator=g) * 2, dim=1)
    ds = torch.randn(M, generator=g) * 0.05 * attn.flatten()
    dcv = torch.randn(M // C, EP, generator=g) * 0.1
    return attn.flatten(), ds, (dcv.to(bf16) if dcv_bf16 else dcv), C


def gather_tables(KP: int, M: int, seed: int = 0):
    """Embedding tables and indices whose concatenation is an [M, KP] x:
    TS = PS = 8 floor(KP / 24) (2 TS + PS <= KP, the rest of x is 0).
    Returns (starts, paths, ends, term, path, x)."""
    g = torch.Generator().manual_seed(seed + 97 * KP + M)
    TS = PS = 8 * (KP // 24)
    T, P = 37, 29
    term = torch.randn(T, TS, generator=g).to(bf16)
    path = torch.randn(P, PS, generator=g).to(bf16)
    starts = torch.randint(0, T, (M,), generator=g, dtype=torch.int32)
    paths = torch.randint(0, P, (M,), generator=g, dtype=torch.int32)
    ends = torch.randint(0, T, (M,), generator=g, dtype=torch.int32)
    x = torch.zeros(M, KP, dtype=bf16)
    x[:, :TS] = term[starts.long()]
    x[:, TS:TS + PS] = path[paths.long()]
    x[:, TS + PS:2 * TS + PS] = term[ends.long()]
    return starts, paths, ends, term, path, x


# ---------------------------------------------------------------------------
# combiner forward


def combiner_fwd_ref(x, w, gamma, beta, E: int, p: float = 0.0,
                     out_stored=None, mean_over=None, drop_k=None):
    """{'z','mean','rstd','out': (ref, tol)} plus 'u' (fp64) of the fused
    forward.  With p > 0 the keep mask is ``out_stored != 0``.  ``mean_over``
    (divide the row sums by it instead of E) and ``drop_k`` (a 32-wide
    k-step left out of the GEMM) build the CPU tests' mutations."""
    x, w, gamma, beta = d(x), d(w), d(gamma), d(beta)
    if drop_k is not None:
        x = x.clone()
        x[:, 32 * drop_k:32 * drop_k + 32] = 0
    M, KP = x.shape
    EP = w.shape[0]
    zf = x @ w.t()
    mag = x.abs() @ w.abs().t()
    zf[:, E:] = 0
    mag[:, E:] = 0
    dz = (KP + 2) * E23 * mag
    zE, dzE = zf[:, :E], dz[:, :E]
    div = E if mean_over is None else mean_over
    mean = zE.sum(dim=1) / div
    dmean = dzE.mean(dim=1) + (E + 2) * E24 * (zE.abs() + dzE).mean(dim=1)
    var = (zE * zE).sum(dim=1) / div - mean * mean
    if mean_over is None:
        var = ((zE - mean[:, None]) ** 2).mean(dim=1)
    Q = ((zE.abs() + dzE) ** 2).mean(dim=1)
    dvar = ((2 * zE.abs() * dzE + dzE * dzE).mean(dim=1)
            + (E + 2) * E24 * Q + 2 * mean.abs() * dmean + dmean * dmean
            + 2 * E24 * (Q + (mean.abs() + dmean) ** 2))
    rstd = (var + LN_EPS) ** -0.5
    hi = ((var - dvar).clamp_min(0.0) + LN_EPS) ** -0.5
    drstd = (hi - rstd) + 2.0 ** -22 * hi
    gm, bt = gamma[:E], beta[:E]
    cen = zE - mean[:, None]
    xh = cen * rstd[:, None]
    u = xh * gm + bt
    du = (gm.abs() * ((dzE + dmean[:, None]) * (rstd + drstd)[:, None]
                      + cen.abs() * drstd[:, None])
          + 4 * E24 * ((xh * gm).abs() + bt.abs()))
    inv = 1.0 / (1.0 - float(np.float32(p))) if p > 0 else 1.0
    keep = torch.ones(M, E, dtype=torch.float64)
    if p > 0:
        keep = (d(out_stored)[:, :E] != 0).double()
    out = torch.zeros(M, EP, dtype=torch.float64)
    otol = torch.zeros(M, EP, dtype=torch.float64)
    out[:, :E] = torch.tanh(u) * inv * keep
    otol[:, :E] = (U * out[:, :E].abs() + inv * (du + 8 * E23)) * keep
    return {"z": (zf, U * zf.abs() + dz), "mean": (mean, dmean),
            "rstd": (rstd, drstd), "out": (out, otol), "u": u}


def scores_ref(out_stored, a, E: int):
    """(ref, tol) of the raw scores: stored bf16 out row . a."""
    o, a = d(out_stored), d(a)
    EP = o.shape[-1]
    ts = min(round8(E), EP)
    ref = o[..., :ts] @ a[:ts]
    mag = o[..., :ts].abs() @ a[:ts].abs()
    return ref, (EP + 16) * E24 * mag


# ---------------------------------------------------------------------------
# combiner backward

BWD_MAX_GRID = 1024


def block_of_row(M: int, rows_per_wave: int) -> torch.Tensor:
    """Block whose dgamma/dbeta partial row accumulates each of the M rows:
    grid = min(ceil(M/4), 1024) blocks of 4 waves; a wave visits row (v1,
    rows_per_wave = 1) or row pair (v2 and the recompute modes, 2) number
    block*4 + wave + k*grid*4."""
    grid = min((M + 3) // 4, BWD_MAX_GRID)
    unit = torch.arange(M) // rows_per_wave
    return (unit % (grid * 4)) // 4


def dout_recompute_ref(attn, ds, dcv, a, C: int, ds_tol=None, dsa=True):
    """(dout, ddout): bf16(attn dcv + ds a) rebuilt in fp64 and rounded to
    bf16, and the bf16 step by which the kernel's rounding of its fp32
    value may differ (0 almost everywhere).  ``dsa=False`` deletes the ds a
    term (a mutation)."""
    attn, ds, dcv, a = d(attn).flatten(), d(ds).flatten(), d(dcv), d(a)
    M = attn.numel()
    rows = torch.arange(M) // C
    t1 = attn[:, None] * dcv[rows]
    t2 = ds[:, None] * a[None, :] if dsa else torch.zeros_like(t1)
    v = t1 + t2
    dv = 2 * E24 * (t1.abs() + t2.abs())
    if ds_tol is not None:
        dv = dv + d(ds_tol).flatten()[:, None] * a.abs()[None, :]
    lo, hi = d(to_bf16(v - dv)), d(to_bf16(v + dv))
    return d(to_bf16(v)), hi - lo


def combiner_bwd_ref(dout, z, out, mean, rstd, gamma, E: int, p: float,
                     ddout=None, tanh_deriv=True, scale=True):
    """dz (ref, tol) and the per-row dgamma/dbeta terms with their mags:
    {'dz': (ref, tol), 'dg': (rows, mag, extra), 'db': (rows, mag, extra)}.
    ``extra`` is the propagated ``ddout`` (see dout_recompute_ref), already
    inside dz's tol.  ``tanh_deriv=False`` (derivative 1) and
    ``scale=False`` (dropout scale missing) are the CPU tests' mutations."""
    dout, z, out = d(dout), d(z), d(out)
    mu, rs, g = d(mean)[:, None], d(rstd)[:, None], d(gamma)[None, :]
    M, EP = z.shape
    p32 = float(np.float32(p))
    inv = 1.0 / (1.0 - p32) if (p > 0 and scale) else 1.0
    valid = (torch.arange(EP) < E)[None, :].double()
    kept = (out != 0).double() * valid
    xh = (z - mu) * rs
    xh_mag = (z.abs() + mu.abs()) * rs
    y = out * (1.0 - p32)
    t = 1.0 - y * y if tanh_deriv else torch.ones_like(y)
    t_mag = 1.0 + y * y

    def chain(dy_abs):
        """mag of (dz, dg, db) for per-element |dy| = dy_abs."""
        dm = dy_abs * t_mag
        hm = dm * g.abs()
        s1m = hm.sum(dim=1, keepdim=True) / E
        s2m = (hm * xh_mag).sum(dim=1, keepdim=True) / E
        return rs * (hm + s1m + xh_mag * s2m) * valid, dm * xh_mag, dm

    dy = dout * inv * kept
    dd = dy * t
    h = dd * g
    s1 = h.sum(dim=1, keepdim=True) / E
    s2 = (h * xh).sum(dim=1, keepdim=True) / E
    dz = rs * (h - s1 - xh * s2) * valid
    zmag, gmag, bmag = chain(dy.abs())
    tol = U * dz.abs() + (E + 16) * E24 * zmag
    zero = torch.zeros_like(dz)
    gext = bext = zero
    if ddout is not None:
        zext, gext, bext = chain(d(ddout) * inv * kept)
        tol = tol + zext
    return {"dz": (dz, tol), "dg": (dd * xh, gmag, gext),
            "db": (dd, bmag, bext)}


def bwd_partials_ref(rows, mag, extra, M: int, rows_per_wave: int,
                     drop_past_grid=False):
    """{'part': (ref, tol) [blocks, EP], 'sum': (ref, tol) [EP]} of a
    dgamma/dbeta reduction.  ``drop_past_grid`` leaves out the rows that the
    first pass of the grid does not cover (a mutation)."""
    grid = min((M + 3) // 4, BWD_MAX_GRID)
    blk = block_of_row(M, rows_per_wave)
    if drop_past_grid:
        rows = rows.clone()
        rows[grid * 4 * rows_per_wave:] = 0
    EP = rows.shape[1]
    part = torch.zeros(grid, EP, dtype=torch.float64).index_add_(0, blk, rows)
    pmag = torch.zeros_like(part).index_add_(0, blk, mag)
    pext = torch.zeros_like(part).index_add_(0, blk, extra)
    k = (M + 8) * E24
    return {"part": (part, k * pmag + pext),
            "sum": (rows.sum(dim=0), k * mag.sum(dim=0) + extra.sum(dim=0))}


# ---------------------------------------------------------------------------
# attention


def attention_fwd_ref(ccv, a, starts, E: int, use_mask=True, raw=None):
    """{'scores','attn','cv','cvb': (ref, tol)} of the attention pool over
    the stored ccv.  ``raw`` (fp32 raw scores from combiner_fwd_scores)
    replaces the reference's own scores and their bound: the streaming
    forward is then judged on mask, softmax and pool alone, its input
    scores having been judged by scores_ref.  ``use_mask=False`` is a
    mutation."""
    c, a = d(ccv), d(a)
    B, C, EP = c.shape
    ts = min(round8(E), EP)
    s = c[..., :ts] @ a[:ts]
    smag = c[..., :ts].abs() @ a[:ts].abs()
    mask = (starts.cpu() > 0).double()
    if not use_mask:
        mask = torch.ones_like(mask)
    raw_ref = (s, (EP + 16) * E24 * smag)
    ds = raw_ref[1] * mask
    if raw is not None:
        s, ds = d(raw).reshape(B, C), torch.zeros_like(ds)
    sm = s * mask + (1.0 - mask) * NINF
    attn = torch.softmax(sm, dim=1)
    atol = attn * (ds + (attn * ds).sum(dim=1, keepdim=True)
                   + (C + 8) * E24 + 2.0 ** -20)
    cv = torch.einsum("bc,bce->be", attn, c)
    cvtol = (torch.einsum("bc,bce->be", atol, c.abs())
             + (C + 8) * E24 * torch.einsum("bc,bce->be", attn, c.abs()))
    cv[:, ts:] = 0
    cvtol[:, ts:] = 0
    return {"scores": raw_ref, "attn": (attn, atol), "cv": (cv, cvtol),
            "cvb": (cv, cvtol + U * cv.abs())}


def attention_bwd_ref(dcv, dattn, ccv, a, starts, attn, E: int,
                      center=True, dsa=True, use_mask=True):
    """{'ds','dccv','da_part','da': (ref, tol)} from the stored attn.
    ``dattn`` may be None.  ``center=False`` deletes - sum attn g,
    ``dsa=False`` the ds a term of dccv, ``use_mask=False`` ignores the
    mask (mutations)."""
    dcv, c, a, at = d(dcv), d(ccv), d(a), d(attn)
    B, C, EP = c.shape
    at = at.reshape(B, C)
    ts = min(round8(E), EP)
    mask = (starts.cpu() > 0).double()
    if not use_mask:
        mask = torch.ones_like(mask)
    g = torch.einsum("bce,be->bc", c[..., :ts], dcv[:, :ts])
    gmag = torch.einsum("bce,be->bc", c[..., :ts].abs(), dcv[:, :ts].abs())
    if dattn is not None:
        g = g + d(dattn)
        gmag = gmag + d(dattn).abs()
    sg = (at * g).sum(dim=1, keepdim=True) if center else 0.0
    ds = at * (g - sg) * mask
    dsmag = at * (gmag + (at * gmag).sum(dim=1, keepdim=True)) * mask
    dstol = (EP + C + 32) * E24 * dsmag
    t1 = at[:, :, None] * dcv[:, None, :]
    t2 = ds[:, :, None] * a[None, None, :]
    if not dsa:
        t2 = torch.zeros_like(t2)
    dccv = t1 + t2
    dctol = (U * dccv.abs() + dstol[:, :, None] * a.abs()[None, None, :]
             + 3 * E24 * (t1.abs() + t2.abs()))
    dccv[..., ts:] = 0
    dctol[..., ts:] = 0
    valid = (torch.arange(EP) < E).double()
    dap = torch.einsum("bc,bce->be", ds, c) * valid
    dapmag = torch.einsum("bc,bce->be", ds.abs(), c.abs()) * valid
    daptol = (torch.einsum("bc,bce->be", dstol, c.abs()) * valid
              + (C + 8) * E24 * dapmag)
    da = dap.sum(dim=0)
    datol = daptol.sum(dim=0) + (B + 8) * E24 * dapmag.sum(dim=0)
    return {"ds": (ds, dstol), "dccv": (dccv, dctol),
            "da_part": (dap, daptol), "da": (da, datol)}


# ---------------------------------------------------------------------------
# the GEMMs of the combiner backward

WGRAD_SLABS = 256


def dgrad_ref(dz, w):
    """(ref, tol) of dx = dz @ w, w [EP, KP]."""
    dz, w = d(dz), d(w)
    ref, mag = dz @ w, dz.abs() @ w.abs()
    return ref, exact_tol(ref, mag, K=w.shape[0])


def wgrad_rows_per_block(M: int, nblocks: int = WGRAD_SLABS) -> int:
    return ((M + nblocks - 1) // nblocks + 31) // 32 * 32


def wgrad_ref(x, dz, nblocks: int = WGRAD_SLABS, drop_row=None):
    """{'slabs': (ref, tol) [S, KP, EP] fp32, 'dw': (ref, tol) [EP, KP]
    bf16} of the split-K weight gradient x^T dz.  An empty slab has ref = tol
    = 0.  ``drop_row`` leaves one row of x out (a mutation)."""
    x, dz = d(x), d(dz)
    if drop_row is not None:
        x = x.clone()
        x[drop_row] = 0
    M, KP = x.shape
    EP = dz.shape[1]
    rpb = wgrad_rows_per_block(M, nblocks)
    xp = torch.zeros(nblocks * rpb, KP, dtype=torch.float64)
    zp = torch.zeros(nblocks * rpb, EP, dtype=torch.float64)
    xp[:M], zp[:M] = x, dz
    xs = xp.view(nblocks, rpb, KP).transpose(1, 2)
    zs = zp.view(nblocks, rpb, EP)
    slabs = xs @ zs
    smag = xs.abs() @ zs.abs()
    rows = (M - torch.arange(nblocks) * rpb).clamp(0, rpb).double()
    stol = rows[:, None, None] * E23 * smag
    dw = slabs.sum(dim=0).t()
    dwmag = smag.sum(dim=0).t()
    return {"slabs": (slabs, stol),
            "dw": (dw, exact_tol(dw, dwmag, K=M + 256)), "rows": rows}
