"""Elementwise fp64 tolerance rule for the output head, the loss and K11.

Not a test file: the shared rule, the fp64 references and the planted test
data of test_head_numerics_cpu.py and test_head_numerics_gpu.py.

The rule.  ``assert_within(got, ref64, tol64, tag)`` is the only comparison:
every element must satisfy |got - ref64| <= tol64.  No element is excluded
and no norm is taken, so one wrong tile cannot hide behind the rest of the
tensor the way it does under a relative Frobenius norm.

The tolerances are worst-case rounding bounds without fitted constants.
``U = 2^-8`` is the bf16 unit roundoff.  Every reference is fp64 arithmetic
on the kernel's actual inputs (the bf16 tensors as stored, upcast), and
every backward reference starts from the logits tensor the forward stored,
so each kernel is judged on its own operation.  ``mag`` is the reference
expression with every factor replaced by its absolute value.

  logits = bf16(cv W^T + bias)   U|ref| + (EP+2) 2^-23 mag
                                 (2^-23 per step covers a truncating MFMA
                                 adder; the library GEMM path rounds the
                                 bias to bf16 first: + U|bias|)
  lse                            (ceil(L/256)+64) 2^-24 + 2^-17 + 2^-22|ref|
                                 (longest serial fp32 chain of positive
                                 terms in any path; __expf/__logf argument
                                 rounding; ref = fp64 logsumexp of the
                                 stored bf16 logits)
  loss                           max_b tol(lse_b)
                                 + (B+32) 2^-24 max_b |lse_b - z[b, y_b]|
  G = coef_b (p - onehot)        U|ref| + 2^-14 coef_b (p + onehot)
  products of a bf16-rounded G   (2U + K 2^-23) mag + U|ref|
    (dW, dbias, dcv of           (one U: G's rounding; one U of slack for
    head_bwd.hip; K = B, B, L)   the fp32 lse/exp/coef errors, each < 1e-4
                                 relative, and second-order terms; the
                                 accumulation; the output rounding, absent
                                 for the fp32 dbias)
  products of exact bf16 inputs  U|ref| + K 2^-23 mag  (U|ref| only where
                                 the output is bf16)

Planted data.  Random data alone does not make an omitted edge visible, so
every case plants its edges (spike_plan): each distinct column of the
boundary set (BOUNDARY, clipped to [0, L)) carries a spike at least 20
above everything else in its row.  The i-th distinct column goes to row
i mod n, n = min(16, B - 1): with fewer rows than columns a row carries
several spikes of equal height, so that all boundary columns are planted
at every shape and losing any one of k spikes moves that row's lse by
log(k / (k - 1)); and at least one row of every case with B > 1 carries no
spike, because a spike swamps the rest of its row: only an unspiked row
feels a skipped chunk that holds no boundary column.  The labels of the
first rows sit on the same set, always including 0 and L-1.  Every skipped
column, tile or sub-step then costs an O(1) error on some row.
"""

from __future__ import annotations

import math

import torch

U = 2.0 ** -8
E23 = 2.0 ** -23
E24 = 2.0 ** -24

# negative entries count from L
BOUNDARY = (0, 7, 8, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 16383, 16384,
            -9, -8, -1)


def d(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().double()


# ---------------------------------------------------------------------------
# the rule


def violations(got, ref64, tol64) -> torch.Tensor:
    """Boolean mask of the elements that break |got - ref64| <= tol64 (a
    non-finite element always does)."""
    got = d(got)
    ref64 = d(ref64)
    tol64 = torch.as_tensor(tol64, dtype=torch.float64).expand_as(ref64)
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    return ~((got - ref64).abs() <= tol64)  # NaN compares false -> flagged


def _tile_report(bad: torch.Tensor, ratio: torch.Tensor) -> str:
    b2 = bad.reshape(1, -1) if bad.dim() < 2 else bad.reshape(bad.shape[0], -1)
    r2 = ratio.reshape(b2.shape)
    flat = int(torch.argmax(torch.where(b2, r2, torch.zeros_like(r2))))
    wr, wc = divmod(flat, b2.shape[1])
    rows, cols = torch.nonzero(b2, as_tuple=True)
    tiles = {}
    for r, c in zip((rows // 16).tolist(), (cols // 16).tolist()):
        tiles[(r, c)] = tiles.get((r, c), 0) + 1
    top = sorted(tiles.items(), key=lambda kv: (-kv[1], kv[0]))[:12]
    lines = [f"worst element [{wr}, {wc}] at |err|/tol = {r2[wr, wc]:.3g}",
             f"{len(tiles)} 16x16 tile(s) hold violations "
             "(row tile, column tile): count"]
    lines += [f"  ({tr}, {tc}): {n}" for (tr, tc), n in top]
    if len(tiles) > len(top):
        lines.append(f"  ... and {len(tiles) - len(top)} more tile(s)")
    return "\n".join(lines)


def assert_within(got, ref64, tol64, tag: str) -> float:
    """Assert that NO element violates |got - ref64| <= tol64; print and
    return max(|err| / tol).  A failure names the worst index and the
    number of violating elements per 16-row x 16-column tile."""
    bad = violations(got, ref64, tol64)
    g, r = d(got), d(ref64)
    tol = torch.as_tensor(tol64, dtype=torch.float64).expand_as(r)
    err = (g - r).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    ratio = torch.where(torch.isfinite(g), ratio,
                        torch.full_like(ratio, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"head_numerics {tag}: max |err|/tol = {worst:.3f} over "
          f"{ratio.numel()} elements, {int(bad.sum())} violation(s)")
    if bool(bad.any()):
        raise AssertionError(
            f"{tag}: {int(bad.sum())} of {bad.numel()} elements exceed the "
            f"bound\n" + _tile_report(bad, ratio))
    return worst


def frobenius(a, b) -> float:
    """The old metric, kept to print next to the rule's verdict."""
    a, b = d(a), d(b)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------
# planted data


def boundary_columns(L: int, labels_first: bool = False):
    """The 16 boundary columns clipped to [0, L).  ``labels_first`` puts 0
    and L-1 in front, so that even three rows carry both as labels."""
    cols = [min(max(c if c >= 0 else L + c, 0), L - 1) for c in BOUNDARY]
    if labels_first:
        cols = [cols[0], cols[-1]] + cols[1:-1]
    return cols


def planted_labels(B: int, L: int, g: torch.Generator) -> torch.Tensor:
    """Random labels with the first rows on the boundary set (0 and L-1
    always among them), one duplicate inside the first 64-row stage and one
    across two stages."""
    lab = torch.randint(0, L, (B,), generator=g)
    cols = boundary_columns(L, labels_first=True)
    for r in range(min(B, 16)):
        lab[r] = cols[r]
    if B > 17:
        lab[16] = lab[2]
    elif B > 3:
        lab[B - 1] = lab[B - 2]
    if B > 64:
        lab[B - 1] = lab[1]
    return lab


def spike_plan(B: int, L: int):
    """{boundary column: row that carries its spike}: the i-th distinct
    clipped boundary column goes to row i mod n, n = min(16, B - 1), so
    every boundary column is planted whatever B is and, for B > 1, the
    rows from n on stay unspiked."""
    n = max(1, min(16, B - 1))
    plan = {}
    for c in boundary_columns(L):
        if c not in plan:
            plan[c] = len(plan) % n
    return plan


def planted_logits(B: int, L: int, seed: int = 0) -> torch.Tensor:
    """bf16 logits for the loss-only tests: N(0, 3) with the spikes of
    spike_plan, each 20 above the maximum of its row's random part."""
    g = torch.Generator().manual_seed(seed + 1009 * B + L)
    z = torch.randn(B, L, generator=g) * 3
    top = z.max(dim=1).values + 20.0
    for c, r in spike_plan(B, L).items():
        z[r, c] = top[r]
    return z.to(torch.bfloat16)


class HeadCase:
    """Seeded inputs of one (B, L, EP) head shape, on the CPU.  cv, w are
    bf16, bias and weight fp32, label int64.  The spikes of spike_plan are
    planted through W and bias (w[c] = 40 cv_r / |cv_r|^2, bias[c] = 0 for
    column c of row r: a logit of about 40); ``spike_row`` is that plan.
    With B >= 32 the last 16 rows repeat the first 16 in reverse, so the
    last batch tile sees the same spikes."""

    def __init__(self, B: int, L: int, EP: int = 128):
        g = torch.Generator().manual_seed(1000003 * B + 7 * L + EP)
        cv = (torch.randn(B, EP, generator=g) * 0.5).to(torch.bfloat16)
        w = (torch.randn(L, EP, generator=g) * 0.1).to(torch.bfloat16)
        bias = torch.randn(L, generator=g)
        if B >= 32:
            for r in range(16):
                cv[B - 1 - r] = cv[r]
        self.spike_row = spike_plan(B, L)
        for c, r in self.spike_row.items():
            v = cv[r].double()
            w[c] = (40.0 / float(v @ v) * v).to(torch.bfloat16)
            bias[c] = 0.0
        self.B, self.L, self.EP = B, L, EP
        self.cv, self.w, self.bias = cv, w, bias
        self.label = planted_labels(B, L, g)
        self.weight = torch.rand(L, generator=g) + 0.5
        self.spike_cols = sorted(self.spike_row)


_CASES = {}


def head_case(B: int, L: int, EP: int = 128) -> HeadCase:
    """One HeadCase per shape, built once and shared read-only."""
    key = (B, L, EP)
    if key not in _CASES:
        _CASES[key] = HeadCase(B, L, EP)
    return _CASES[key]


# ---------------------------------------------------------------------------
# fp64 references and their bounds.  Each returns (ref, tol) or the pieces
# a bound is built from.


def logits_ref(cv, w, bias):
    """(ref, mag) of cv W^T + bias."""
    cv, w, bias = d(cv), d(w), d(bias)
    return cv @ w.t() + bias, cv.abs() @ w.abs().t() + bias.abs()


def logits_tol(ref, mag, EP: int, library_bias=None):
    tol = U * ref.abs() + (EP + 2) * E23 * mag
    if library_bias is not None:
        tol = tol + U * d(library_bias).abs()
    return tol


def merge_partials(pm, ps):
    """fp64 merge of per-block (max, sumexp) partials [GX, B] -> lse [B]."""
    pm, ps = d(pm), d(ps)
    m = pm.max(dim=0).values
    return m + torch.log((ps * torch.exp(pm - m)).sum(dim=0))


def lse_ref(z):
    """(ref, tol) of the row log-sum-exp of stored logits z [B, L]."""
    z = d(z)
    L = z.shape[1]
    ref = torch.logsumexp(z, dim=1)
    tol = ((math.ceil(L / 256) + 64) * E24 + 2.0 ** -17
           + 2.0 ** -22 * ref.abs())
    return ref, tol


def _row_weights(label, weight, B):
    if weight is None:
        return torch.ones(B, dtype=torch.float64)
    return d(weight)[label.cpu()]


def loss_ref(z, label, weight):
    """(ref, tol) of sum_b w_y (lse_b - z[b, y_b]) / sum_b w_y."""
    z = d(z)
    B = z.shape[0]
    lab = label.cpu()
    lse, ltol = lse_ref(z)
    nll = lse - z[torch.arange(B), lab]
    wy = _row_weights(lab, weight, B)
    ref = (wy * nll).sum() / wy.sum()
    tol = float(ltol.max()) + (B + 32) * E24 * float(nll.abs().max())
    return ref, torch.tensor(tol, dtype=torch.float64)


def g_ref(z, label, weight, gscale: float = 1.0, softmax: bool = True,
          shift: int = 0, exp_of=None):
    """(ref, mag) of G = coef_b (p - onehot) from stored logits z, with
    coef_b = gscale w_y / sum w_y and p = exp(z - lse64).  ``softmax=False``
    and ``shift`` build the mutated references of the CPU tests (softmax
    term deleted; one-hot shifted by ``shift`` columns).  ``exp_of`` (fp64
    logits) replaces z inside the exponential only: the streaming dcv
    kernel recomputes its logits from cv, W and bias but takes lse from the
    forward, which saw the stored ones."""
    z = d(z)
    B, L = z.shape
    lab = label.cpu()
    wy = _row_weights(lab, weight, B)
    coef = (gscale * wy / wy.sum())[:, None]
    p = torch.exp((z if exp_of is None else d(exp_of))
                  - torch.logsumexp(z, dim=1, keepdim=True))
    onehot = torch.zeros_like(z)
    onehot[torch.arange(B), (lab + shift) % L] = 1.0
    ref = coef * ((p if softmax else 0.0) - onehot)
    return ref, coef.abs() * (p + onehot)


def g_tol(ref, mag):
    return U * ref.abs() + 2.0 ** -14 * mag


def product(a, a_mag, b):
    """(ref, mag) of a @ b for an fp64 a with magnitude a_mag."""
    b = d(b)
    return a @ b, a_mag @ b.abs()


def rounded_g_tol(ref, mag, K: int, bf16_out: bool = True):
    """Bound for a product whose G operand was rounded to bf16 in-kernel."""
    tol = (2 * U + K * E23) * mag
    return tol + U * ref.abs() if bf16_out else tol


def exact_tol(ref, mag, K: int, bf16_out: bool = True):
    """Bound for a product of exact bf16 inputs accumulated in fp32."""
    tol = K * E23 * mag
    return tol + U * ref.abs() if bf16_out else tol


def fused_backward_refs(z, cv, w, label, weight, gscale: float = 1.0,
                        exp_of=None):
    """{name: (ref, tol)} for dW, dbias, dcv of the recompute-G backward
    over the stored logits z."""
    B, L = z.shape
    G, Gm = g_ref(z, label, weight, gscale, exp_of=exp_of)
    dw, dwm = product(G.t(), Gm.t(), cv)
    dcv, dcvm = product(G, Gm, w)
    db, dbm = G.sum(dim=0), Gm.sum(dim=0)
    return {"dW": (dw, rounded_g_tol(dw, dwm, B)),
            "dbias": (db, rounded_g_tol(db, dbm, B, bf16_out=False)),
            "dcv": (dcv, rounded_g_tol(dcv, dcvm, L))}


# ---------------------------------------------------------------------------
# K11 (angular.hip) references


def inv_rownorm_ref(x):
    ref = 1.0 / d(x).norm(dim=1).clamp_min(1e-12)
    return ref, 2.0 ** -20 * ref


def rowscale_ref(x, inv):
    ref = d(x) * d(inv)[:, None]
    return ref, U * ref.abs()


def dphi_dcos(c, cos_m: float, sin_m: float):
    """d phi / d cos of phi = c cos_m - sqrt(1 - c^2) sin_m."""
    return cos_m + sin_m * c / torch.sqrt((1.0 - c * c).clamp_min(1e-300))


def angular_fwd_ref(ucv, uw, label, cos_m, sin_m, s):
    """{'cos': (ref, tol), 'out': (ref, tol)} of the margin epilogue over
    the unit matrices the kernel was given."""
    ucv, uw = d(ucv), d(uw)
    B = ucv.shape[0]
    lab = label.cpu()
    c = ucv @ uw.t()
    acc = 130 * E23 * (ucv.abs() @ uw.abs().t())
    rows = torch.arange(B)
    cy = c[rows, lab]
    out = s * c
    oacc = s * acc
    phi = cy * cos_m - torch.sqrt((1.0 - cy * cy).clamp_min(0.0)) * sin_m
    pos = cy > 0
    out[rows, lab] = torch.where(pos, s * phi, s * cy)
    oacc[rows, lab] = torch.where(
        pos, oacc[rows, lab] * dphi_dcos(cy, cos_m, sin_m).abs(),
        oacc[rows, lab])
    return {"cos": (c, U * c.abs() + acc), "out": (out, U * out.abs() + oacc)}


def angular_dcos_ref(dout, cos, label, cos_m, sin_m, s, unit_margin=False):
    """(ref, tol) of dcos = dout s (d phi/d cos at label positions with
    cos > 0).  ``unit_margin`` is the CPU tests' mutation d phi/d cos = 1."""
    dout, cos = d(dout), d(cos)
    B = cos.shape[0]
    lab = label.cpu()
    rows = torch.arange(B)
    ref = dout * s
    cy = cos[rows, lab]
    if not unit_margin:
        ref[rows, lab] = ref[rows, lab] * torch.where(
            cy > 0, dphi_dcos(cy, cos_m, sin_m), torch.ones_like(cy))
    return ref, 2 * U * ref.abs()


def norm_project_ref(du, u, inv):
    du, u, inv = d(du), d(u), d(inv)[:, None]
    dot = (du * u).sum(dim=1, keepdim=True)
    ref = (du - dot * u) * inv
    mag = (du.abs() + (du.abs() * u.abs()).sum(dim=1, keepdim=True)
           * u.abs()) * inv.abs()
    return ref, U * ref.abs() + 130 * E23 * mag


def angular_case(B: int, L: int):
    """Seeded K11 inputs on the CPU: (cv bf16 [B,128], w bf16 [L,128],
    label).  Labels include 0 and L-1; the label rows of W are built so
    that the label cosine is well away from 0 and from 1 (alternately about
    +0.6 and -0.6): cos = 0 is phi's discontinuity, where a reference and
    an honest kernel may legitimately take different branches."""
    g = torch.Generator().manual_seed(31 * B + L)
    cv = (torch.randn(B, 128, generator=g) * 0.7).to(torch.bfloat16)
    w = (torch.randn(L, 128, generator=g) * 0.2)
    assert L >= B  # distinct labels: each label row of W serves one row
    label = torch.cat([torch.tensor([0]),
                       torch.randperm(L - 2, generator=g)[:B - 2] + 1,
                       torch.tensor([L - 1])])
    for b in range(B):
        v = cv[b].float()
        n = torch.randn(128, generator=g)
        n = n - (n @ v) / (v @ v) * v
        sign = 1.0 if b % 2 == 0 else -1.0
        w[label[b]] = 0.2 * (sign * 0.6 * v / v.norm()
                             + 0.8 * n / n.norm())
    return cv, w.to(torch.bfloat16), label


def crafted_cos(B, L, label):
    """A bf16 cosine tensor whose label entries cycle through
    {-0.5, 0, 0.5, 0.96875} (all exact in bf16), and a random upstream
    gradient."""
    g = torch.Generator().manual_seed(5 * B + L)
    cos = (torch.rand(B, L, generator=g) * 1.8 - 0.9).to(torch.bfloat16)
    vals = torch.tensor([-0.5, 0.0, 0.5, 0.96875])
    cos[torch.arange(B), label] = vals[torch.arange(B) % 4].to(torch.bfloat16)
    dout = (torch.randn(B, L, generator=g) * 0.05).to(torch.bfloat16)
    return cos, dout
