"""The head-numerics rule (tests/head_numerics.py) is neither loose nor
tight: (a) a torch CPU emulation of the kernels, with their rounding points
(fp32 math, G -> bf16, fp32 accumulation, bf16 or fp32 output), passes every
bound with zero violations; (b) mutations of the fp64 reference - each a
plausible kernel bug - are flagged at the planted elements they target; (c)
for the first three mutations the old relative-Frobenius number is printed
next to the verdict, and test_old_metric_was_blind_on_its_own_inputs repeats
them on the random inputs of the older tests, where that number stays under
the older tests' bounds: this records why the old metric was blind.

No GPU: this file covers every shape of test_head_numerics_gpu.py with
B * L <= 1e6.  Run with -s to see the ratios.
"""

import math

import pytest
import torch

import head_numerics as H

bf16 = torch.bfloat16

FWD_SHAPES = [(8, 8, 128), (72, 1096, 128), (136, 2040, 128),
              (8, 98312, 128), (1, 1, 32), (65, 257, 96), (5, 997, 320)]
LOSS_SHAPES = [(3, 5), (33, 2055), (3, 32768), (3, 32777), (8, 32776)]
FUSED_SHAPES = [(8, 8), (72, 1096), (136, 2040), (8, 98312)]
UNFUSED_SHAPES = [(33, 1097), (64, 1096)]
K11_SHAPES = [(64, 2048), (33, 517)]
COS_M, SIN_M, S = math.cos(0.5), math.sin(0.5), 30.0


# ---------------------------------------------------------------------------
# the emulation: fp32 torch with the kernels' rounding points


def emu_logits(c):
    return (c.cv.float() @ c.w.float().t() + c.bias).to(bf16)


def emu_lse(z):
    return torch.logsumexp(z.float(), dim=1)


def emu_loss(z, label, weight):
    lse = emu_lse(z)
    nll = lse - z.float()[torch.arange(z.shape[0]), label]
    wy = weight[label] if weight is not None else torch.ones_like(nll)
    return (wy * nll).sum() / wy.sum()


def emu_g(z, label, weight, gscale=1.0):
    B = z.shape[0]
    wy = weight[label] if weight is not None else torch.ones(B)
    coef = (torch.tensor(gscale, dtype=torch.float32) * wy / wy.sum())[:, None]
    g = coef * torch.exp(z.float() - emu_lse(z)[:, None])
    g[torch.arange(B), label] -= coef[:, 0]
    return g.to(bf16)


def emu_fused_backward(z, c, gscale=1.0):
    g = emu_g(z, c.label, c.weight, gscale).float()
    return {"dW": (g.t() @ c.cv.float()).to(bf16), "dbias": g.sum(dim=0),
            "dcv": (g @ c.w.float()).to(bf16)}


# ---------------------------------------------------------------------------
# (a) accept


@pytest.mark.parametrize("B,L,EP", FWD_SHAPES)
def test_emulated_forward_accepted(B, L, EP):
    c = H.head_case(B, L, EP)
    z = emu_logits(c)
    ref, mag = H.logits_ref(c.cv, c.w, c.bias)
    H.assert_within(z, ref, H.logits_tol(ref, mag, EP),
                    f"emu logits ({B},{L},{EP})")
    lref, ltol = H.lse_ref(z)
    H.assert_within(emu_lse(z), lref, ltol, f"emu lse ({B},{L},{EP})")
    # the planted spikes are what the data promises: every boundary column
    # stands at least 20 above all of its row but the row's other spikes
    z64 = H.d(z)
    assert set(c.spike_row) == set(H.boundary_columns(L))
    for col, r in c.spike_row.items():
        rest = z64[r].clone()
        rest[[k for k, v in c.spike_row.items() if v == r]] = -math.inf
        assert L == 1 or float(z64[r, col] - rest.max()) >= 20.0
        if B >= 32:  # the last batch tile repeats the first 16 rows
            assert bool((z[B - 1 - r] == z[r]).all())
    if B > 1:
        assert max(c.spike_row.values()) < B - 1  # an unspiked row is left


@pytest.mark.parametrize("B,L", LOSS_SHAPES)
@pytest.mark.parametrize("weighted", [True, False])
def test_emulated_loss_accepted(B, L, weighted):
    z = H.planted_logits(B, L)
    g = torch.Generator().manual_seed(B + L)
    label = H.planted_labels(B, L, g)
    weight = torch.rand(L, generator=g) + 0.5 if weighted else None
    lref, ltol = H.lse_ref(z)
    H.assert_within(emu_lse(z), lref, ltol, f"emu lse ({B},{L})")
    ref, tol = H.loss_ref(z, label, weight)
    H.assert_within(emu_loss(z, label, weight), ref, tol,
                    f"emu loss ({B},{L})")
    gref, gmag = H.g_ref(z, label, weight, 2.5)
    H.assert_within(emu_g(z, label, weight, 2.5), gref,
                    H.g_tol(gref, gmag), f"emu dlogits ({B},{L})")


@pytest.mark.parametrize("B,L", FUSED_SHAPES)
def test_emulated_fused_backward_accepted(B, L):
    c = H.head_case(B, L)
    z = emu_logits(c)
    got = emu_fused_backward(z, c)
    refs = H.fused_backward_refs(z, c.cv, c.w, c.label, c.weight)
    for name, (ref, tol) in refs.items():
        r = H.assert_within(got[name], ref, tol, f"emu {name} ({B},{L})")
        assert r <= 1.0


@pytest.mark.parametrize("B,L", UNFUSED_SHAPES)
def test_emulated_unfused_chain_accepted(B, L):
    c = H.head_case(B, L)
    z = emu_logits(c)
    dl = emu_g(z, c.label, c.weight)
    gref, gmag = H.g_ref(z, c.label, c.weight)
    H.assert_within(dl, gref, H.g_tol(gref, gmag), f"emu dlogits ({B},{L})")
    # each later stage from the stage's actual input, the bf16 dlogits
    d64 = H.d(dl)
    for name, got, (ref, mag), K, out16 in (
            ("dcv", (dl.float() @ c.w.float()).to(bf16),
             H.product(d64, d64.abs(), c.w), L, True),
            ("dW", (dl.float().t() @ c.cv.float()).to(bf16),
             H.product(d64.t(), d64.abs().t(), c.cv), B, True),
            ("dbias", dl.float().sum(dim=0),
             (d64.sum(dim=0), d64.abs().sum(dim=0)), B, False)):
        H.assert_within(got, ref, H.exact_tol(ref, mag, K, out16),
                        f"emu unfused {name} ({B},{L})")


@pytest.mark.parametrize("B,L", K11_SHAPES)
def test_emulated_k11_accepted(B, L):
    cv, w, label = H.angular_case(B, L)
    cv = cv.clone()
    cv[B // 2] = 0  # the all-zero row of the inv_rownorm contract
    inv_c = 1.0 / cv.float().norm(dim=1).clamp_min(1e-12)
    inv_w = 1.0 / w.float().norm(dim=1).clamp_min(1e-12)
    for x, inv in ((cv, inv_c), (w, inv_w)):
        ref, tol = H.inv_rownorm_ref(x)
        H.assert_within(inv, ref, tol, f"emu inv_rownorm ({B},{L})")
    ucv = (cv.float() * inv_c[:, None]).to(bf16)
    uw = (w.float() * inv_w[:, None]).to(bf16)
    ref, tol = H.rowscale_ref(w, inv_w)
    H.assert_within(uw, ref, tol, f"emu rowscale ({B},{L})")
    c32 = ucv.float() @ uw.float().t()
    rows = torch.arange(B)
    cy = c32[rows, label]
    out = c32.clone()
    out[rows, label] = torch.where(
        cy > 0, cy * COS_M - torch.sqrt((1 - cy * cy).clamp_min(0)) * SIN_M,
        cy)
    out = (out * S).to(bf16)
    refs = H.angular_fwd_ref(ucv, uw, label, COS_M, SIN_M, S)
    H.assert_within(c32.to(bf16), *refs["cos"], f"emu cos ({B},{L})")
    H.assert_within(out, *refs["out"], f"emu out ({B},{L})")
    cos, dout = H.crafted_cos(B, L, label)
    g = dout.float() * S
    cl = cos.float()[rows, label]
    g[rows, label] *= torch.where(
        cl > 0, COS_M + SIN_M * cl / torch.sqrt((1 - cl * cl).clamp_min(1e-12)),
        torch.ones_like(cl))
    ref, tol = H.angular_dcos_ref(dout, cos, label, COS_M, SIN_M, S)
    H.assert_within(g.to(bf16), ref, tol, f"emu dcos ({B},{L})")
    du = (g.to(bf16).float() @ uw.float()).to(bf16)
    dot = (du.float() * ucv.float()).sum(dim=1, keepdim=True)
    dcv = ((du.float() - dot * ucv.float()) * inv_c[:, None]).to(bf16)
    # the zero row's 1e12 scale makes its bound as wide as its values
    ref, tol = H.norm_project_ref(du, ucv, inv_c)
    H.assert_within(dcv, ref, tol, f"emu norm_project ({B},{L})")


# ---------------------------------------------------------------------------
# (b) reject, (c) the old metric


def flagged(got, ref, tol, tag, old_metric=False):
    """The rule must reject ``got``; returns the violation mask."""
    bad = H.violations(got, ref, tol)
    with pytest.raises(AssertionError):
        H.assert_within(got, ref, tol, tag)
    msg = f"  {tag}: {100.0 * float(bad.double().mean()):.1f}% flagged"
    if old_metric:
        msg += f"; old metric: relative Frobenius = {H.frobenius(got, ref):.3%}"
    print(msg)
    return bad


@pytest.fixture(scope="module", params=[(72, 1096), (136, 2040)])
def fused(request):
    B, L = request.param
    c = H.head_case(B, L)
    z = emu_logits(c)
    return c, z, H.fused_backward_refs(z, c.cv, c.w, c.label, c.weight)


def test_rejects_softmax_term_deleted(fused):
    c, z, refs = fused
    G, Gm = H.g_ref(z, c.label, c.weight, softmax=False)
    mut = {"dW": G.t() @ H.d(c.cv), "dbias": G.sum(dim=0),
           "dcv": G @ H.d(c.w)}
    for name in ("dW", "dbias", "dcv"):
        bad = flagged(mut[name], *refs[name], f"softmax deleted, {name}",
                      old_metric=True)
        assert float(bad.double().mean()) > 0.5
    # the spike columns' rows of dW lose an O(1) softmax mass
    assert bool(bad.any())
    assert bool(H.violations(mut["dW"], *refs["dW"])[c.spike_cols].any(dim=1)
                .all())


def test_rejects_last_label_rows_zeroed(fused):
    c, z, refs = fused
    for name in ("dW", "dbias"):
        mut = refs[name][0].clone()
        mut[c.L - 8:] = 0
        bad = flagged(mut, *refs[name], f"last 8 label rows zeroed, {name}",
                      old_metric=True)
        assert not bool(bad[:c.L - 8].any())
        # L-1 is a planted label and spike column, L-8 a spike column
        assert bool(bad[c.L - 1].any()) and bool(bad[c.L - 8].any())


def test_rejects_last_dcv_substep_omitted(fused):
    c, z, refs = fused
    G, _ = H.g_ref(z, c.label, c.weight)
    cut = (c.L - 1) // 32 * 32
    mut = G[:, :cut] @ H.d(c.w)[:cut]
    bad = flagged(mut, *refs["dcv"], "last 32-label sub-step omitted, dcv",
                  old_metric=True)
    # row 1 carries label L-1, another row the spike at L-1
    assert c.label[1] == c.L - 1 and c.spike_row[c.L - 1] != 1
    assert bool(bad[1].any()) and bool(bad[c.spike_row[c.L - 1]].any())


def test_rejects_batch_rows_past_64_omitted(fused):
    c, z, refs = fused
    G, _ = H.g_ref(z, c.label, c.weight)
    mut = G[:64].t() @ H.d(c.cv)[:64]
    bad = flagged(mut, *refs["dW"], "batch rows >= 64 omitted, dW")
    # row B-1 repeats row 0 (spike at column 0) and carries label L-1
    assert bool(bad[0].any()) and bool(bad[c.L - 1].any())


def test_rejects_lse_missing_columns(fused):
    c, z, _ = fused
    z64 = H.d(z)
    ref, tol = H.lse_ref(z)
    bad = flagged(torch.logsumexp(z64[:, :c.L - 8], dim=1), ref, tol,
                  "lse without its last 8 columns")
    # the rows that hold the spikes at L-8 and L-1
    assert bool(bad[c.spike_row[c.L - 8]]) and bool(bad[c.spike_row[c.L - 1]])
    keep = torch.ones(c.L, dtype=torch.bool)
    keep[256] = False
    bad = flagged(torch.logsumexp(z64[:, keep], dim=1), ref, tol,
                  "lse without column 256")
    assert bool(bad[c.spike_row[256]])  # the row of the spike at 256
    # loss-only data: the 7-element scalar tail of (33, 2055)
    z = H.planted_logits(33, 2055)
    ref, tol = H.lse_ref(z)
    bad = flagged(torch.logsumexp(H.d(z)[:, :2055 - 7], dim=1), ref, tol,
                  "lse without the scalar tail")
    # the row of the spike at L-1, and the unspiked rows 16..32
    assert bool(bad[H.spike_plan(33, 2055)[2054]]) and bool(bad[16:].all())


# the small-B, large-L shapes: the only ones that reach lsm_partial, the
# non-temporal stores and the 4096-label dcv chunk.  Here a row carries
# several spikes and the last row none.


def test_rejects_dropped_lsm_partial_chunks():
    B, L = 3, 32777
    z = H.planted_logits(B, L)
    z64 = H.d(z)
    ref, tol = H.lse_ref(z)
    plan = H.spike_plan(B, L)
    assert sorted(set(plan.values())) == [0, 1]
    for cut, what in ((32768, "the 9-element third chunk"),
                      (16384, "every chunk but the first")):
        bad = flagged(torch.logsumexp(z64[:, :cut], dim=1), ref, tol,
                      f"lse of (3,32777) without {what}")
        # spikes at L-9, L-8, L-1 (and 16384) sit on both spiked rows; the
        # unspiked row 2 feels any dropped column
        assert bool(bad.all())
    keep = torch.ones(L, dtype=torch.bool)
    keep[16384:32768] = False
    bad = flagged(torch.logsumexp(z64[:, keep], dim=1), ref, tol,
                  "lse of (3,32777) without the second chunk")
    assert bool(bad[plan[16384]]) and bool(bad[2])


@pytest.mark.parametrize("L", [32776, 98312, 131080])
def test_rejects_dropped_columns_at_large_vocab(L):
    B = 8
    c = H.head_case(B, L)
    z = emu_logits(c)
    z64 = H.d(z)
    ref, tol = H.lse_ref(z)
    bad = flagged(torch.logsumexp(z64[:, :L - 8], dim=1), ref, tol,
                  f"lse of (8,{L}) without the 8-label tail block")
    assert bool(bad[c.spike_row[L - 8]]) and bool(bad[c.spike_row[L - 1]])
    assert bool(bad[B - 1])  # the unspiked row
    keep = torch.ones(L, dtype=torch.bool)
    keep[4096:L - 4096] = False
    bad = flagged(torch.logsumexp(z64[:, keep], dim=1), ref, tol,
                  f"lse of (8,{L}) without columns 4096..L-4097")
    assert bool(bad[c.spike_row[4096]]) and bool(bad[c.spike_row[16384]])
    assert bool(bad[B - 1])
    # dcv with label chunks dropped from G: the chunk that starts at the
    # boundary column 16384 (1024-label chunks) or 4096 (4096-label
    # chunks), then all middle chunks
    ref, tol = H.fused_backward_refs(z, c.cv, c.w, c.label,
                                     c.weight)["dcv"]
    G, _ = H.g_ref(z, c.label, c.weight)
    w64 = H.d(c.w)
    chunk = 1024 if L <= 131072 else 4096
    first = 16384 if chunk == 1024 else 4096
    for lo, hi, what in ((first, first + chunk, "one middle chunk"),
                         (chunk, (L - 1) // chunk * chunk,
                          "all middle chunks")):
        keep = torch.ones(L, dtype=torch.bool)
        keep[lo:hi] = False
        bad = flagged(G[:, keep] @ w64[keep], ref, tol,
                      f"dcv of (8,{L}) without {what} of {chunk} labels")
        assert bool(bad[c.spike_row[first]].any())


def test_rejects_shifted_onehot(fused):
    c, z, refs = fused
    G, _ = H.g_ref(z, c.label, c.weight, shift=1)
    gref, gmag = H.g_ref(z, c.label, c.weight)
    bad = flagged(G, gref, H.g_tol(gref, gmag), "one-hot shifted, dlogits")
    rows = torch.arange(c.B)
    assert bool(bad[rows, c.label].all())
    flagged(G.t() @ H.d(c.cv), *refs["dW"], "one-hot shifted, dW")
    flagged(G @ H.d(c.w), *refs["dcv"], "one-hot shifted, dcv")


@pytest.mark.parametrize("B,L,EP", [(72, 1096, 128), (65, 257, 96)])
def test_rejects_forward_mutations(B, L, EP):
    c = H.head_case(B, L, EP)
    ref, mag = H.logits_ref(c.cv, c.w, c.bias)
    tol = H.logits_tol(ref, mag, EP)
    cv, w = H.d(c.cv), H.d(c.w)
    bad = flagged(cv @ w.t(), ref, tol, f"bias missing ({B},{L},{EP})")
    assert float(bad.double().mean()) > 0.9
    bad = flagged(cv[:, :EP - 32] @ w[:, :EP - 32].t() + H.d(c.bias), ref,
                  tol, f"last 32-wide k-chunk missing ({B},{L},{EP})")
    assert float(bad.double().mean()) > 0.9
    assert bool(bad[:, c.spike_cols].any(dim=0).all())


@pytest.mark.parametrize("B,L", K11_SHAPES)
def test_rejects_unit_margin_derivative(B, L):
    _, _, label = H.angular_case(B, L)
    cos, dout = H.crafted_cos(B, L, label)
    ref, tol = H.angular_dcos_ref(dout, cos, label, COS_M, SIN_M, S)
    mut, _ = H.angular_dcos_ref(dout, cos, label, COS_M, SIN_M, S,
                                unit_margin=True)
    bad = flagged(mut, ref, tol, f"d phi/d cos = 1 ({B},{L})")
    rows = torch.arange(B)
    pos = cos.float()[rows, label] > 0
    assert bool(bad[rows, label][pos].all())
    off = torch.ones(B, L, dtype=torch.bool)
    off[rows, label] = False
    assert not bool(bad[off].any())


def test_old_metric_was_blind_on_its_own_inputs():
    """(c) on the inputs TestFusedHeadLoss.test_matches_fp32_oracle draws
    (random data, seed 23, (96, 7320)): the three mutations stay under that
    test's bounds (3e-2 relative Frobenius, 1e-2 relative loss) and the
    rule rejects each of them."""
    B, L = 96, 7320
    g = torch.Generator().manual_seed(23)
    cv = (torch.randn(B, 128, generator=g) * 0.5).to(bf16)
    w = (torch.randn(L, 128, generator=g) * 0.1).to(bf16)
    bias = torch.randn(L, generator=g)
    label = torch.randint(0, L, (B,), generator=g)
    weight = torch.rand(L, generator=g) + 0.5
    z = (cv.float() @ w.float().t() + bias).to(bf16)
    refs = H.fused_backward_refs(z, cv, w, label, weight)
    G, _ = H.g_ref(z, label, weight, softmax=False)
    mut = G.t() @ H.d(cv)
    flagged(mut, *refs["dW"], "old inputs, softmax deleted, dW", True)
    assert H.frobenius(mut, refs["dW"][0]) < 3e-2
    flagged(G @ H.d(w), *refs["dcv"], "old inputs, softmax deleted, dcv",
            True)
    rows = [r for r in range(L - 1, -1, -1)
            if r not in set(label.tolist())][:16]
    mut = refs["dW"][0].clone()
    mut[rows] = 0
    bad = flagged(mut, *refs["dW"],
                  "old inputs, last 16 non-label rows of dW zeroed", True)
    assert H.frobenius(mut, refs["dW"][0]) < 3e-2
    assert bool(bad[rows].any(dim=1).all())
    ref, tol = H.lse_ref(z)
    cut = (L - 1) // 256 * 256
    mut = torch.logsumexp(H.d(z)[:, :cut], dim=1)
    flagged(mut, ref, tol, "old inputs, last partial 256-block off lse")
    lref, _ = H.loss_ref(z, label, weight)
    wy = H.d(weight)[label]
    zy = H.d(z)[torch.arange(B), label]
    lmut = (wy * (mut - zy)).sum() / wy.sum()
    rel = abs(float(lmut - lref)) / abs(float(lref))
    print(f"  old metric: |d loss| / loss = {rel:.3%} (bound 1%)")
    assert rel < 1e-2


def test_assert_within_reports_the_tile():
    ref = torch.zeros(40, 40, dtype=torch.float64)
    got = ref.clone()
    got[33, 17] = 1.0
    got[34, 18] = float("nan")
    with pytest.raises(AssertionError) as e:
        H.assert_within(got, ref, torch.full_like(ref, 0.5), "tile report")
    assert "(2, 1): 2" in str(e.value) and "2 of 1600" in str(e.value)
    assert H.assert_within(ref, ref, 0.0, "exact") == 0.0
