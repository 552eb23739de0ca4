"""The output head, the loss and K11 on the GPU under the elementwise fp64
rule of tests/head_numerics.py (bounds and planted data are described
there).  Shapes are the smallest that reach each tile tail and each
dispatch branch; none is the workload's own.  Every case runs twice and
must repeat bit for bit.  Run with -s to see max(|err|/tol) per output;
the figures of the MI355X run are in tests/README.md.
"""

import math

import pytest
import torch

import head_numerics as H

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import ext
from code2vec_amd.ops import functional as Fn

COS_M, SIN_M, S = math.cos(0.5), math.sin(0.5), 30.0


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def stop_after_gpu_fault():
    """A HIP error is sticky: nothing more is launched after one."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, stopping: {e}", returncode=3)


def twice(fn):
    """Run ``fn`` twice; every tensor it returns must repeat bit for bit."""
    a, b = fn(), fn()
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert torch.equal(x, y), "not deterministic run to run"
    return a


# ---------------------------------------------------------------------------
# forward: head_logits_with_stats / ext().head_fwd(_img)

# (72, 1096): grid 5x2, identity block mapping, 8-row batch tail, 72-label
# tail block; (136, 2040): grid 8x3 = 24, the XCD remap with GYB > 1;
# (8, 98312): nontemporal stores, 8-label tail block; (5, 997, 320): odd L,
# misaligned rows and the scalar tail store
FWD_CASES = [(8, 8, 128, "image"), (72, 1096, 128, "image"),
             (136, 2040, 128, "image"), (8, 98312, 128, "image"),
             (72, 1096, 128, "direct"), (1, 1, 32, "generic"),
             (65, 257, 96, "generic"), (5, 997, 320, "generic")]


@pytest.mark.parametrize("B,L,EP,path", FWD_CASES)
def test_forward(dev, monkeypatch, B, L, EP, path):
    if path == "direct":
        monkeypatch.setattr(Fn, "_HF_AIMG", False)
    c = H.head_case(B, L, EP)
    cv, w, bias = c.cv.to(dev), c.w.to(dev), c.bias.to(dev)
    label, weight = c.label.to(dev), c.weight.to(dev)
    wimg = []

    def run():
        logits = Fn.head_logits_with_stats(cv, w, bias)
        pm, ps = logits._c2v_lsm_partials
        assert hasattr(logits, "_c2v_wimg_a") == (path == "image")
        wimg[:] = [getattr(logits, "_c2v_wimg_a", None)]
        lse = torch.empty(B, dtype=torch.float32, device=dev)
        _, loss = Fn._finalize_stats(logits, pm, ps, label, weight, lse)
        return logits, pm, ps, lse, loss

    logits, pm, ps, lse, loss = twice(run)
    tag = f"({B},{L},{EP}) {path}"
    ref, mag = H.logits_ref(c.cv, c.w, c.bias)
    H.assert_within(logits, ref, H.logits_tol(ref, mag, EP),
                    f"fwd logits {tag}")
    lref, ltol = H.lse_ref(logits)
    H.assert_within(H.merge_partials(pm, ps), lref, ltol,
                    f"fwd lse of partials {tag}")
    H.assert_within(lse, lref, ltol, f"fwd lse finalize {tag}")
    H.assert_within(loss, *H.loss_ref(logits, c.label, c.weight),
                    f"fwd loss {tag}")
    # the no-stats variant stores the same bits
    plain = torch.full_like(logits, float("nan"))
    if path == "image":
        ext().head_fwd_img(cv, wimg[0], bias, plain, Fn._NONE_T, Fn._NONE_T,
                           L)
    else:
        ext().head_fwd(cv, w, bias, plain, Fn._NONE_T, Fn._NONE_T)
    assert torch.equal(plain, logits)


# ---------------------------------------------------------------------------
# the loss alone on planted logits

# (33, 2055): 7-element scalar tail, misaligned rows; (3, 32777):
# lsm_partial_kernel with a 9-element third chunk
LOSS_CASES = [(3, 5), (33, 2055), (3, 32768), (3, 32777)]


def check_loss(dev, z, label, weight, gscale, tag):
    """FusedLogSoftmaxNLL on logits z (device bf16): lse, loss and dlogits
    rules; returns dlogits."""
    wd = weight.to(dev) if weight is not None else None
    ld = label.to(dev)

    def run():
        zh = z.detach().clone().requires_grad_(True)
        loss = Fn.FusedLogSoftmaxNLL.apply(zh, ld, wd)
        lse = loss.grad_fn.saved_tensors[3].clone()
        (loss * gscale).backward()
        return loss.detach(), lse, zh.grad

    loss, lse, dl = twice(run)
    H.assert_within(lse, *H.lse_ref(z), f"loss lse {tag}")
    H.assert_within(loss, *H.loss_ref(z, label, weight), f"loss {tag}")
    gref, gmag = H.g_ref(z, label, weight, gscale)
    H.assert_within(dl, gref, H.g_tol(gref, gmag), f"loss dlogits {tag}")
    return dl


@pytest.mark.parametrize("B,L", LOSS_CASES)
def test_loss_alone(dev, B, L):
    z = H.planted_logits(B, L).to(dev)
    g = torch.Generator().manual_seed(B + L)
    label = H.planted_labels(B, L, g)
    weight = torch.rand(L, generator=g) + 0.5
    # non-uniform weights under a non-unit upstream gradient, then none
    check_loss(dev, z, label, weight, 2.5, f"({B},{L}) weighted x2.5")
    check_loss(dev, z, label, None, 1.0, f"({B},{L}) unweighted")


def test_loss_after_library_forward(dev, monkeypatch):
    """C2V_HEAD_FWD=0: the library GEMM forward (no stats partials), then
    lsm_partial + finalize over its logits."""
    monkeypatch.setattr(Fn, "_HEAD_FWD", False)
    B, L = 8, 32776
    c = H.head_case(B, L)
    logits = Fn.head_logits_with_stats(c.cv.to(dev), c.w.to(dev),
                                       c.bias.to(dev))
    assert not hasattr(logits, "_c2v_lsm_partials")
    ref, mag = H.logits_ref(c.cv, c.w, c.bias)
    H.assert_within(logits, ref,
                    H.logits_tol(ref, mag, 128, library_bias=c.bias),
                    f"library fwd logits ({B},{L})")
    check_loss(dev, logits, c.label, c.weight, 1.0, f"({B},{L}) library fwd")


# ---------------------------------------------------------------------------
# fused recompute-G backward over the forward's stored logits


def run_fused(c, dev, gscale=1.0, weight="case"):
    cv, w, bias = c.cv.to(dev), c.w.to(dev), c.bias.to(dev)
    label = c.label.to(dev)
    wt = c.weight.to(dev) if weight == "case" else weight

    def run():
        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        bh = bias.clone().requires_grad_(True)
        logits = Fn.head_logits_with_stats(cvh.detach(), wh.detach(),
                                           bh.detach())
        loss = Fn.FusedHeadLoss.apply(logits, cvh, wh, bh, label, wt)
        (loss * gscale).backward()
        return logits, loss.detach(), cvh.grad, wh.grad, bh.grad

    return twice(run)


def check_fused(c, dev, tag, gscale=1.0, recompute=False, weighted=True):
    weight = c.weight if weighted else None
    logits, loss, dcv, dw, dbias = run_fused(
        c, dev, gscale, "case" if weighted else None)
    assert dbias.dtype == torch.float32 and dw.dtype == torch.bfloat16
    H.assert_within(loss, *H.loss_ref(logits, c.label, weight),
                    f"fused loss {tag}")
    refs = H.fused_backward_refs(logits, c.cv, c.w, c.label, weight, gscale)
    if recompute:
        # The streaming dcv never reads the stored logits: its exponent is
        # the recomputed f32 logit (cv W^T + bias, unrounded) minus the
        # forward's lse, and that lse is of the bf16-ROUNDED stored logits.
        # The two differ by the logit's bf16 rounding (up to 2^-9 |z|,
        # 0.08 at the planted 40), so this G is not the exact softmax
        # gradient and differs from the logits-reading kernel's by that
        # factor.  The reference mirrors the kernel's definition: fp64
        # logits inside the exponential, lse of the stored ones.
        z64, _ = H.logits_ref(c.cv, c.w, c.bias)
        refs["dcv"] = H.fused_backward_refs(
            logits, c.cv, c.w, c.label, weight, gscale, exp_of=z64)["dcv"]
    got = {"dW": dw, "dbias": dbias, "dcv": dcv}
    for name, (ref, tol) in refs.items():
        H.assert_within(got[name], ref, tol, f"fused {name} {tag}")
    return got


# (136, 2040): GYB = 2 in dcv; (8, 98312): 1024-label chunk; (8, 131080):
# 4096-label chunk, 8-label tail
@pytest.mark.parametrize("B,L", [(8, 8), (72, 1096), (136, 2040),
                                 (8, 98312), (8, 131080)])
def test_fused_backward(dev, B, L):
    c = H.head_case(B, L)
    assert Fn.fused_head_loss_supported(c.cv.to(dev), c.w, True)
    check_fused(c, dev, f"({B},{L})")


def test_fused_backward_upstream_gradient(dev):
    check_fused(H.head_case(72, 1096), dev, "(72,1096) x2.5", gscale=2.5)


def test_fused_backward_unweighted(dev):
    check_fused(H.head_case(72, 1096), dev, "(72,1096) weight=None",
                weighted=False)


def test_fused_backward_dcv_chunk_512(dev, monkeypatch):
    monkeypatch.setenv("C2V_HB_DCV_CHUNK", "512")
    check_fused(H.head_case(72, 1096), dev, "(72,1096) chunk 512")


def test_fused_backward_streaming_dcv(dev, monkeypatch):
    monkeypatch.setattr(Fn, "_HB_RC", True)
    check_fused(H.head_case(72, 1096), dev, "(72,1096) streaming dcv",
                recompute=True)


def test_fused_backward_dw128(dev, monkeypatch):
    monkeypatch.setenv("C2V_HBDW128", "0")
    check_fused(H.head_case(72, 1096), dev, "(72,1096) dw128")


# ---------------------------------------------------------------------------
# unfused chain: OutputHead + FusedLogSoftmaxNLL, stage by stage


def run_unfused(c, dev):
    cv, w, bias = c.cv.to(dev), c.w.to(dev), c.bias.to(dev)
    label, weight = c.label.to(dev), c.weight.to(dev)

    def run():
        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        bh = bias.clone().requires_grad_(True)
        logits = Fn.OutputHead.apply(cvh, wh, bh)
        assert hasattr(logits, "_c2v_lsm_partials")
        logits.retain_grad()
        loss = Fn.FusedLogSoftmaxNLL.apply(logits, label, weight)
        loss.backward()
        return (logits.detach(), loss.detach(), logits.grad, cvh.grad,
                wh.grad, bh.grad)

    return twice(run)


# (33, 1097): rocBLAS dcv, colsum_bf16; (64, 1096): head_dgrad with three
# label splits; the same with C2V_HEAD_WGRAD=1: head_wgrad
@pytest.mark.parametrize("B,L,wgrad", [(33, 1097, False), (64, 1096, False),
                                       (64, 1096, True)])
def test_unfused_chain(dev, monkeypatch, B, L, wgrad):
    if wgrad:
        monkeypatch.setenv("C2V_HEAD_WGRAD", "1")
    c = H.head_case(B, L)
    logits, loss, dl, dcv, dw, dbias = run_unfused(c, dev)
    tag = f"({B},{L})" + (" head_wgrad" if wgrad else "")
    ref, mag = H.logits_ref(c.cv, c.w, c.bias)
    H.assert_within(logits, ref, H.logits_tol(ref, mag, 128),
                    f"unfused logits {tag}")
    H.assert_within(loss, *H.loss_ref(logits, c.label, c.weight),
                    f"unfused loss {tag}")
    gref, gmag = H.g_ref(logits, c.label, c.weight)
    H.assert_within(dl, gref, H.g_tol(gref, gmag), f"unfused dlogits {tag}")
    # each later stage from its actual input, the stored bf16 dlogits
    d64 = H.d(dl)
    ref, mag = H.product(d64, d64.abs(), c.w)
    H.assert_within(dcv, ref, H.exact_tol(ref, mag, L),
                    f"unfused dcv {tag}")
    ref, mag = H.product(d64.t(), d64.abs().t(), c.cv)
    H.assert_within(dw, ref, H.exact_tol(ref, mag, B), f"unfused dW {tag}")
    ref, mag = d64.sum(dim=0), d64.abs().sum(dim=0)
    assert dbias.dtype == torch.float32
    H.assert_within(dbias, ref, H.exact_tol(ref, mag, B, bf16_out=False),
                    f"unfused dbias {tag}")


# ---------------------------------------------------------------------------
# K11 stage by stage through ext()

K11_CASES = [(64, 2048), (33, 517)]
_K11 = {}


def k11_stage(B, L, dev):
    """Inputs plus the kernels' own inv norms and unit matrices, once per
    shape (each later stage is judged from these actual inputs)."""
    if (B, L) not in _K11:
        cv, w, label = H.angular_case(B, L)
        cv, w = cv.to(dev), w.to(dev)
        inv_c = torch.empty(B, dtype=torch.float32, device=dev)
        inv_w = torch.empty(L, dtype=torch.float32, device=dev)
        ext().inv_rownorm(cv, inv_c)
        ext().inv_rownorm(w, inv_w)
        ucv = torch.empty_like(cv)
        uw = torch.empty_like(w)
        ext().rowscale(cv, inv_c, ucv)
        ext().rowscale(w, inv_w, uw)
        _K11[(B, L)] = (cv, w, label, inv_c, inv_w, ucv, uw)
    return _K11[(B, L)]


@pytest.mark.parametrize("N", [1, 4, 517])
def test_k11_inv_rownorm_rowscale(dev, N):
    g = torch.Generator().manual_seed(N)
    x = (torch.randn(N, 128, generator=g)
         * torch.logspace(-3, 2, N)[:, None]).to(torch.bfloat16)
    x[N // 2] = 0  # contract: 1 / max(|x|, 1e-12)
    xd = x.to(dev)

    def run():
        inv = torch.full((N,), float("nan"), device=dev)
        ext().inv_rownorm(xd, inv)
        out = torch.full_like(xd, float("nan"))
        ext().rowscale(xd, inv, out)
        return inv, out

    inv, out = twice(run)
    H.assert_within(inv, *H.inv_rownorm_ref(x), f"inv_rownorm N={N}")
    H.assert_within(out, *H.rowscale_ref(x, inv), f"rowscale N={N}")


@pytest.mark.parametrize("B,L", K11_CASES)
def test_k11_angular_fwd(dev, B, L):
    cv, w, label, inv_c, inv_w, ucv, uw = k11_stage(B, L, dev)
    ld = label.to(dev)

    def run():
        out = torch.full((B, L), float("nan"), dtype=torch.bfloat16,
                         device=dev)
        cos = torch.full_like(out, float("nan"))
        ext().angular_fwd(ucv, uw, ld, out, cos, COS_M, SIN_M, S)
        return out, cos

    out, cos = twice(run)
    refs = H.angular_fwd_ref(ucv, uw, label, COS_M, SIN_M, S)
    # the data keeps every label cosine clear of phi's jump at 0
    cy = refs["cos"][0][torch.arange(B), label]
    assert float(cy.abs().min()) > 0.3 and float(cy.abs().max()) < 0.9
    assert bool((cy > 0).any()) and bool((cy < 0).any())
    H.assert_within(cos, *refs["cos"], f"angular_fwd cos ({B},{L})")
    H.assert_within(out, *refs["out"], f"angular_fwd out ({B},{L})")
    rows = torch.arange(B)
    ref, tol = refs["out"]
    H.assert_within(out.cpu()[rows, label], ref[rows, label],
                    tol[rows, label], f"angular_fwd out, labels ({B},{L})")


@pytest.mark.parametrize("B,L", K11_CASES)
def test_k11_angular_dcos(dev, B, L):
    _, _, label = H.angular_case(B, L)
    cos, dout = H.crafted_cos(B, L, label)
    cd, dd, ld = cos.to(dev), dout.to(dev), label.to(dev)

    def run():
        dcos = torch.full_like(cd, float("nan"))
        ext().angular_dcos(dd, cd, ld, dcos, COS_M, SIN_M, S)
        return (dcos,)

    dcos = twice(run)[0].cpu()
    ref, tol = H.angular_dcos_ref(dout, cos, label, COS_M, SIN_M, S)
    rows = torch.arange(B)
    # label and non-label positions separately: B label entries cannot be
    # diluted by the B * (L - 1) others
    H.assert_within(dcos[rows, label], ref[rows, label], tol[rows, label],
                    f"angular_dcos labels ({B},{L})")
    off = torch.ones(B, L, dtype=torch.bool)
    off[rows, label] = False
    H.assert_within(dcos[off], ref[off], tol[off],
                    f"angular_dcos non-labels ({B},{L})")


@pytest.mark.parametrize("B,L", K11_CASES)
def test_k11_norm_project(dev, B, L):
    cv, w, label, inv_c, inv_w, ucv, uw = k11_stage(B, L, dev)
    g = torch.Generator().manual_seed(B * L)
    for name, u, inv in (("cv", ucv, inv_c), ("w", uw, inv_w)):
        du = (torch.randn(u.shape[0], 128, generator=g) * 0.05).to(
            dev, torch.bfloat16)

        def run():
            out = torch.full_like(du, float("nan"))
            ext().norm_project(du, u, inv, out)
            return (out,)

        out = twice(run)[0]
        H.assert_within(out, *H.norm_project_ref(du, u, inv),
                        f"norm_project {name} ({B},{L})")


def run_k11(cv, w, label, dev):
    ld = label.to(dev)

    def run():
        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        out = Fn.AngularMarginHead.apply(cvh, wh, ld, COS_M, SIN_M, S)
        # the gradient a cross-entropy loss sends: softmax - onehot of the
        # head's own output
        dl = torch.softmax(out.detach().float(), dim=1)
        dl[torch.arange(cv.shape[0], device=dev), ld] -= 1.0
        dl = dl.to(torch.bfloat16)
        out.backward(dl)
        return out.detach(), dl, cvh.grad, wh.grad

    return twice(run)


# (64, 2048) takes the custom head_dgrad / head_wgrad branches, (33, 517)
# the rocBLAS fallbacks
@pytest.mark.parametrize("B,L", K11_CASES)
def test_k11_end_to_end(dev, B, L):
    from code2vec_amd.ops import reference as R

    cv, w, label = H.angular_case(B, L)
    out, dl, dcv, dw = run_k11(cv.to(dev), w.to(dev), label, dev)
    cvr = cv.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    ref = R.angular_margin_head(cvr, wr, label, COS_M, SIN_M, S)
    ref.backward(dl.cpu().double())
    for name, got, want in (("out", out, ref.detach()),
                            ("dcv", dcv, cvr.grad), ("dw", dw, wr.grad)):
        err = H.frobenius(got, want)
        print(f"head_numerics k11 end to end {name} ({B},{L}): relative "
              f"Frobenius = {err:.3e}")
        assert err < 4e-2


# ---------------------------------------------------------------------------
# scratch hygiene

SCRATCH_TAGS = ("hf_aimg", "head_cvimg", "head_wimg", "head_cvimg_a",
                "head_coef_lse", "head_fused_dcv", "head_wt", "head_dgrad",
                "ang_uw", "ang_uwt", "ang_dcv")


def test_scratch_buffers_are_fully_overwritten(dev, monkeypatch):
    """Persistent scratch is torch.empty memory that usually happens to be
    zero.  Filled with NaN between two runs, every output must come out
    finite and with the same bits: each buffer is fully overwritten by its
    producer, and tail-stage fragment reads hit written (zero-padded)
    chunks."""
    c = H.head_case(72, 1096)
    cu = H.head_case(64, 1096)
    k11 = [H.angular_case(33, 517), H.angular_case(64, 2048)]

    def run_all():
        outs = list(run_fused(c, dev))
        with monkeypatch.context() as m:
            m.setattr(Fn, "_HB_RC", True)
            outs += run_fused(c, dev)
        outs += run_unfused(cu, dev)
        for cv, w, label in k11:
            outs += run_k11(cv.to(dev), w.to(dev), label, dev)
        return outs

    first = run_all()
    seen = set()
    for key, buf in Fn._scratch_cache.items():
        tags = [t for t in SCRATCH_TAGS if t in key]
        if tags and buf.is_floating_point():
            buf.fill_(float("nan"))
            seen.update(tags)
    assert seen == set(SCRATCH_TAGS), set(SCRATCH_TAGS) - seen
    second = run_all()
    for a, b in zip(first, second):
        assert bool(torch.isfinite(a.float()).all())
        assert torch.equal(a, b)
