"""Streaming attention pool: scores from the combiner's flush, the forward
that reads the combiner output once from registers, and the compact backward
with a method's rows in registers.

The new kernels keep every summation order of the tiled kernels, so the
extension-level checks are bitwise against those on the same buffers; the
accuracy check uses ops/reference.py in fp32 as the independent reference
(tests/README.md).
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import reference as R

E, EP, KP = 100, 128, 32

# (1,1) smallest; (3,5) span 2 with a ragged last wave; (2,16)/(2,17) a
# group's second row appears; (5,199) uneven spans 50/50/50/49; (2,200)
# M = 400: not a multiple of the 128-row combiner tile, several blocks
SHAPES = [(1, 1), (3, 5), (2, 16), (2, 17), (5, 199), (2, 200)]


def relerr(a, b):
    a = a.detach().float()
    b = b.detach().float()
    d = (a - b).norm()
    n = b.norm()
    return float(d / n) if float(n) > 0 else float(d)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _inputs(B, C, kp, dev, seed):
    """The inputs of test_backward_fusions_gpu._inputs: 30% scattered masked
    contexts, first context masked, last one valid, method 1 fully masked
    (where there is a method 1)."""
    g = torch.Generator().manual_seed(seed)
    M = B * C
    x = torch.randn(M, kp, generator=g)
    w = torch.zeros(EP, kp)
    w[:E] = torch.randn(E, kp, generator=g) * (0.4 / kp ** 0.5)
    gamma = torch.zeros(EP)
    gamma[:E] = torch.rand(E, generator=g) + 0.5
    beta = torch.zeros(EP)
    beta[:E] = torch.randn(E, generator=g) * 0.1
    a = torch.zeros(EP)
    a[:E] = torch.randn(E, generator=g) * 0.2
    starts = torch.randint(1, 100, (B, C), generator=g, dtype=torch.int32)
    starts[torch.rand(B, C, generator=g) < 0.3] = 0
    starts[0, 0] = 0
    if B > 1:
        starts[1, :] = 0
    starts[B - 1, C - 1] = 7
    g_cvb = torch.zeros(B, EP)
    g_cvb[:, :E] = torch.randn(B, E, generator=g) * 0.1
    g_cv32 = torch.zeros(B, EP)
    g_cv32[:, :E] = torch.randn(B, E, generator=g) * 0.1
    g_attn = torch.randn(B, C, generator=g) * 0.1
    return dict(
        x=x.to(dev, torch.bfloat16), w=w.to(dev, torch.bfloat16),
        gamma=gamma.to(dev), beta=beta.to(dev), a=a.to(dev),
        starts=starts.to(dev), g_cvb=g_cvb.to(dev, torch.bfloat16),
        g_cv32=g_cv32.to(dev), g_attn=g_attn.to(dev))


def _forward(t, B, C, p, stream):
    """combiner + attention forward at the extension level, old or new."""
    from code2vec_amd.ops import ext
    from code2vec_amd.ops import functional as Fn

    dev = t["x"].device
    M = B * C
    out = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
    z = torch.empty_like(out)
    mean = torch.empty(M, dtype=torch.float32, device=dev)
    rstd = torch.empty_like(mean)
    cv = torch.empty(B, EP, dtype=torch.float32, device=dev)
    cvb = torch.empty(B, EP, dtype=torch.bfloat16, device=dev)
    attn = torch.empty(B, C, dtype=torch.float32, device=dev)
    Fn.reseed_dropout_rng(1234)
    seed, off_t = Fn._philox_state(dev)
    if stream:
        raw = torch.full((M,), float("nan"), device=dev)
        wrote = ext().combiner_fwd_scores(
            t["x"], t["w"], t["gamma"], t["beta"], t["a"], out, z, mean,
            rstd, raw, E, p, seed, off_t, 1)
        assert wrote
        ext().attention_fwd_scores(out.view(B, C, EP), raw, t["starts"], cv,
                                   cvb, attn, E)
    else:
        ext().combiner_fwd(t["x"], t["w"], t["gamma"], t["beta"], out, z,
                           mean, rstd, E, p, seed, off_t, 1)
        ext().attention_fwd_cvb(out.view(B, C, EP), t["a"], t["starts"], cv,
                                cvb, attn, E)
    return dict(out=out, z=z, mean=mean, rstd=rstd, attn=attn, cv=cv, cvb=cvb)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("B,C", SHAPES)
def test_stream_kernels_match_tiled_bitwise(dev, B, C, p):
    from code2vec_amd.ops import ext

    t = _inputs(B, C, KP, dev, seed=300 + 7 * B + C)
    old = _forward(t, B, C, p, stream=False)
    new = _forward(t, B, C, p, stream=True)
    for k in ("out", "z", "mean", "rstd", "attn", "cv", "cvb"):
        assert torch.equal(new[k], old[k]), k

    ccv = old["out"].view(B, C, EP)
    none_t = torch.empty(0, dtype=torch.float32, device=dev)
    for dcv in (t["g_cv32"], t["g_cvb"]):
        for has_dattn in (False, True):
            dattn = t["g_attn"] if has_dattn else none_t
            res = []
            for stream in (False, True):
                # NaN-filled: an element a kernel skips cannot compare equal
                ds = torch.full((B * C,), float("nan"), device=dev)
                da_p = torch.full((B, EP), float("nan"), device=dev)
                if stream:
                    ext().attention_bwd_compact_reg(
                        dcv, dattn, ccv, t["starts"], old["attn"], ds, da_p,
                        E, has_dattn)
                else:
                    ext().attention_bwd_compact(
                        dcv, dattn, ccv, t["a"], t["starts"], old["attn"],
                        ds, da_p, E, has_dattn)
                res.append((ds, da_p))
            tag = f"{dcv.dtype} dattn={has_dattn}"
            assert not torch.isnan(res[0][0]).any(), tag
            assert torch.equal(res[1][0], res[0][0]), "ds " + tag
            assert torch.equal(res[1][1], res[0][1]), "da partials " + tag


# ---------------------------------------------------------------------------
# gates: through CombinerAttentionPool, C = 201 and each switch at 0 take
# the tiled kernels and give the bits of the unfused chain
def _run(fused, t, B, C, p):
    from code2vec_amd.ops import functional as Fn

    leaves = [t[k].detach().clone().requires_grad_(True)
              for k in ("x", "w", "gamma", "beta", "a")]
    xh, wh, gh, bh, ah = leaves
    Fn.reseed_dropout_rng(1234)
    if fused:
        cv, attn, cvb = Fn.CombinerAttentionPool.apply(
            xh, wh, gh, bh, ah, t["starts"], E, p, True)
    else:
        y = Fn.CombinerLNTanh.apply(xh, wh, gh, bh, E, p, True)
        cv, attn = Fn.AttentionPool.apply(y.view(B, C, EP), ah, t["starts"],
                                          E)
        cvb = cv.to(torch.bfloat16)
    torch.autograd.backward([cvb, cv, attn],
                            [t["g_cvb"], t["g_cv32"], t["g_attn"]])
    return dict(cv=cv.detach(), attn=attn.detach(), cvb=cvb.detach(),
                dx=xh.grad, dw=wh.grad, dgamma=gh.grad, dbeta=bh.grad,
                da=ah.grad)


KEYS = ("cv", "attn", "cvb", "dx", "dw", "dgamma", "dbeta", "da")


@pytest.mark.parametrize("fwd,bwd,C", [
    (True, True, 200), (True, True, 201), (False, True, 200),
    (True, False, 200), (False, False, 200)])
def test_gates(dev, monkeypatch, fwd, bwd, C):
    from code2vec_amd.ops import functional as Fn

    B, p = 2, 0.25
    monkeypatch.setattr(Fn, "_ATTN_STREAM_FWD", fwd)
    monkeypatch.setattr(Fn, "_ATTN_STREAM_BWD", bwd)
    # record which extension entry points the fused node calls
    real, calls = Fn.ext(), []

    class Spy:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(real, name)

    spy = Spy()
    monkeypatch.setattr(Fn, "ext", lambda: spy)
    t = _inputs(B, C, KP, dev, seed=77 + C)
    chain = _run(False, t, B, C, p)
    del calls[:]
    fused = _run(True, t, B, C, p)
    for k in KEYS:
        assert torch.equal(fused[k], chain[k]), k
    new_fwd = fwd and C <= 200
    new_bwd = bwd and C <= 200
    assert ("attention_fwd_scores" in calls) == new_fwd
    assert ("combiner_fwd_scores" in calls) == new_fwd
    assert ("attention_fwd_cvb" in calls) == (not new_fwd)
    assert ("attention_bwd_compact_reg" in calls) == new_bwd
    assert ("attention_bwd_compact" in calls) == (not new_bwd)


# ---------------------------------------------------------------------------
# accuracy of the new path on its own, against ops/reference.py in fp32
@pytest.mark.parametrize("B,C", [(2, 200), (3, 5)])
def test_stream_path_accuracy(dev, B, C):
    from code2vec_amd.ops import ext

    t = _inputs(B, C, KP, dev, seed=300 + 7 * B + C)
    new = _forward(t, B, C, 0.25, stream=True)
    ccv = new["out"].view(B, C, EP)
    ds = torch.empty(B * C, dtype=torch.float32, device=dev)
    da_p = torch.empty(B, EP, dtype=torch.float32, device=dev)
    dcv = t["g_cv32"]
    ext().attention_bwd_compact_reg(dcv, t["g_attn"], ccv, t["starts"],
                                    new["attn"], ds, da_p, E, True)
    da = da_p.sum(dim=0)

    # the reference is fed the bf16 tensor the kernels are fed, as the
    # attention oracle of test_kernels_gpu.py is
    y = ccv[:, :, :E].float().requires_grad_(True)
    ar = t["a"][:E].clone().requires_grad_(True)
    mask = (t["starts"] > 0).float()
    cv_r, attn_r = R.attention_code_vector(y, ar, mask)
    torch.autograd.backward([cv_r, attn_r], [dcv[:, :E], t["g_attn"]])
    e_attn = relerr(new["attn"], attn_r)
    e_cv = relerr(new["cv"][:, :E], cv_r)
    e_da = relerr(da[:E], ar.grad)
    print(f"stream ({B},{C}): attn {e_attn:.3e} cv {e_cv:.3e} da {e_da:.3e}")
    # tolerances of test_kernels_gpu.py: 2e-2 forward, 4e-2 backward
    assert e_attn < 2e-2
    assert e_cv < 2e-2
    assert e_da < 4e-2
    assert torch.all(new["cv"][:, E:] == 0)
    assert torch.all(da[E:] == 0)
