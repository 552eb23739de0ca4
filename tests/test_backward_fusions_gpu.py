"""Backward fusions: the combiner+attention node that never writes the
attention gradient, and the one-launch reductions.

Bitwise checks compare each new path with the chain it replaces on the
same inputs; accuracy checks use plain torch / ops/reference.py in fp32 or
float64 as the independent reference (tests/README.md).
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import reference as R


def relerr(a, b):
    a = a.detach().float()
    b = b.detach().float()
    d = (a - b).norm()
    n = b.norm()
    return float(d / n) if float(n) > 0 else float(d)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# 1. CombinerAttentionPool vs CombinerLNTanh -> view -> AttentionPool ->
#    .to(bf16), bitwise, and both against the fp32 oracle
E, EP = 100, 128


def _inputs(B, C, KP, dev, seed):
    g = torch.Generator().manual_seed(seed)
    M = B * C
    x = torch.randn(M, KP, generator=g)
    w = torch.zeros(EP, KP)
    w[:E] = torch.randn(E, KP, generator=g) * (0.4 / KP ** 0.5)
    gamma = torch.zeros(EP)
    gamma[:E] = torch.rand(E, generator=g) + 0.5
    beta = torch.zeros(EP)
    beta[:E] = torch.randn(E, generator=g) * 0.1
    a = torch.zeros(EP)
    a[:E] = torch.randn(E, generator=g) * 0.2
    starts = torch.randint(1, 100, (B, C), generator=g, dtype=torch.int32)
    starts[torch.rand(B, C, generator=g) < 0.3] = 0  # scattered masked
    starts[0, 0] = 0
    starts[B - 1, C - 1] = 7
    starts[1, :] = 0                                  # one method all masked
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


def _run(fused, t, B, C, p, extra):
    from code2vec_amd.ops import functional as Fn

    leaves = [t[k].detach().clone().requires_grad_(True)
              for k in ("x", "w", "gamma", "beta", "a")]
    xh, wh, gh, bh, ah = leaves
    Fn.reseed_dropout_rng(1234)
    if fused:
        cv, attn, cvb = Fn.CombinerAttentionPool.apply(
            xh, wh, gh, bh, ah, t["starts"], E, p, True)
        y = None
    else:
        y = Fn.CombinerLNTanh.apply(xh, wh, gh, bh, E, p, True)
        cv, attn = Fn.AttentionPool.apply(y.view(B, C, EP), ah, t["starts"],
                                          E)
        cvb = cv.to(torch.bfloat16)
    outs, grads = [cvb], [t["g_cvb"]]
    if extra:
        outs += [cv, attn]
        grads += [t["g_cv32"], t["g_attn"]]
    torch.autograd.backward(outs, grads)
    res = dict(cv=cv.detach(), attn=attn.detach(), cvb=cvb.detach(),
               dx=xh.grad, dw=wh.grad, dgamma=gh.grad, dbeta=bh.grad,
               da=ah.grad)
    return res, (y.detach() if y is not None else None)


def _oracle(t, B, C, p, extra, y_chain):
    """fp32 torch/reference math on the same operands; the dropout mask is
    the kernel's own (recovered from the chain's combiner output).  As in
    the per-op tests of test_kernels_gpu.py, whose attention oracle is fed
    the bf16 tensor the attention kernel is fed, the attention part sees
    the combiner output rounded to bf16 (value of the chain's, gradient of
    the fp32 math): their tolerances are for that comparison."""
    xr, wr, gr, br, ar = [t[k].detach().float().requires_grad_(True)
                          for k in ("x", "w", "gamma", "beta", "a")]
    z = xr @ wr.t()
    u = F.layer_norm(z[:, :E], (E,), gr[:E], br[:E], 1e-5)
    y = torch.tanh(u)
    if p > 0:
        keep = (y_chain[:, :E].float() != 0).float()
        y = y * keep / (1.0 - p)
    assert relerr(y_chain[:, :E], y) < 2e-2
    y = y + (y_chain[:, :E].float() - y).detach()
    mask = (t["starts"] > 0).float()
    cv, attn = R.attention_code_vector(y.view(B, C, E), ar[:E], mask)
    # the kernels see the f32 sum of both cv gradients
    g_cv = t["g_cvb"].float()[:, :E]
    outs, grads = [cv], [g_cv]
    if extra:
        grads = [g_cv + t["g_cv32"][:, :E]]
        outs.append(attn)
        grads.append(t["g_attn"])
    torch.autograd.backward(outs, grads)
    return dict(cv=cv.detach(), attn=attn.detach(), dx=xr.grad, dw=wr.grad,
                dgamma=gr.grad, dbeta=br.grad, da=ar.grad)


CAP_CASES = [(B, C, KP, p, False)
             for (B, C) in ((3, 5), (2, 200))
             for KP in (32, 320)
             for p in (0.0, 0.25)] + [
                 (3, 5, 320, 0.25, True),
                 # C = 1000 no longer fits the LDS-staged attention kernels:
                 # the unstaged compact backward, with and without dattn
                 (2, 1000, 32, 0.25, False),
                 (2, 1000, 32, 0.25, True)]


@pytest.mark.parametrize("B,C,KP,p,extra", CAP_CASES)
def test_fused_node_matches_chain_bitwise_and_oracle(dev, B, C, KP, p, extra):
    t = _inputs(B, C, KP, dev, seed=100 + B + KP)
    chain, y_chain = _run(False, t, B, C, p, extra)
    fused, _ = _run(True, t, B, C, p, extra)
    for k in ("cv", "attn", "cvb", "dx", "dw", "dgamma", "dbeta", "da"):
        assert torch.equal(fused[k], chain[k]), k
    ref = _oracle(t, B, C, p, extra, y_chain)
    # tolerances of test_kernels_gpu.py: 2e-2 forward, 4e-2 backward
    assert relerr(fused["attn"], ref["attn"]) < 2e-2
    assert relerr(fused["cv"][:, :E], ref["cv"]) < 2e-2
    assert relerr(fused["dx"], ref["dx"]) < 4e-2
    assert relerr(fused["dw"][:E], ref["dw"][:E]) < 4e-2
    assert relerr(fused["dgamma"][:E], ref["dgamma"][:E]) < 4e-2
    assert relerr(fused["dbeta"][:E], ref["dbeta"][:E]) < 4e-2
    assert relerr(fused["da"][:E], ref["da"][:E]) < 4e-2
    assert torch.all(fused["dw"].float()[E:] == 0)
    assert torch.all(fused["da"][E:] == 0)


# ---------------------------------------------------------------------------
# 2. wgrad_reduce: [S, KP, EP] f32 slabs -> [EP, KP] bf16
@pytest.mark.parametrize("KP", [32, 320])
def test_wgrad_reduce_accuracy(dev, KP):
    from code2vec_amd.ops import ext

    S = 256
    g = torch.Generator().manual_seed(7 + KP)
    scale = 10.0 ** torch.randint(-3, 4, (S, KP, EP), generator=g).float()
    part = (torch.randn(S, KP, EP, generator=g) * scale).to(dev)
    p64 = part.double()
    s64 = p64.sum(dim=0).t()                 # [EP, KP]
    sabs = p64.abs().sum(dim=0).t()
    # recursive fp32 summation of 256 terms + one bf16 rounding
    bound = 255 * 2.0 ** -24 * sabs + 2.0 ** -8 * s64.abs()

    dw = torch.empty(EP, KP, dtype=torch.bfloat16, device=dev)
    ext().wgrad_reduce(part, dw)
    chain = part.sum(dim=0).t().contiguous().to(torch.bfloat16)
    err_new = (dw.double() - s64).abs()
    err_old = (chain.double() - s64).abs()
    print(f"wgrad_reduce KP={KP}: max err/bound new "
          f"{float((err_new / bound).max()):.4f} old "
          f"{float((err_old / bound).max()):.4f}")
    assert torch.all(err_old <= bound)       # the inputs are fair
    assert torch.all(err_new <= bound)
    dw2 = torch.empty_like(dw)
    ext().wgrad_reduce(part, dw2)
    assert torch.equal(dw, dw2)


# ---------------------------------------------------------------------------
# 3. slab_sum_bf16 with 8 loads in flight: same order, same bits
@pytest.mark.parametrize("S", [1, 7, 71])
@pytest.mark.parametrize("N", [129, 256, 1024 * 128])
def test_slab_sum_bf16_bitwise(dev, S, N):
    from code2vec_amd.ops import ext

    g = torch.Generator().manual_seed(S * 1000 + N % 997)
    part = torch.randn(S, N, generator=g).to(dev)
    acc = torch.zeros(N, dtype=torch.float32, device=dev)
    for s in range(S):
        acc = acc + part[s]
    out = torch.empty(N, dtype=torch.bfloat16, device=dev)
    ext().slab_sum_bf16(part, out)
    assert torch.equal(out, acc.to(torch.bfloat16))


# ---------------------------------------------------------------------------
# 4. dgamma+dbeta in one launch; loss partials -> acc and loss in one launch
@pytest.mark.parametrize("S", [1, 64, 300])
def test_slab_sum2_bitwise(dev, S):
    from code2vec_amd.ops import ext

    N = 128
    g = torch.Generator().manual_seed(S)
    p0 = torch.randn(S, N, generator=g).to(dev)
    p1 = (torch.randn(S, N, generator=g) * 3).to(dev)
    r0 = torch.empty(N, dtype=torch.float32, device=dev)
    r1 = torch.empty_like(r0)
    ext().slab_sum_f32(p0, r0)
    ext().slab_sum_f32(p1, r1)
    o0 = torch.empty_like(r0)
    o1 = torch.empty_like(r0)
    ext().slab_sum2_f32(p0, p1, o0, o1)
    assert torch.equal(o0, r0) and torch.equal(o1, r1)
    for o, p in ((o0, p0), (o1, p1)):
        s64 = p.double().sum(dim=0)
        tol = S * 2.0 ** -24 * p.double().abs().sum(dim=0)
        assert torch.all((o.double() - s64).abs() <= tol)


@pytest.mark.parametrize("S", [1, 64, 300])
def test_loss_reduce_bitwise(dev, S):
    from code2vec_amd.ops import ext

    g = torch.Generator().manual_seed(50 + S)
    acc_p = torch.empty(S, 2)
    acc_p[:, 0] = torch.rand(S, generator=g) * 40      # sum w_y * nll
    acc_p[:, 1] = torch.rand(S, generator=g) * 4 + 0.5  # sum w_y
    acc_p = acc_p.to(dev)
    ref_acc = torch.empty(2, dtype=torch.float32, device=dev)
    ext().slab_sum_f32(acc_p, ref_acc)
    ref_loss = ref_acc[0] / ref_acc[1]
    acc = torch.empty(2, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ext().loss_reduce(acc_p, acc, loss)
    assert torch.equal(acc, ref_acc)
    assert torch.equal(loss, ref_loss)
    s64 = acc_p.double().sum(dim=0)
    assert torch.all((acc.double() - s64).abs() <= S * 2.0 ** -24 * s64)
    l64 = s64[0] / s64[1]
    assert abs(float(loss) - float(l64)) <= (2 * S + 1) * 2.0 ** -24 * float(l64)
