"""HIP kernel numerics vs the fp32 PyTorch oracle (ops/reference.py).

Every kernel is compared against the exact reference math computed in fp32;
tolerances account for bf16 storage/compute (rel. Frobenius < ~2%).
"""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import reference as R
from code2vec_amd.ops import round_up


def relerr(a, b):
    a = a.detach().float()
    b = b.detach().float()
    d = (a - b).norm()
    n = b.norm()
    return float(d / n) if float(n) > 0 else float(d)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_tables(T, P, dt, dp, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    TS, PS = round_up(dt), round_up(dp)
    term = torch.zeros(T, TS)
    path = torch.zeros(P, PS)
    term[:, :dt] = torch.randn(T, dt, generator=g)
    path[:, :dp] = torch.randn(P, dp, generator=g)
    return term.to(dev, torch.bfloat16), path.to(dev, torch.bfloat16), TS, PS


def make_batch(B, C, T, P, dev, seed=1, with_pad=True):
    g = torch.Generator().manual_seed(seed)
    starts = torch.randint(1, T, (B, C), generator=g, dtype=torch.int32)
    paths = torch.randint(1, P, (B, C), generator=g, dtype=torch.int32)
    ends = torch.randint(1, T, (B, C), generator=g, dtype=torch.int32)
    if with_pad:
        lens = torch.randint(1, C + 1, (B,), generator=g)
        mask = torch.arange(C)[None, :] >= lens[:, None]
        starts[mask] = 0
        paths[mask] = 0
        ends[mask] = 0
    return starts.to(dev), paths.to(dev), ends.to(dev)


# ---------------------------------------------------------------------------
class TestGatherConcat:
    def test_fwd(self, dev):
        from code2vec_amd.ops.functional import GatherConcat

        B, C, T, P, dt, dp = 8, 24, 500, 400, 100, 100
        term, path, TS, PS = make_tables(T, P, dt, dp, dev)
        starts, paths, ends = make_batch(B, C, T, P, dev)
        out = GatherConcat.apply(starts, paths, ends, term, path)
        assert out.shape == (B * C, 2 * TS + PS)
        # oracle on the padded fp32 tables
        ref = R.gather_concat(
            starts, paths, ends, term.float(), path.float()
        ).view(B * C, -1)
        assert torch.equal(out.float(), ref)  # pure gather: bitwise

    def test_bwd_matches_autograd(self, dev):
        from code2vec_amd.ops.functional import GatherConcat

        B, C, T, P, dt, dp = 4, 16, 300, 200, 36, 36
        term, path, TS, PS = make_tables(T, P, dt, dp, dev)
        starts, paths, ends = make_batch(B, C, T, P, dev)
        term_l = term.detach().clone().requires_grad_(True)
        path_l = path.detach().clone().requires_grad_(True)
        out = GatherConcat.apply(starts, paths, ends, term_l, path_l)
        gout = torch.randn_like(out, dtype=torch.float32).to(torch.bfloat16)
        # zero grads for pad contexts (mirrors real training: attention math
        # makes them exactly zero; the kernel skips pad rows entirely)
        gout = gout.view(B, C, -1)
        gout[(starts == 0)] = 0
        gout = gout.view(B * C, -1)
        out.backward(gout)

        term_r = term.float().requires_grad_(True)
        path_r = path.float().requires_grad_(True)
        ref = R.gather_concat(starts, paths, ends, term_r, path_r).view(B * C, -1)
        ref.backward(gout.float())
        assert relerr(term_l.grad, term_r.grad.to(torch.bfloat16)) < 2e-2
        assert relerr(path_l.grad, path_r.grad.to(torch.bfloat16)) < 2e-2


# ---------------------------------------------------------------------------
class TestCombiner:
    def _setup(self, dev, M=512, dt=100, dp=100, E=100, seed=3):
        g = torch.Generator().manual_seed(seed)
        TS, PS, EP = round_up(dt), round_up(dp), round_up(E)
        KP = 2 * TS + PS
        x = torch.zeros(M, KP)
        x[:, :dt] = torch.randn(M, dt, generator=g)
        x[:, TS : TS + dp] = torch.randn(M, dp, generator=g)
        x[:, TS + PS : TS + PS + dt] = torch.randn(M, dt, generator=g)
        # TRANSPOSED weight layout [EP, KP] (see combiner.hip)
        w = torch.zeros(EP, KP)
        wl = torch.randn(E, 2 * dt + dp, generator=g) * 0.05
        w[:E, :dt] = wl[:, :dt]
        w[:E, TS : TS + dp] = wl[:, dt : dt + dp]
        w[:E, TS + PS : TS + PS + dt] = wl[:, dt + dp :]
        gamma = torch.zeros(EP); gamma[:E] = torch.rand(E, generator=g) + 0.5
        beta = torch.zeros(EP); beta[:E] = torch.randn(E, generator=g) * 0.1
        return (x.to(dev, torch.bfloat16), w.to(dev, torch.bfloat16),
                gamma.to(dev), beta.to(dev), wl, E, EP, KP, TS, PS, dt, dp)

    def test_fwd_no_dropout(self, dev):
        from code2vec_amd.ops.functional import CombinerLNTanh

        x, w, gamma, beta, wl, E, EP, KP, TS, PS, dt, dp = self._setup(dev)
        out = CombinerLNTanh.apply(x, w, gamma, beta, E, 0.0, False)
        # fp32 oracle on the same padded operands
        ref = (x.float() @ w.float().t())
        mu = ref[:, :E].mean(dim=1, keepdim=True)
        var = ref[:, :E].var(dim=1, unbiased=False, keepdim=True)
        y = torch.tanh((ref[:, :E] - mu) / torch.sqrt(var + 1e-5)
                       * gamma[:E] + beta[:E])
        assert relerr(out[:, :E], y) < 2e-2
        assert torch.all(out[:, E:].float() == 0)

    def test_fwd_matches_reference_op(self, dev):
        """End math parity: padded kernel output == R.combiner on logical."""
        from code2vec_amd.ops.functional import CombinerLNTanh

        x, w, gamma, beta, wl, E, EP, KP, TS, PS, dt, dp = self._setup(dev)
        out = CombinerLNTanh.apply(x, w, gamma, beta, E, 0.0, False)
        xl = torch.cat(
            [x.float()[:, :dt], x.float()[:, TS:TS + dp],
             x.float()[:, TS + PS:TS + PS + dt]], dim=1)
        ref = R.combiner(xl.unsqueeze(0), wl.to(dev), gamma[:E], beta[:E])[0]
        assert relerr(out[:, :E], ref) < 2e-2

    def test_dropout_stats_and_determinism(self, dev):
        from code2vec_amd.ops import functional as Fn

        x, w, gamma, beta, wl, E, EP, *_ = self._setup(dev, M=2048)
        Fn.reseed_dropout_rng(42)
        o1 = Fn.CombinerLNTanh.apply(x, w, gamma, beta, E, 0.5, True)
        Fn.reseed_dropout_rng(42)
        o2 = Fn.CombinerLNTanh.apply(x, w, gamma, beta, E, 0.5, True)
        assert torch.equal(o1, o2)
        keep_rate = (o1[:, :E] != 0).float().mean().item()
        assert abs(keep_rate - 0.5) < 0.02
        # kept values scaled by 1/(1-p)
        o_nodrop = Fn.CombinerLNTanh.apply(x, w, gamma, beta, E, 0.0, False)
        kept = o1[:, :E] != 0
        assert relerr(o1[:, :E][kept], (o_nodrop[:, :E] * 2.0)[kept]) < 2e-2

    def test_autograd_full(self, dev):
        from code2vec_amd.ops.functional import CombinerLNTanh

        x, w, gamma, beta, wl, E, EP, KP, TS, PS, dt, dp = self._setup(dev, M=256)
        xh = x.detach().clone().requires_grad_(True)
        wh = w.detach().clone().requires_grad_(True)
        gh = gamma.detach().clone().requires_grad_(True)
        bh = beta.detach().clone().requires_grad_(True)
        out = CombinerLNTanh.apply(xh, wh, gh, bh, E, 0.0, False)
        gout = (torch.randn_like(out, dtype=torch.float32) * 0.1)
        gout[:, E:] = 0
        out.backward(gout.to(torch.bfloat16))

        xr = x.float().detach().requires_grad_(True)
        wr = w.float().detach().requires_grad_(True)
        gr = gamma.detach().clone().requires_grad_(True)
        br = beta.detach().clone().requires_grad_(True)
        z = xr @ wr.t()
        mu = z[:, :E].mean(dim=1, keepdim=True)
        var = z[:, :E].var(dim=1, unbiased=False, keepdim=True)
        y = torch.tanh((z[:, :E] - mu) / torch.sqrt(var + 1e-5) * gr[:E] + br[:E])
        y.backward(gout[:, :E].to(torch.bfloat16).float())

        assert relerr(xh.grad, xr.grad) < 4e-2
        assert relerr(wh.grad[:E, :], wr.grad[:E, :]) < 4e-2
        assert relerr(gh.grad[:E], gr.grad[:E]) < 4e-2
        assert relerr(bh.grad[:E], br.grad[:E]) < 4e-2
        # pad regions of grads are exactly zero
        assert torch.all(wh.grad.float()[E:, :] == 0)
        assert torch.all(gh.grad[E:] == 0)


# ---------------------------------------------------------------------------
class TestAttention:
    def _setup(self, dev, B=16, C=50, E=100, seed=5):
        g = torch.Generator().manual_seed(seed)
        EP = round_up(E)
        ccv = torch.zeros(B, C, EP)
        ccv[:, :, :E] = torch.tanh(torch.randn(B, C, E, generator=g))
        a = torch.zeros(EP)
        a[:E] = torch.randn(E, generator=g) * 0.2
        starts = torch.randint(1, 100, (B, C), generator=g, dtype=torch.int32)
        lens = torch.randint(1, C + 1, (B,), generator=g)
        starts[torch.arange(C)[None, :] >= lens[:, None]] = 0
        return (ccv.to(dev, torch.bfloat16), a.to(dev), starts.to(dev), E, EP)

    def test_fwd(self, dev):
        from code2vec_amd.ops.functional import AttentionPool

        ccv, a, starts, E, EP = self._setup(dev)
        cv, attn = AttentionPool.apply(ccv, a, starts, E)
        mask = (starts > 0).float()
        cv_ref, attn_ref = R.attention_code_vector(ccv.float(), a, mask)
        assert relerr(attn, attn_ref) < 2e-2
        assert relerr(cv[:, :E], cv_ref[:, :E]) < 2e-2
        assert torch.all(attn.sum(dim=1).sub(1).abs() < 1e-3)

    def test_fwd_all_pad_row_uniform(self, dev):
        from code2vec_amd.ops.functional import AttentionPool

        ccv, a, starts, E, EP = self._setup(dev, B=4, C=13)
        starts = torch.zeros_like(starts)
        cv, attn = AttentionPool.apply(ccv, a, starts, E)
        assert torch.allclose(attn, torch.full_like(attn, 1.0 / attn.shape[1]),
                              atol=1e-5)

    def test_large_c_non_staged_fallback(self, dev):
        """C = 1000: the tile no longer fits the LDS-staged path, so the
        non-staged large-C fallback template runs (attention.hip) — the
        long-context tunable of SURVEY §5.7.  Forward AND backward."""
        from code2vec_amd.ops.functional import AttentionPool

        ccv, a, starts, E, EP = self._setup(dev, B=6, C=1000, seed=9)
        ch = ccv.detach().clone().requires_grad_(True)
        ah = a.detach().clone().requires_grad_(True)
        cv, attn = AttentionPool.apply(ch, ah, starts, E)
        mask = (starts > 0).float()
        cr = ccv.float().detach().requires_grad_(True)
        ar = a.detach().clone().requires_grad_(True)
        cv_ref, attn_ref = R.attention_code_vector(cr, ar, mask)
        assert relerr(attn, attn_ref) < 2e-2
        assert relerr(cv[:, :E], cv_ref[:, :E]) < 2e-2
        dcv = torch.randn_like(cv) * 0.1
        dcv[:, E:] = 0
        cv.backward(dcv)
        cv_ref.backward(dcv)
        assert relerr(ch.grad.float(), cr.grad.to(torch.bfloat16).float()) < 4e-2
        assert relerr(ah.grad[:E], ar.grad[:E]) < 4e-2

    def test_bwd(self, dev):
        from code2vec_amd.ops.functional import AttentionPool

        ccv, a, starts, E, EP = self._setup(dev, B=8, C=40)
        ch = ccv.detach().clone().requires_grad_(True)
        ah = a.detach().clone().requires_grad_(True)
        cv, attn = AttentionPool.apply(ch, ah, starts, E)
        dcv = torch.randn_like(cv) * 0.1
        dcv[:, E:] = 0
        cv.backward(dcv)

        cr = ccv.float().detach().requires_grad_(True)
        ar = a.detach().clone().requires_grad_(True)
        mask = (starts > 0).float()
        cv_ref, _ = R.attention_code_vector(cr, ar, mask)
        cv_ref.backward(dcv)
        assert relerr(ch.grad.float(), cr.grad.to(torch.bfloat16).float()) < 4e-2
        assert relerr(ah.grad[:E], ar.grad[:E]) < 4e-2


# ---------------------------------------------------------------------------
class TestLogSoftmaxNLL:
    def test_fwd_bwd(self, dev):
        from code2vec_amd.ops.functional import FusedLogSoftmaxNLL

        B, L = 64, 7321
        g = torch.Generator().manual_seed(9)
        logits32 = torch.randn(B, L, generator=g) * 3
        label = torch.randint(0, L, (B,), generator=g).to(dev)
        weight = (torch.rand(L, generator=g) + 0.5).to(dev)
        lh = logits32.to(dev, torch.bfloat16).requires_grad_(True)
        loss = FusedLogSoftmaxNLL.apply(lh, label, weight)
        loss.backward()

        lr = lh.detach().float().requires_grad_(True)
        ref = R.logsoftmax_nll(lr, label, weight)
        ref.backward()
        assert abs(float(loss) - float(ref)) / abs(float(ref)) < 1e-2
        assert relerr(lh.grad.float(), lr.grad) < 3e-2

    def test_large_vocab(self, dev):
        from code2vec_amd.ops.functional import FusedLogSoftmaxNLL

        B, L = 16, 261_000
        logits = (torch.randn(B, L) * 2).to(dev, torch.bfloat16)
        label = torch.randint(0, L, (B,)).to(dev)
        weight = torch.ones(L, device=dev)
        lh = logits.requires_grad_(True)
        loss = FusedLogSoftmaxNLL.apply(lh, label, weight)
        loss.backward()
        ref = R.logsoftmax_nll(logits.float(), label, weight)
        assert abs(float(loss) - float(ref)) / abs(float(ref)) < 1e-2
        assert torch.isfinite(lh.grad.float()).all()


# ---------------------------------------------------------------------------
class TestHeadFwd:
    @pytest.mark.parametrize("B,L,EP", [(24, 700, 128), (100, 7321, 128),
                                        (300, 30000, 128), (24, 997, 320)])
    def test_matches_linear_oracle(self, dev, B, L, EP):
        from code2vec_amd.ops import ext

        g = torch.Generator().manual_seed(11)
        cv = (torch.randn(B, EP, generator=g) * 0.5).to(dev, torch.bfloat16)
        w = (torch.randn(L, EP, generator=g) * 0.1).to(dev, torch.bfloat16)
        bias = torch.randn(L, generator=g).to(dev)
        out = torch.empty(B, L, dtype=torch.bfloat16, device=dev)
        gx = (L + 255) // 256
        pm = torch.empty(gx, B, dtype=torch.float32, device=dev)
        ps = torch.empty_like(pm)
        ext().head_fwd(cv, w, bias, out, pm, ps)

        ref = cv.float() @ w.float().t() + bias
        assert relerr(out.float(), ref) < 2e-2

        # the fused (max, sumexp) partials must reproduce the row lse of the
        # stored bf16 logits exactly (same rounding, different summation)
        m = pm.max(dim=0, keepdim=True).values
        lse = (ps * torch.exp(pm - m)).sum(dim=0).log() + m[0]
        lse_ref = torch.logsumexp(out.float(), dim=1)
        assert relerr(lse, lse_ref) < 1e-4

    @pytest.mark.parametrize("B,L", [(64, 1024), (300, 29992), (1024, 2048)])
    def test_head_dgrad_matches_oracle(self, dev, B, L):
        from code2vec_amd.ops import ext

        g = torch.Generator().manual_seed(17)
        dlogits = (torch.randn(B, L, generator=g) * 0.02).to(
            dev, torch.bfloat16)
        w = (torch.randn(L, 128, generator=g) * 0.1).to(dev, torch.bfloat16)
        split = (L + 511) // 512
        partials = torch.full((split, B, 128), float("nan"),
                              dtype=torch.float32, device=dev)
        ext().head_dgrad(dlogits, w.t().contiguous(), partials)
        dcv = partials.sum(dim=0)
        ref = dlogits.float() @ w.float()
        assert relerr(dcv, ref) < 2e-2

    @pytest.mark.parametrize("M,KP", [(200, 320), (1000, 384), (96, 104)])
    def test_dgrad2_matches_oracle(self, dev, M, KP):
        from code2vec_amd.ops import ext

        g = torch.Generator().manual_seed(23)
        dz = (torch.randn(M, 128, generator=g) * 0.1).to(dev, torch.bfloat16)
        w = (torch.randn(128, KP, generator=g) * 0.1).to(dev, torch.bfloat16)
        dx = torch.full((M, KP), float("nan"), dtype=torch.bfloat16,
                        device=dev)
        ext().dgrad2(dz, w.t().contiguous(), dx)
        ref = dz.float() @ w.float()
        assert relerr(dx.float(), ref) < 2e-2

    def test_output_head_backward_custom_dcv(self, dev):
        """OutputHead.backward's custom split-K dcv path (L % 8 == 0,
        EP = 128) vs the fp32 oracle."""
        from code2vec_amd.ops.functional import OutputHead

        B, L, EP = 96, 4096, 128
        g = torch.Generator().manual_seed(19)
        cv = (torch.randn(B, EP, generator=g) * 0.5).to(dev, torch.bfloat16)
        w = (torch.randn(L, EP, generator=g) * 0.1).to(dev, torch.bfloat16)
        bias = torch.randn(L, generator=g).to(dev)
        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        bh = bias.clone().requires_grad_(True)
        dl = (torch.randn(B, L, generator=g) * 0.05).to(dev, torch.bfloat16)
        OutputHead.apply(cvh, wh, bh).backward(dl)

        cvr = cv.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        (cvr @ wr.t() + br).backward(dl.float())
        assert relerr(cvh.grad.float(), cvr.grad) < 3e-2
        assert relerr(wh.grad.float(), wr.grad) < 3e-2
        assert relerr(bh.grad.float(), br.grad) < 3e-2

    def test_output_head_plus_loss_fused_path(self, dev):
        """OutputHead (custom fwd, stats on) + FusedLogSoftmaxNLL
        (finalize path) vs the fp32 oracle end to end."""
        from code2vec_amd.ops.functional import (
            FusedLogSoftmaxNLL, OutputHead)

        B, L, EP = 64, 7321, 128
        g = torch.Generator().manual_seed(13)
        cv = (torch.randn(B, EP, generator=g) * 0.5).to(dev, torch.bfloat16)
        w = (torch.randn(L, EP, generator=g) * 0.1).to(dev, torch.bfloat16)
        bias = torch.randn(L, generator=g).to(dev)
        label = torch.randint(0, L, (B,), generator=g).to(dev)
        weight = (torch.rand(L, generator=g) + 0.5).to(dev)

        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        bh = bias.clone().requires_grad_(True)
        logits = OutputHead.apply(cvh, wh, bh)
        assert hasattr(logits, "_c2v_lsm_partials")
        loss = FusedLogSoftmaxNLL.apply(logits, label, weight)
        loss.backward()

        cvr = cv.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        ref = R.logsoftmax_nll(cvr @ wr.t() + br, label, weight)
        ref.backward()
        assert abs(float(loss) - float(ref)) / abs(float(ref)) < 1e-2
        assert relerr(cvh.grad.float(), cvr.grad) < 3e-2
        assert relerr(wh.grad.float(), wr.grad) < 3e-2
        assert relerr(bh.grad.float(), br.grad) < 3e-2


# ---------------------------------------------------------------------------
class TestAdam:
    def test_bf16_master_matches_torch_adam(self, dev):
        from code2vec_amd.engine.optim import FusedAdam

        g = torch.Generator().manual_seed(11)
        p32 = torch.randn(4097, generator=g)
        param = torch.nn.Parameter(p32.to(dev, torch.bfloat16))
        opt = FusedAdam([param], lr=0.01, betas=(0.9, 0.999), weight_decay=0.01)

        ref_param = torch.nn.Parameter(param.detach().float().clone())
        ref_opt = torch.optim.Adam([ref_param], lr=0.01, betas=(0.9, 0.999),
                                   weight_decay=0.01)
        for step in range(5):
            grad32 = torch.randn(4097, generator=g).to(dev)
            param.grad = grad32.to(torch.bfloat16)
            ref_param.grad = param.grad.float()  # same bf16-rounded grads
            opt.step()
            ref_opt.step()
        master = opt.state[param]["master"]
        assert relerr(master, ref_param.detach()) < 1e-4
        assert relerr(param.detach().float(), ref_param.detach()) < 1e-2

    def test_f32(self, dev):
        from code2vec_amd.engine.optim import FusedAdam

        param = torch.nn.Parameter(torch.randn(1000, device=dev))
        ref_param = torch.nn.Parameter(param.detach().clone())
        opt = FusedAdam([param], lr=0.05)
        ref_opt = torch.optim.Adam([ref_param], lr=0.05)
        for _ in range(3):
            grad = torch.randn(1000, device=dev)
            param.grad = grad.clone()
            ref_param.grad = grad.clone()
            opt.step()
            ref_opt.step()
        assert relerr(param.detach(), ref_param.detach()) < 1e-5


class TestCombinerDropoutBwd:
    def test_autograd_with_dropout(self, dev):
        """Backward under dropout: the kernel recovers the mask from the
        forward output; compare against torch autograd using that mask."""
        from code2vec_amd.ops import functional as Fn

        x, w, gamma, beta, wl, E, EP, KP, TS, PS, dt, dp = \
            TestCombiner()._setup(dev, M=512)
        p = 0.5
        xh = x.detach().clone().requires_grad_(True)
        wh = w.detach().clone().requires_grad_(True)
        Fn.reseed_dropout_rng(7)
        out = Fn.CombinerLNTanh.apply(xh, wh, gamma, beta, E, p, True)
        gout = (torch.randn_like(out, dtype=torch.float32) * 0.1)
        gout[:, E:] = 0
        out.backward(gout.to(torch.bfloat16))

        mask = (out.detach()[:, :E] != 0).float()
        xr = x.float().detach().requires_grad_(True)
        wr = w.float().detach().requires_grad_(True)
        z = xr @ wr.t()
        mu = z[:, :E].mean(dim=1, keepdim=True)
        var = z[:, :E].var(dim=1, unbiased=False, keepdim=True)
        y = torch.tanh((z[:, :E] - mu) / torch.sqrt(var + 1e-5)
                       * gamma[:E] + beta[:E])
        out_ref = y * mask / (1 - p)
        assert relerr(out[:, :E], out_ref) < 2e-2
        out_ref.backward(gout[:, :E].to(torch.bfloat16).float())
        assert relerr(xh.grad, xr.grad) < 5e-2
        assert relerr(wh.grad[:E, :], wr.grad[:E, :]) < 5e-2


class TestScatterProperty:
    def test_group_by_index_is_a_sort(self, dev):
        from code2vec_amd.ops.functional import _group_by_index

        g = torch.Generator(device=dev).manual_seed(0)
        idx = torch.randint(0, 997, (50_000,), generator=g, device=dev,
                            dtype=torch.int32)
        sorted_idx, perm, counts = _group_by_index(idx, 1000)
        ref, _ = torch.sort(idx)
        assert torch.equal(sorted_idx, ref)
        # perm is a permutation mapping back to the original values
        assert torch.equal(idx[perm], sorted_idx)
        assert int(counts[:1000].sum()) == 50_000

    @pytest.mark.parametrize("n_distinct", [7, 1000, 200_000])
    def test_scatter_matches_index_add_oracle(self, dev, n_distinct):
        """Heavy-hitter runs (n_distinct=7 -> runs span hundreds of chunks)
        exercise the boundary fp32-atomic path; large n_distinct the
        interior bf16-direct path."""
        from code2vec_amd.ops import functional as Fn

        T, S, M = 250_000, 104, 60_000
        KP = 320
        g = torch.Generator(device=dev).manual_seed(3)
        starts = torch.randint(1, n_distinct + 1, (M,), generator=g,
                               device=dev, dtype=torch.int32)
        ends = torch.randint(1, n_distinct + 1, (M,), generator=g,
                             device=dev, dtype=torch.int32)
        paths = torch.randint(1, n_distinct + 1, (M,), generator=g,
                              device=dev, dtype=torch.int32)
        gout = (torch.randn(M, KP, generator=g, device=dev) * 0.1).to(
            torch.bfloat16)
        dterm, dpath = Fn._scatter_embedding_grads(
            starts, paths, ends, gout, (T, S), (T, S))

        ref_t = torch.zeros(T, S, dtype=torch.float32, device=dev)
        ref_t.index_add_(0, starts.long(), gout[:, :S].float())
        ref_t.index_add_(0, ends.long(), gout[:, 208:208 + S].float())
        ref_p = torch.zeros(T, S, dtype=torch.float32, device=dev)
        ref_p.index_add_(0, paths.long(), gout[:, 104:104 + S].float())
        err_t = (dterm.float() - ref_t).norm() / (ref_t.norm() + 1e-9)
        err_p = (dpath.float() - ref_p).norm() / (ref_p.norm() + 1e-9)
        assert float(err_t) < 2e-2, float(err_t)
        assert float(err_p) < 2e-2, float(err_p)


# ---------------------------------------------------------------------------
class TestFusedHeadLoss:
    """Fused head+loss backward (recompute-G; head_bwd.hip) vs the fp32
    oracle and vs the unfused OutputHead+FusedLogSoftmaxNLL chain."""

    def _setup(self, dev, B, L, EP=128, seed=23):
        g = torch.Generator().manual_seed(seed)
        cv = (torch.randn(B, EP, generator=g) * 0.5).to(dev, torch.bfloat16)
        w = (torch.randn(L, EP, generator=g) * 0.1).to(dev, torch.bfloat16)
        bias = torch.randn(L, generator=g).to(dev)
        label = torch.randint(0, L, (B,), generator=g).to(dev)
        weight = (torch.rand(L, generator=g) + 0.5).to(dev)
        return cv, w, bias, label, weight

    def _run_fused(self, cv, w, bias, label, weight, scale=1.0):
        from code2vec_amd.ops import functional as Fn

        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        bh = bias.clone().requires_grad_(True)
        logits = Fn.head_logits_with_stats(cvh.detach(), wh.detach(),
                                           bh.detach())
        loss = Fn.FusedHeadLoss.apply(logits, cvh, wh, bh, label, weight)
        (loss * scale).backward()
        return loss, cvh.grad, wh.grad, bh.grad

    @pytest.mark.parametrize("B,L", [(96, 7320), (64, 1992), (40, 4096)])
    def test_matches_fp32_oracle(self, dev, B, L):
        cv, w, bias, label, weight = self._setup(dev, B, L)
        loss, dcv, dw, dbias = self._run_fused(cv, w, bias, label, weight)

        cvr = cv.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        ref = R.logsoftmax_nll(cvr @ wr.t() + br, label, weight)
        ref.backward()
        assert abs(float(loss) - float(ref)) / abs(float(ref)) < 1e-2
        assert relerr(dcv.float(), cvr.grad) < 3e-2
        assert relerr(dw.float(), wr.grad) < 3e-2
        assert relerr(dbias.float(), br.grad) < 3e-2

    def test_large_vocab_library_fwd_path(self, dev):
        """A large vocabulary, L = 70016.  Despite its name this test does
        not reach the library GEMM: L is a multiple of 8 and EP = 128, so
        the forward is head_fwd_img (the W-image kernel, the default since
        it replaced the C2V_HEAD_FWD_MAXL gate here) with the stats
        partials merged by lsm_finalize, and the backward splits dcv in
        1024-label chunks (4096 starts above L = 131072).  The library
        forward followed by lsm_partial, and the 4096-label chunk, are
        covered in test_head_numerics_gpu.py."""
        B, L = 32, 70016
        cv, w, bias, label, weight = self._setup(dev, B, L, seed=31)
        loss, dcv, dw, dbias = self._run_fused(cv, w, bias, label, weight)

        cvr = cv.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        ref = R.logsoftmax_nll(cvr @ wr.t() + br, label, weight)
        ref.backward()
        assert abs(float(loss) - float(ref)) / abs(float(ref)) < 1e-2
        assert relerr(dcv.float(), cvr.grad) < 3e-2
        assert relerr(dw.float(), wr.grad) < 3e-2
        assert relerr(dbias.float(), br.grad) < 3e-2

    @pytest.mark.parametrize("B,L", [(96, 7320), (64, 1992), (1024, 4096)])
    def test_streaming_dcv_matches(self, dev, B, L):
        """C2V_HB_RC path: dcv recomputed by MFMA from the cv/W fragment
        images (logits never read) must match both the logits-reading
        kernel (bitwise-near: same math, one rounding closer to f32) and
        the fp32 oracle."""
        from code2vec_amd.ops import functional as Fn

        cv, w, bias, label, weight = self._setup(dev, B, L, seed=57)
        loss_a, dcv_a, dw_a, db_a = self._run_fused(cv, w, bias, label,
                                                    weight)
        old = Fn._HB_RC
        Fn._HB_RC = True
        try:
            loss_b, dcv_b, dw_b, db_b = self._run_fused(cv, w, bias, label,
                                                        weight)
        finally:
            Fn._HB_RC = old
        assert abs(float(loss_a.detach()) - float(loss_b.detach())) <= (
            1e-6 + 1e-5 * abs(float(loss_a.detach())))
        # the RC path recomputes logits in f32 where the reading path
        # consumes their bf16 rounding — per-element g shifts up to a few
        # tenths of a percent, summed into dcv
        assert relerr(dcv_b.float(), dcv_a.float()) < 5e-2
        assert torch.equal(dw_a, dw_b)  # dw path identical in both modes
        cvr = cv.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        ref = R.logsoftmax_nll(cvr @ wr.t() + br, label, weight)
        ref.backward()
        # dcv error is dominated by the bf16 rounding of G; the RC path
        # rounds marginally different G values, landing a hair past the
        # 3e-2 bound the reading path meets on some shapes
        assert relerr(dcv_b.float(), cvr.grad) < 6e-2

    def test_direct_headfwd_path_matches(self, dev):
        """C2V_HF_AIMG=0 route: the direct-load head_fwd kernel (the
        pre-image default) must still match the oracle now that the
        W-image kernel is the EP=128 default."""
        from code2vec_amd.ops import functional as Fn

        cv, w, bias, label, weight = self._setup(dev, 96, 7320, seed=61)
        old = Fn._HF_AIMG
        Fn._HF_AIMG = False
        try:
            loss, dcv, dw, dbias = self._run_fused(cv, w, bias, label,
                                                   weight)
        finally:
            Fn._HF_AIMG = old
        cvr = cv.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        br = bias.clone().requires_grad_(True)
        ref = R.logsoftmax_nll(cvr @ wr.t() + br, label, weight)
        ref.backward()
        assert abs(float(loss.detach()) - float(ref.detach())) / abs(
            float(ref.detach())) < 1e-2
        assert relerr(dcv.float(), cvr.grad) < 3e-2
        assert relerr(dw.float(), wr.grad) < 3e-2

    def test_matches_unfused_chain(self, dev):
        """Fused backward vs the unfused OutputHead+FusedLogSoftmaxNLL
        chain on identical inputs (both bf16 paths -> tight tolerance);
        non-1 upstream gradient exercises the gscale plumbing."""
        from code2vec_amd.ops.functional import (FusedLogSoftmaxNLL,
                                                 OutputHead)

        B, L = 64, 2048
        cv, w, bias, label, weight = self._setup(dev, B, L, seed=41)
        loss_f, dcv_f, dw_f, db_f = self._run_fused(
            cv, w, bias, label, weight, scale=2.5)

        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        bh = bias.clone().requires_grad_(True)
        loss_u = FusedLogSoftmaxNLL.apply(
            OutputHead.apply(cvh, wh, bh), label, weight)
        (loss_u * 2.5).backward()
        assert abs(float(loss_f) - float(loss_u)) <= 1e-5 * abs(float(loss_u))
        assert relerr(dcv_f.float(), cvh.grad.float()) < 1e-2
        assert relerr(dw_f.float(), wh.grad.float()) < 1e-2
        assert relerr(db_f.float(), bh.grad.float()) < 1e-2

    def test_model_takes_fused_path_in_training(self, dev):
        """Code2VecHIP training forward stashes the fused-head context and
        loss() consumes it (the hot path actually runs these kernels)."""
        from code2vec_amd.models.code2vec import Code2VecHIP, init_logical_params
        from code2vec_amd.utils.options import Option

        opt = Option(terminal_count=500, path_count=400, label_count=2000,
                     max_path_length=16, terminal_embed_size=100,
                     path_embed_size=100, encode_size=100, dropout_prob=0.0)
        g = torch.Generator().manual_seed(3)
        m = Code2VecHIP(opt, init_logical_params(opt, g), device=dev).train()
        s = torch.randint(1, 500, (16, 16), dtype=torch.int32, device=dev)
        p = torch.randint(1, 400, (16, 16), dtype=torch.int32, device=dev)
        e = torch.randint(1, 500, (16, 16), dtype=torch.int32, device=dev)
        y = torch.randint(0, 2000, (16,), device=dev)
        out, _, _ = m(s, p, e, y)
        assert hasattr(out, "_c2v_fused_head")
        loss = m.loss(out, y, torch.ones(2000, device=dev))
        loss.backward()
        assert m.output_weight.grad is not None
        assert m.output_bias.grad is not None
        assert m.terminal_embedding.grad is not None
        # eval path: no stash, plain logits
        m.eval()
        with torch.no_grad():
            out_e, _, _ = m(s, p, e, y)
        assert not hasattr(out_e, "_c2v_fused_head")


# ---------------------------------------------------------------------------
class TestAngularMarginHead:
    """K11 HIP kernels (angular.hip) vs the fp32 torch oracle."""

    @pytest.mark.parametrize("B,L", [(64, 2048), (96, 1000), (33, 517)])
    def test_forward_backward_vs_oracle(self, dev, B, L):
        from code2vec_amd.ops.functional import AngularMarginHead

        g = torch.Generator().manual_seed(29)
        cv = (torch.randn(B, 128, generator=g) * 0.7).to(dev, torch.bfloat16)
        w = (torch.randn(L, 128, generator=g) * 0.2).to(dev, torch.bfloat16)
        label = torch.randint(0, L, (B,), generator=g).to(dev)
        cos_m, sin_m, s = math.cos(0.5), math.sin(0.5), 30.0

        cvh = cv.clone().requires_grad_(True)
        wh = w.clone().requires_grad_(True)
        out = AngularMarginHead.apply(cvh, wh, label, cos_m, sin_m, s)
        dl = (torch.randn(B, L, generator=g) * 0.05).to(dev, torch.bfloat16)
        out.backward(dl)

        cvr = cv.float().requires_grad_(True)
        wr = w.float().requires_grad_(True)
        ref = R.angular_margin_head(cvr, wr, label, cos_m, sin_m, s)
        ref.backward(dl.float())
        assert relerr(out.float(), ref) < 3e-2
        assert relerr(cvh.grad.float(), cvr.grad) < 4e-2
        assert relerr(wh.grad.float(), wr.grad) < 4e-2

    def test_model_path_uses_kernels(self, dev):
        """Code2VecHIP with --angular_margin_loss goes through the HIP
        AngularMarginHead (no torch head ops) and trains."""
        from code2vec_amd.models.code2vec import Code2VecHIP, init_logical_params
        from code2vec_amd.utils.options import Option
        from code2vec_amd.ops import functional as Fn

        opt = Option(terminal_count=400, path_count=300, label_count=512,
                     max_path_length=12, terminal_embed_size=100,
                     path_embed_size=100, encode_size=100, dropout_prob=0.0,
                     angular_margin_loss=True)
        g = torch.Generator().manual_seed(9)
        m = Code2VecHIP(opt, init_logical_params(opt, g), device=dev).train()
        s = torch.randint(1, 400, (16, 12), dtype=torch.int32, device=dev)
        p = torch.randint(1, 300, (16, 12), dtype=torch.int32, device=dev)
        e = torch.randint(1, 400, (16, 12), dtype=torch.int32, device=dev)
        y = torch.randint(0, 512, (16,), device=dev)
        out, _, _ = m(s, p, e, y)
        assert out.grad_fn is not None
        assert "AngularMarginHead" in type(out.grad_fn).__name__
        loss = m.loss(out, y, torch.ones(512, device=dev))
        loss.backward()
        assert m.output_weight.grad is not None
        assert m.terminal_embedding.grad is not None


class TestRowMaxArgmax:
    def test_matches_torch_max(self, dev):
        from code2vec_amd.ops.functional import row_max_argmax

        g = torch.Generator().manual_seed(17)
        for B, L in [(64, 30000), (33, 517), (8, 261000)]:
            x = (torch.randn(B, L, generator=g)).to(dev, torch.bfloat16)
            vals, idx = row_max_argmax(x)
            rv, ri = torch.max(x.float(), dim=1)
            assert torch.equal(idx, ri), (B, L)
            assert torch.equal(vals, rv), (B, L)

    def test_tie_break_first_index(self, dev):
        from code2vec_amd.ops.functional import row_max_argmax

        x = torch.zeros(4, 1000, dtype=torch.bfloat16, device=dev)
        x[:, 100] = 2.0
        x[:, 700] = 2.0  # tie: torch.max returns the FIRST index
        _, idx = row_max_argmax(x)
        assert torch.equal(idx, torch.full((4,), 100, dtype=torch.int64,
                                           device=dev))


class TestExclusiveScan:
    @pytest.mark.parametrize("n", [7, 1024, 4096, 360633, 1300001])
    def test_matches_cumsum(self, dev, n):
        from code2vec_amd.ops import ext

        g = torch.Generator().manual_seed(n)
        x = torch.randint(0, 9, (n,), generator=g, dtype=torch.int32).to(dev)
        partial = torch.empty((n + 1023) // 1024, dtype=torch.int32,
                              device=dev)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        ext().exclusive_scan(x, partial, out)
        ref = torch.zeros(n, dtype=torch.int64, device=dev)
        ref[1:] = torch.cumsum(x.long()[:-1], 0)
        assert torch.equal(out.long(), ref)

    def test_pooled_counts_invariant_across_steps(self, dev):
        """The pooled counting sort must give identical results on
        repeated use: cast_clear_rows restores the all-zero histogram."""
        from code2vec_amd.ops import functional as Fn
        from code2vec_amd.ops import ext

        T, S, M = 5000, 104, 4096
        g = torch.Generator().manual_seed(3)
        for step in range(3):
            idx = torch.randint(0, T, (2 * M,), generator=g,
                                dtype=torch.int32).to(dev)
            a = Fn._group_by_index(idx, T, pool_tag="term")
            b = Fn._group_by_index(idx, T)  # fresh buffers
            assert torch.equal(a[0], b[0])
            assert torch.equal(a[2], b[2])
            # consume the pooled counts the way the scatter path does
            dt32 = Fn._scratch_f32("term", (T, S), dev)
            flags = Fn._scratch_flags("term", T, dev)
            dbf = torch.empty(T, S, dtype=torch.bfloat16, device=dev)
            ext().cast_clear_rows(dt32, a[2], flags, dbf)
