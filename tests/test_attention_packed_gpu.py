"""K21 (attention_packed.hip) under the elementwise fp64 rule of
tests/encoder_numerics.py, and its batch-composition invariance, bit for
bit.

One packed batch per (E, EP) holds a single-PAD method and every length at
which the kernel changes behaviour: 1, 2, the 16-row group step, the 64-row
wave step, the 200/201 limit of the streaming kernels, the LDS score chunk
(ATTN_PACKED_CHUNK = 256) at -1/0/+1, and methods far past it whose scores
are parked in the attn output.  Each method is judged on its own rows by
``attention_fwd_ref`` (the bounds scale with the method's length; none is
added here).  Outputs are NaN-filled before every launch and everything is
run twice.  Run with -s to see max |err| / tol per output.
"""

import pytest
import torch

import encoder_numerics as N
from code2vec_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
f32 = torch.float32
NAN = float("nan")

# the first method is a single PAD context (starts = 0)
LENGTHS = (1, 1, 2, 15, 16, 17, 63, 64, 65, 199, 200, 201, 255, 256, 257,
           1000, 4097, 20000)
EEP = ((100, 128), (20, 32), (300, 320))
INVARIANT = (1, 17, 200, 257, 4097)

assert all(Fn.ATTN_PACKED_CHUNK + k in LENGTHS for k in (-1, 0, 1))


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


class PackedCase:
    """Seeded packed inputs in the style of AttentionCase, on the CPU: ccv
    [M, EP] bf16 (pad columns 0), a [EP] fp32, starts [M] int32.  Methods
    of 2 rows and more carry dominant contexts (score 16, the rest at least
    10 below, rows that differ) at positions 0, 63, 64 and n-1 where they
    exist; methods of 15 rows and more have row n // 2 masked."""

    def __init__(self, E: int, EP: int):
        g = torch.Generator().manual_seed(7919 * E + EP)
        M = sum(LENGTHS)
        ccv = torch.zeros(M, EP)
        ccv[:, :E] = torch.tanh(torch.randn(M, E, generator=g))
        a = torch.zeros(EP)
        a[:E] = torch.randn(E, generator=g) * 0.2
        starts = torch.randint(1, 100, (M,), generator=g, dtype=torch.int32)
        spike = 16.0 * a / float(a.double() @ a.double())
        self.segs = []
        lo = 0
        for i, n in enumerate(LENGTHS):
            self.segs.append((lo, lo + n))
            if i == 0:
                starts[lo] = 0
            if n >= 2:
                for c in sorted({0, min(63, n - 1), min(64, n - 1), n - 1}):
                    noise = torch.zeros(EP)
                    noise[:E] = torch.randn(E, generator=g) * 0.5
                    ccv[lo + c] = (spike + noise
                                   - float(noise @ a) / float(a @ a) * a)
            if n >= 15:
                starts[lo + n // 2] = 0
            lo += n
        self.E, self.EP, self.M = E, EP, M
        self.ccv, self.a, self.starts = ccv.to(bf16), a, starts

    def seg_of(self, n: int):
        return self.segs[len(LENGTHS) - 1 - LENGTHS[::-1].index(n)]


_CASES = {}


def packed_case(E, EP) -> PackedCase:
    if (E, EP) not in _CASES:
        _CASES[(E, EP)] = PackedCase(E, EP)
    return _CASES[(E, EP)]


def run(ccv, a, starts, lengths, E, dev):
    """One launch into NaN-filled outputs."""
    M, EP = ccv.shape
    B = len(lengths)
    out = (torch.full((B, EP), NAN, dtype=f32, device=dev),
           torch.full((B, EP), NAN, dtype=bf16, device=dev),
           torch.full((M,), NAN, dtype=f32, device=dev))
    cv, cvb, attn = Fn.attention_pool_packed(ccv, a, starts, list(lengths),
                                             E, out=out)
    torch.cuda.synchronize()
    return dict(cv=cv, cvb=cvb, attn=attn)


def same_bits(x, y):
    if x.dtype == bf16:
        return torch.equal(x.view(torch.int16), y.view(torch.int16))
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def twice(fn):
    o1, o2 = fn(), fn()
    for k in o1:
        assert same_bits(o1[k], o2[k]), f"{k}: two runs differ"
    return o1


@pytest.mark.parametrize("E,EP", EEP)
def test_packed_pool_within_fp64_bounds(dev, E, EP):
    c = packed_case(E, EP)
    ccv, a, starts = c.ccv.to(dev), c.a.to(dev), c.starts.to(dev)
    o = twice(lambda: run(ccv, a, starts, LENGTHS, E, dev))
    got = {k: v.cpu() for k, v in o.items()}
    for b, (lo, hi) in enumerate(c.segs):
        n = hi - lo
        where = f"({E},{EP}) method {b} n={n}"
        r = N.attention_fwd_ref(c.ccv[lo:hi][None], c.a,
                                c.starts[lo:hi][None], E)
        N.check(got["attn"][lo:hi][None], *r["attn"], "attn (packed)", where)
        N.check(got["cv"][b][None], *r["cv"], "cv (packed)", where)
        N.check(got["cvb"][b][None], *r["cvb"], "cvb (packed)", where)
    ts = min(N.round8(E), EP)
    assert bool((got["cv"][:, ts:] == 0).all())
    assert bool((got["cvb"][:, ts:] == 0).all())
    # one masked row: softmax over a single NINF is weight 1
    assert float(got["attn"][0]) == 1.0
    for lo, hi in c.segs:
        if hi - lo >= 15:
            assert float(got["attn"][lo + (hi - lo) // 2]) == 0.0


@pytest.mark.parametrize("E,EP", EEP)
def test_batch_composition_invariance_bitwise(dev, E, EP):
    c = packed_case(E, EP)
    a = c.a.to(dev)
    whole = run(c.ccv.to(dev), a, c.starts.to(dev), LENGTHS, E, dev)

    def batch(ns):
        rows = [c.seg_of(n) for n in ns]
        ccv = torch.cat([c.ccv[lo:hi] for lo, hi in rows]).to(dev)
        st = torch.cat([c.starts[lo:hi] for lo, hi in rows]).to(dev)
        return run(ccv, a, st, ns, E, dev)

    def method(o, ns, i):
        lo = sum(ns[:i])
        return dict(attn=o["attn"][lo:lo + ns[i]], cv=o["cv"][i],
                    cvb=o["cvb"][i])

    for n in INVARIANT:
        alone = method(batch([n]), [n], 0)
        ways = {
            "first": ([n, 65, 1000], 0),
            "last": ([1000, 2, 65, n], 3),
            "after the 20000-row method": ([63, 20000, n, 256], 2),
            "whole": (list(LENGTHS), len(LENGTHS) - 1
                      - LENGTHS[::-1].index(n)),
        }
        for name, (ns, i) in ways.items():
            o = whole if name == "whole" else batch(ns)
            got = method(o, ns, i)
            for k in ("attn", "cv", "cvb"):
                assert same_bits(got[k], alone[k]), (n, name, k)


def test_binding_rejects_bad_arguments(dev):
    c = packed_case(20, 32)
    ccv, a, starts = c.ccv[:10].to(dev), c.a.to(dev), c.starts[:10].to(dev)
    for bad in ([5, 0, 5], [4, 5], [11]):
        with pytest.raises(ValueError):
            Fn.attention_pool_packed(ccv, a, starts, bad, 20)
    with pytest.raises(RuntimeError):      # f32 rows
        Fn.attention_pool_packed(ccv.float(), a, starts, [10], 20)
    with pytest.raises(RuntimeError):      # non-contiguous rows
        Fn.attention_pool_packed(c.ccv[:20].to(dev)[::2], a, starts, [10], 20)
    with pytest.raises(RuntimeError):      # starts dtype
        Fn.attention_pool_packed(ccv, a, starts.long(), [10], 20)
    with pytest.raises(RuntimeError):      # a of another width
        Fn.attention_pool_packed(ccv, a[:16].contiguous(), starts, [10], 20)
    with pytest.raises(RuntimeError):      # output buffer of another shape
        out = (torch.empty(3, 32, device=dev),
               torch.empty(2, 32, dtype=bf16, device=dev),
               torch.empty(10, device=dev))
        Fn.attention_pool_packed(ccv, a, starts, [4, 6], 20, out=out)
