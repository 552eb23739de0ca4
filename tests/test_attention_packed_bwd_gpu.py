"""K22, the segmented attention backward over a packed batch, and the packed
modes of the recomputing combiner backward, under the elementwise fp64 rule
of tests/encoder_numerics.py (its attention-backward and recompute references
and bounds, applied per method with C = the method's length).

Every output is allocated NaN-filled (seg: -1), every launch runs twice and
the runs are compared bit for bit.  Run with -s to see max |err| / tol.
"""

import pytest
import torch

import encoder_numerics as N
from code2vec_amd.ops import functional as Fn

pytestmark = pytest.mark.gpu

bf16, f32, i32 = torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")
CHUNK = Fn.ATTN_PACKED_CHUNK

# around the 16-row group stride, the 64-row prefetch round, the LDS chunk
# (256) and far past it (one block walks 5,000 rows)
LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 5000)
EEP = ((20, 32), (100, 128), (300, 320))
ALL_MASKED = 2                 # the method of length 15
HOLES = {4: (5,), 8: (0, 100, 254), 10: (256,), 11: (999,), 12: (17, 4999)}
BIG = LENGTHS.index(5000)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def ext():
    from code2vec_amd.ops import ext as _ext
    return _ext()


def nans(shape, dtype, dev):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def same_bits(a, b):
    if a.dtype == bf16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def twice(fn):
    r1, r2 = fn(), fn()
    for k in r1:
        assert same_bits(r1[k], r2[k]), f"{k}: run-to-run bits differ"
    return r1


def offsets_of(lengths, dev):
    off = torch.zeros(len(lengths) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lengths), 0)
    return off.to(i32).to(dev)


_RAGGED = {}


def ragged_case(E, EP):
    """Seeded CPU inputs of the ragged batch: ccv [M, EP] bf16 (pad columns
    0), a, starts [M] (masked rows inside methods, one all-masked method),
    dcv [B, EP] f32, dattn [M]."""
    if (E, EP) in _RAGGED:
        return _RAGGED[(E, EP)]
    g = torch.Generator().manual_seed(1009 * EP + E)
    M, B = sum(LENGTHS), len(LENGTHS)
    ccv = torch.zeros(M, EP)
    ccv[:, :E] = torch.tanh(torch.randn(M, E, generator=g))
    a = torch.zeros(EP)
    a[:E] = torch.randn(E, generator=g) * 0.2
    starts = torch.randint(1, 100, (M,), generator=g, dtype=i32)
    lo = [0]
    for n in LENGTHS:
        lo.append(lo[-1] + n)
    starts[lo[ALL_MASKED]:lo[ALL_MASKED + 1]] = 0
    for b, rows in HOLES.items():
        for r in rows:
            assert r < LENGTHS[b]
            starts[lo[b] + r] = 0
    dcv = torch.zeros(B, EP)
    dcv[:, :E] = torch.randn(B, E, generator=g) * 0.1
    dattn = torch.randn(M, generator=g) * 0.1
    c = dict(ccv=ccv.to(bf16), a=a, starts=starts, dcv=dcv, dattn=dattn,
             lo=lo, M=M, B=B)
    _RAGGED[(E, EP)] = c
    return c


def forward_attn(ccv, a, starts, lengths, E):
    return Fn.attention_pool_packed(ccv, a, starts, list(lengths), E)[2]


def run_k22(dcv, dattn, ccv, a, starts, off, attn, E, compact):
    """One K22 launch into NaN-filled outputs."""
    M, EP = ccv.shape
    B = off.numel() - 1
    dev = ccv.device
    has = dattn is not None
    da_ = dattn if has else torch.empty(0, dtype=f32, device=dev)
    o = dict(ds=nans((M,), f32, dev), da_p=nans((B, EP), f32, dev))
    if compact:
        o["seg"] = torch.full((M,), -1, dtype=i32, device=dev)
        ext().attention_packed_bwd_compact(dcv, da_, ccv, a, starts, off,
                                           attn, o["ds"], o["seg"], o["da_p"],
                                           E, has, CHUNK)
    else:
        o["dccv"] = nans((M, EP), bf16, dev)
        ext().attention_packed_bwd(dcv, da_, ccv, a, starts, off, attn,
                                   o["dccv"], o["ds"], o["da_p"], E, has,
                                   CHUNK)
        del o["ds"]  # a workspace in the dense form
    return o


def per_method_ref(c, dcv, dattn, attn, E):
    """attention_bwd_ref per method (B = 1, C = n), concatenated."""
    ds, dccv, dap = [], [], []
    for b, n in enumerate(LENGTHS):
        s = slice(c["lo"][b], c["lo"][b + 1])
        r = N.attention_bwd_ref(
            dcv[b:b + 1], None if dattn is None else dattn[s][None],
            c["ccv"][s][None], c["a"], c["starts"][s][None], attn[s][None], E)
        ds.append(r["ds"])
        dccv.append(r["dccv"])
        dap.append(r["da_part"])

    def cat(parts, dim):
        return (torch.cat([p[0] for p in parts], dim),
                torch.cat([p[1] for p in parts], dim))
    return cat(ds, 1), cat(dccv, 1), cat(dap, 0)


@pytest.mark.parametrize("E,EP", EEP)
def test_ragged_batch_fp64_rule(dev, E, EP):
    c = ragged_case(E, EP)
    t = {k: c[k].to(dev) for k in ("ccv", "a", "starts", "dcv", "dattn")}
    off = offsets_of(LENGTHS, dev)
    attn = forward_attn(t["ccv"], t["a"], t["starts"], LENGTHS, E)
    attn_c = attn.cpu()
    seg_ref = torch.repeat_interleave(torch.arange(c["B"]),
                                      torch.tensor(LENGTHS)).to(i32)
    for dcv_bf16 in (False, True):
        dcv = t["dcv"].to(bf16) if dcv_bf16 else t["dcv"]
        for has_dattn in (True, False):
            dattn = t["dattn"] if has_dattn else None
            tag = f"({E},{EP}) dcv_bf16={dcv_bf16} dattn={has_dattn}"
            ds, dccv, dap = per_method_ref(
                c, dcv.cpu(), c["dattn"] if has_dattn else None, attn_c, E)
            oc = twice(lambda: run_k22(dcv, dattn, t["ccv"], t["a"],
                                       t["starts"], off, attn, E, True))
            N.check(oc["ds"][None], *ds, "ds (K22 compact)", tag)
            N.check(oc["da_p"], *dap, "da_part (K22 compact)", tag)
            assert torch.equal(oc["seg"].cpu(), seg_ref)
            od = twice(lambda: run_k22(dcv, dattn, t["ccv"], t["a"],
                                       t["starts"], off, attn, E, False))
            N.check(od["dccv"][None], *dccv, "dccv (K22 dense)", tag)
            N.check(od["da_p"], *dap, "da_part (K22 dense)", tag)
            assert same_bits(od["da_p"], oc["da_p"])
            # pad columns exactly zero, masked rows' ds exactly zero
            ts = min(N.round8(E), EP)
            assert int((od["dccv"][:, ts:] != 0).sum()) == 0
            assert int((oc["ds"][t["starts"] == 0] != 0).sum()) == 0


@pytest.mark.parametrize("E,EP", EEP)
def test_composition_invariance(dev, E, EP):
    """A method's ds slice and da_p row depend on its own rows only: alone,
    first, last, right after the 5,000-row method, in the whole batch."""
    c = ragged_case(E, EP)
    t = {k: c[k].to(dev) for k in ("ccv", "a", "starts", "dcv", "dattn")}
    B = c["B"]

    def run(order):
        rows = torch.cat([torch.arange(c["lo"][b], c["lo"][b + 1])
                          for b in order]).to(dev)
        lens = [LENGTHS[b] for b in order]
        ccv = t["ccv"][rows].contiguous()
        st = t["starts"][rows].contiguous()
        sel = torch.tensor(order, device=dev)
        attn = forward_attn(ccv, t["a"], st, lens, E)
        o = run_k22(t["dcv"][sel].contiguous(), t["dattn"][rows].contiguous(),
                    ccv, t["a"], st, offsets_of(lens, dev), attn, E, True)
        out, lo = {}, 0
        for i, b in enumerate(order):
            out[b] = (o["ds"][lo:lo + lens[i]].clone(), o["da_p"][i].clone(),
                      attn[lo:lo + lens[i]].clone())
            lo += lens[i]
        return out

    whole = run(list(range(B)))
    for m in range(B):
        rest = [b for b in range(B) if b != m]
        small = [b for b in rest if b != BIG]
        orders = [[m], [m] + rest, rest + [m]]
        if m != BIG:
            orders.append(small[:3] + [BIG, m] + small[3:])
        for order in orders:
            got = run(order)[m]
            for k, name in enumerate(("ds", "da_p", "attn")):
                assert same_bits(got[k], whole[m][k]), (m, order[:4], name)


@pytest.mark.parametrize("C", [50, 200, 201])
@pytest.mark.parametrize("E,EP", [(100, 128), (300, 320)])
def test_equal_lengths_have_the_padded_kernels_bits(dev, C, E, EP):
    B = 5
    c = N.attention_case(B, C, E, EP)
    ccv, a, starts = c.ccv.to(dev), c.a.to(dev), c.starts.to(dev)
    cv = nans((B, EP), f32, dev)
    attn = nans((B, C), f32, dev)
    ext().attention_fwd(ccv, a, starts, cv, attn, E)
    off = offsets_of([C] * B, dev)
    flat = ccv.view(B * C, EP)
    for dcv in (c.dcv.to(dev), c.dcv16.to(dev)):
        for dattn in (c.dattn.to(dev), None):
            has = dattn is not None
            da_ = dattn if has else torch.empty(0, dtype=f32, device=dev)
            ds = nans((B * C,), f32, dev)
            dap = nans((B, EP), f32, dev)
            ext().attention_bwd_compact(dcv, da_, ccv, a, starts, attn, ds,
                                        dap, E, has)
            fd = dattn.reshape(-1) if has else None
            oc = twice(lambda: run_k22(dcv, fd, flat, a, starts.view(-1),
                                       off, attn.view(-1), E, True))
            od = twice(lambda: run_k22(dcv, fd, flat, a, starts.view(-1),
                                       off, attn.view(-1), E, False))
            assert torch.equal(oc["ds"], ds)
            assert torch.equal(oc["da_p"], dap)
            assert torch.equal(od["da_p"], dap)
            if dcv.dtype == f32:   # the padded dense binding takes f32 only
                dccv = nans((B, C, EP), bf16, dev)
                dap2 = nans((B, EP), f32, dev)
                ext().attention_bwd(dcv, da_, ccv, a, starts, attn, dccv,
                                    dap2, E, has)
                assert torch.equal(od["dccv"], dccv.view(B * C, EP))
                assert torch.equal(od["da_p"], dap2)
            assert torch.equal(
                oc["seg"].cpu(), (torch.arange(B * C) // C).to(i32))


# ---------------------------------------------------------------------------
# the packed modes of the recomputing combiner backward

SEED, OFFSET = 0x1234ABCD5678, 1000003


def combiner_forward(c, M, E, EP, p, dev):
    t = {k: getattr(c, k).to(dev) for k in ("x", "w", "gamma", "beta", "a")}
    f = dict(out=nans((M, EP), bf16, dev), z=nans((M, EP), bf16, dev),
             mean=nans((M,), f32, dev), rstd=nans((M,), f32, dev))
    off = torch.tensor([OFFSET], dtype=torch.int64, device=dev)
    ext().combiner_fwd(t["x"], t["w"], t["gamma"], t["beta"], f["out"],
                       f["z"], f["mean"], f["rstd"], E, p, SEED, off, 1)
    return t, f


def run_recompute(t, f, attn, ds, dcv, M, E, p, dev, C=None, seg=None):
    EP = 128
    grid = min((M + 3) // 4, 1024)
    o = dict(dz=nans((M, EP), bf16, dev), dgp=nans((grid, EP), f32, dev),
             dbp=nans((grid, EP), f32, dev))
    if seg is None:
        ext().combiner_bwd_recompute(attn, ds, dcv, t["a"], C, f["z"],
                                     f["out"], f["mean"], f["rstd"],
                                     t["gamma"], t["beta"], o["dz"], o["dgp"],
                                     o["dbp"], E, p)
    else:
        ext().combiner_bwd_recompute_packed(
            attn, ds, dcv, t["a"], seg, f["z"], f["out"], f["mean"],
            f["rstd"], t["gamma"], t["beta"], o["dz"], o["dgp"], o["dbp"], E,
            p)
    return o


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("M", [129, 8193])   # odd: a one-row tail pair
def test_combiner_packed_equal_lengths_bits(dev, M, p):
    E, EP, C = 100, 128, N.RECOMPUTE_C[M]
    t, f = combiner_forward(N.combiner_case(M, 32, E, EP), M, E, EP, p, dev)
    seg = (torch.arange(M) // C).to(i32).to(dev)
    for dcv_bf16 in (False, True):
        attn, ds, dcv, _ = N.recompute_inputs(M, C, EP, dcv_bf16)
        attn, ds, dcv = attn.to(dev), ds.to(dev), dcv.to(dev)
        ref = run_recompute(t, f, attn, ds, dcv, M, E, p, dev, C=C)
        got = twice(lambda: run_recompute(t, f, attn, ds, dcv, M, E, p, dev,
                                          seg=seg))
        for k in ("dz", "dgp", "dbp"):
            assert torch.equal(got[k], ref[k]), (k, dcv_bf16)


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_combiner_packed_ragged_fp64_rule(dev, p):
    """K21 -> compact K22 -> combiner_bwd_recompute_packed on the ragged
    batch; dz against the recompute bound with the fp64 dout rebuilt from
    the stored attn and ds through the stored seg."""
    E, EP, M, B = 100, 128, sum(LENGTHS), len(LENGTHS)
    c = N.combiner_case(M, 32, E, EP)
    t, f = combiner_forward(c, M, E, EP, p, dev)
    rc = ragged_case(E, EP)
    starts = rc["starts"].to(dev)
    off = offsets_of(LENGTHS, dev)
    attn = forward_attn(f["out"], t["a"], starts, LENGTHS, E)
    for dcv_bf16 in (False, True):
        dcv = rc["dcv"].to(dev)
        dcv = dcv.to(bf16) if dcv_bf16 else dcv
        k22 = run_k22(dcv, None, f["out"], t["a"], starts, off, attn, E, True)
        got = twice(lambda: run_recompute(t, f, attn, k22["ds"], dcv, M, E, p,
                                          dev, seg=k22["seg"]))
        seg = k22["seg"].cpu().long()
        dout, ddout = N.dout_recompute_ref(attn.cpu(), k22["ds"].cpu(),
                                           dcv.cpu()[seg], c.a, 1)
        r = N.combiner_bwd_ref(dout, f["z"].cpu(), f["out"].cpu(),
                               f["mean"].cpu(), f["rstd"].cpu(), c.gamma, E,
                               p, ddout)
        where = f"ragged M={M} p={p} dcv_bf16={dcv_bf16}"
        N.check(got["dz"], *r["dz"], "dz (recompute packed)", where)
        for nm, key in (("dgamma", "dg"), ("dbeta", "db")):
            pr = N.bwd_partials_ref(*r[key], M, 2)
            N.check(got[key + "p"], *pr["part"], f"{nm} partials (packed)",
                    where)


# ---------------------------------------------------------------------------
# the bindings' argument checks


def test_bindings_reject_bad_arguments(dev):
    E, EP, lens = 20, 32, [3, 4]
    M, B = 7, 2
    g = torch.Generator().manual_seed(0)
    ccv = torch.randn(M, EP, generator=g).to(bf16).to(dev)
    a = torch.randn(EP, generator=g).to(dev)
    starts = torch.ones(M, dtype=i32, device=dev)
    off = offsets_of(lens, dev)
    attn = forward_attn(ccv, a, starts, lens, E)
    dcv = torch.randn(B, EP, generator=g).to(dev)
    none = torch.empty(0, dtype=f32, device=dev)

    def call(**kw):
        v = dict(dcv=dcv, dattn=none, ccv=ccv, a=a, starts=starts, off=off,
                 attn=attn, ds=nans((M,), f32, dev),
                 seg=torch.zeros(M, dtype=i32, device=dev),
                 da=nans((B, EP), f32, dev), E=E, has=False, chunk=CHUNK)
        v.update(kw)
        ext().attention_packed_bwd_compact(
            v["dcv"], v["dattn"], v["ccv"], v["a"], v["starts"], v["off"],
            v["attn"], v["ds"], v["seg"], v["da"], v["E"], v["has"],
            v["chunk"])

    call()  # the baseline is accepted
    bad = dict(
        ccv_dtype=dict(ccv=ccv.float()),
        dcv_dtype=dict(dcv=dcv.double()),
        starts_dtype=dict(starts=starts.long()),
        seg_dtype=dict(seg=torch.zeros(M, dtype=torch.int64, device=dev)),
        off_dtype=dict(off=off.long()),
        ds_shape=dict(ds=nans((M - 1,), f32, dev)),
        da_shape=dict(da=nans((B + 1, EP), f32, dev)),
        attn_shape=dict(attn=attn[:-1].contiguous()),
        dattn_shape=dict(dattn=nans((M - 1,), f32, dev), has=True),
        attn_device=dict(attn=attn.cpu()),
        ccv_device=dict(ccv=ccv.cpu()),
        off_device=dict(off=off.cpu()),
        off_len=dict(off=offsets_of(lens + [0], dev)),
        ep_not_32=dict(ccv=ccv[:, :16].contiguous(),
                       dcv=dcv[:, :16].contiguous(), a=a[:16].contiguous(),
                       da=nans((B, 16), f32, dev), E=16),
        e_range=dict(E=EP + 1),
        chunk=dict(chunk=CHUNK + 1),
    )
    for name, kw in bad.items():
        with pytest.raises(RuntimeError):
            call(**kw)
            pytest.fail(f"accepted: {name}")
    # EP = 48: a multiple of 16 only
    ccv48 = torch.zeros(M, 48, dtype=bf16, device=dev)
    with pytest.raises(RuntimeError):
        call(ccv=ccv48, dcv=torch.zeros(B, 48, device=dev),
             a=torch.zeros(48, device=dev), da=nans((B, 48), f32, dev))
    # the dense form checks dccv
    with pytest.raises(RuntimeError):
        ext().attention_packed_bwd(dcv, none, ccv, a, starts, off, attn,
                                   nans((M, EP), f32, dev),
                                   nans((M,), f32, dev),
                                   nans((B, EP), f32, dev), E, False, CHUNK)
    # combiner_bwd_recompute_packed: seg dtype / length, EP != 128
    Mc, Ec = 6, 100
    c = N.combiner_case(5, 32, Ec, 128)
    t, f = combiner_forward(c, 5, Ec, 128, 0.0, dev)
    at5 = torch.full((5,), 0.2, device=dev)
    dcv5 = torch.zeros(1, 128, device=dev)
    seg5 = torch.zeros(5, dtype=i32, device=dev)
    run_recompute(t, f, at5, at5, dcv5, 5, Ec, 0.0, dev, seg=seg5)
    for seg_bad in (seg5.long(), seg5[:4].contiguous(), seg5.cpu()):
        with pytest.raises(RuntimeError):
            run_recompute(t, f, at5, at5, dcv5, 5, Ec, 0.0, dev, seg=seg_bad)
    with pytest.raises(RuntimeError):
        run_recompute(t, f, at5, at5, torch.zeros(1, 64, device=dev), 5, Ec,
                      0.0, dev, seg=seg5)


def test_autograd_wrappers_check_lengths_before_launch(dev):
    ccv = torch.zeros(5, 32, dtype=bf16, device=dev, requires_grad=True)
    a = torch.zeros(32, device=dev)
    starts = torch.ones(5, dtype=i32, device=dev)
    for lens in ([3, 0, 2], [3, -1, 3], [3, 3]):
        with pytest.raises(ValueError):
            Fn.attention_pool_packed_train(ccv, a, starts, lens, 20)
