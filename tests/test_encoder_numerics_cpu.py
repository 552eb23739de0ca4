"""The encoder-numerics bounds (tests/encoder_numerics.py) are neither loose
nor tight: (a) a torch CPU emulation of each encoder op - fp32 math with the
kernels' rounding points: bf16 z, fp32 one-pass statistics, fast_tanh, bf16
out, bf16 dz, fp32 partials - passes every bound with zero violations at
every shape of test_encoder_numerics_gpu.py; (b) mutations of the fp64
reference, each a plausible kernel bug, are flagged, at the planted element
where there is one.

No GPU.  Run with -s to see max |err| / tol per output.
"""

import itertools

import pytest
import torch

import encoder_numerics as N

bf16 = torch.bfloat16
f32 = torch.float32

MS = (5, 129, 300)
KPS = (32, 64, 96, 320, 512)
EEP = ((100, 128), (128, 128), (20, 32), (150, 160), (200, 224))
ATTN = ((3, 1, 100, 128), (5, 63, 100, 128), (5, 65, 100, 128),
        (4, 200, 100, 128), (3, 201, 100, 128), (2, 1000, 100, 128),
        (4, 50, 20, 32))
DGRAD = tuple(itertools.product((1, 127, 129, 1023, 1025),
                                (8, 40, 256, 264, 320, 512)))
WGRAD_M = (40, 300, 8193)
WGRAD_KP = (32, 96, 160, 320, 352, 512)
WGRAD_EP = (32, 128)
SEED, OFFSET = 0x1234ABCD5678, 1000003


# ---------------------------------------------------------------------------
# the emulation: fp32 torch with the kernels' rounding points


def emu_combiner_fwd(c, p=0.0, M=None):
    M = c.M if M is None else M
    E, EP = c.E, c.EP
    acc = c.x[:M].float() @ c.w.float().t()
    invE = torch.tensor(1.0, dtype=f32) / torch.tensor(float(E), dtype=f32)
    mean = acc.sum(dim=1) * invE
    var = ((acc * acc).sum(dim=1) * invE - mean * mean).clamp_min(0.0)
    rstd = torch.rsqrt(var + torch.tensor(N.LN_EPS, dtype=f32))
    u = (acc - mean[:, None]) * rstd[:, None] * c.gamma + c.beta
    t = 1.0 - 2.0 / (torch.exp(2.0 * u.abs()) + 1.0)
    y = torch.copysign(t, u)
    if p > 0:
        inv = torch.tensor(1.0, dtype=f32) / (1.0 - torch.tensor(p, dtype=f32))
        u01 = N.dropout_uniform(SEED, OFFSET, M, EP).float()
        y = torch.where(u01 >= p, y * inv, torch.zeros_like(y))
    y[:, E:] = 0
    acc[:, E:] = 0
    out = y.to(bf16)
    ts = min(N.round8(E), EP)
    scores = (out.float()[:, :ts] * c.a[:ts]).sum(dim=1)
    return dict(z=acc.to(bf16), mean=mean, rstd=rstd, out=out, scores=scores)


def emu_combiner_bwd(dout, f, gamma, E, p, rows_per_wave):
    z, out = f["z"].float(), f["out"].float()
    M, EP = z.shape
    invE = torch.tensor(1.0 / E, dtype=f32)
    one_mp = 1.0 - torch.tensor(p, dtype=f32)
    inv = (1.0 / one_mp) if p > 0 else torch.tensor(1.0, dtype=f32)
    xh = (z - f["mean"][:, None]) * f["rstd"][:, None]
    y = out * one_mp
    dy = torch.where(out != 0, dout.float() * inv, torch.zeros_like(out))
    dd = dy * (1.0 - y * y)
    h = dd * gamma
    s1 = h.sum(dim=1, keepdim=True) * invE
    s2 = (h * xh).sum(dim=1, keepdim=True) * invE
    dz = f["rstd"][:, None] * (h - s1 - xh * s2)
    dz[:, E:] = 0
    blk = N.block_of_row(M, rows_per_wave)
    grid = min((M + 3) // 4, N.BWD_MAX_GRID)
    dgp = torch.zeros(grid, EP).index_add_(0, blk, dd * xh)
    dbp = torch.zeros(grid, EP).index_add_(0, blk, dd)
    return dict(dz=dz.to(bf16), dgp=dgp, dbp=dbp, dg=dgp.sum(dim=0),
                db=dbp.sum(dim=0))


def emu_dout(attn, ds, dcv, a, C):
    rows = torch.arange(attn.numel()) // C
    return (attn.flatten()[:, None] * dcv.float()[rows]
            + ds.flatten()[:, None] * a[None, :]).to(bf16)


def emu_attention_fwd(c):
    ts = min(N.round8(c.E), c.EP)
    x = c.ccv.float()
    s = (x[..., :ts] * c.a[:ts]).sum(dim=-1)
    mask = (c.starts > 0).float()
    sm = s * mask + (1.0 - mask) * torch.tensor(N.NINF, dtype=f32)
    e = torch.exp(sm - sm.max(dim=1, keepdim=True).values)
    attn = e * (1.0 / e.sum(dim=1, keepdim=True))
    cv = torch.einsum("bc,bce->be", attn, x)
    cv[:, ts:] = 0
    return dict(scores=s, attn=attn, cv=cv, cvb=cv.to(bf16))


def emu_attention_bwd(c, attn, dcv, dattn):
    ts = min(N.round8(c.E), c.EP)
    x = c.ccv.float()
    g = (x[..., :ts] * dcv.float()[:, None, :ts]).sum(dim=-1)
    if dattn is not None:
        g = g + dattn
    sg = (attn * g).sum(dim=1, keepdim=True)
    ds = attn * (g - sg) * (c.starts > 0).float()
    dccv = attn[:, :, None] * dcv.float()[:, None, :] + ds[:, :, None] * c.a
    dccv[..., ts:] = 0
    dap = torch.einsum("bc,bce->be", ds, x)
    dap[:, c.E:] = 0
    return dict(ds=ds, dccv=dccv.to(bf16), da_part=dap, da=dap.sum(dim=0))


def emu_wgrad(x, dz):
    M, KP = x.shape
    EP = dz.shape[1]
    S = N.WGRAD_SLABS
    rpb = N.wgrad_rows_per_block(M)
    xp = torch.zeros(S * rpb, KP)
    zp = torch.zeros(S * rpb, EP)
    xp[:M], zp[:M] = x.float(), dz.float()
    slabs = xp.view(S, rpb, KP).transpose(1, 2) @ zp.view(S, rpb, EP)
    return slabs, slabs.sum(dim=0).t().contiguous().to(bf16)


# ---------------------------------------------------------------------------
# (a) accept


def _fwd_checks(c, p, where):
    f = emu_combiner_fwd(c, p)
    r = N.combiner_fwd_ref(c.x, c.w, c.gamma, c.beta, c.E, p, f["out"])
    for k in ("z", "mean", "rstd", "out"):
        N.check(f[k], *r[k], f"emu {k}", where)
    N.check(f["scores"], *N.scores_ref(f["out"], c.a, c.E), "emu scores",
            where)
    return f, r


@pytest.mark.parametrize("KP", KPS)
@pytest.mark.parametrize("E,EP", EEP)
def test_emulated_combiner_forward_accepted(KP, E, EP):
    for M in MS:
        c = N.combiner_case(M, KP, E, EP)
        f0, r0 = _fwd_checks(c, 0.0, f"({M},{KP},{E},{EP}) p=0")
        # the mask is unambiguous: no kept element of the p = 0 run is 0
        assert bool((f0["out"][:, :E] != 0).all())
        assert bool((f0["out"][:, E:] == 0).all())
        f1, _ = _fwd_checks(c, 0.25, f"({M},{KP},{E},{EP}) p=0.25")
        keep = N.dropout_uniform(SEED, OFFSET, M, EP)[:, :E] >= 0.25
        assert bool(((f1["out"][:, :E] != 0) == keep).all())
        # the data is what the docstring promises
        zr, mr = r0["z"][0][:, :E], r0["mean"][0]
        std = (zr - mr[:, None]).pow(2).mean(dim=1).sqrt()
        for r in c.offset_rows:
            assert 7.0 < float(mr[r].abs() / std[r]) < 9.0, (M, KP, r)
        for r in c.zero_rows:
            assert float(zr[r].abs().max()) == 0.0
            assert abs(float(r0["rstd"][0][r]) - N.LN_EPS ** -0.5) < 1e-9
        u = r0["u"].abs()
        assert float(u[:, c.small_cols].max()) < 0.2
        if M > 5:
            assert float(u[:, c.sat_cols].max()) > 8.0


def test_dropout_mask_depends_on_seed_row_col_only():
    c = N.combiner_case(300, 64, 100, 128)
    full = emu_combiner_fwd(c, 0.25)["out"]
    part = emu_combiner_fwd(c, 0.25, M=129)["out"]
    assert torch.equal(full[:129] != 0, part != 0)
    rate = float((full[:, :100] != 0).float().mean())
    assert abs(rate - 0.75) < 0.02


def _bwd_checks(c, p, rows_per_wave, where, recompute=None):
    f = emu_combiner_fwd(c, p)
    dout_emu, dout_ref, ddout = c.dout, c.dout, None
    if recompute is not None:
        attn, ds, dcv, C = recompute
        dout_emu = emu_dout(attn, ds, dcv, c.a, C)
        dout_ref, ddout = N.dout_recompute_ref(attn, ds, dcv, c.a, C)
        # the fp32 rounding differs from the fp64 one only where allowed
        assert bool(((N.d(dout_emu) - dout_ref).abs() <= ddout).all())
    e = emu_combiner_bwd(dout_emu, f, c.gamma, c.E, p, rows_per_wave)
    r = N.combiner_bwd_ref(dout_ref, f["z"], f["out"], f["mean"], f["rstd"],
                           c.gamma, c.E, p, ddout)
    N.check(e["dz"], *r["dz"], "emu dz", where)
    for nm, key in (("dgamma", "dg"), ("dbeta", "db")):
        pr = N.bwd_partials_ref(*r[key], c.M, rows_per_wave)
        N.check(e[key + "p"], *pr["part"], f"emu {nm} partials", where)
        N.check(e[key], *pr["sum"], f"emu {nm}", where)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("E,EP,rpw", [
    (100, 128, 2), (128, 128, 2), (100, 128, 1), (128, 128, 1),
    (20, 32, 1), (150, 160, 1), (200, 224, 1)])
def test_emulated_combiner_backward_accepted(E, EP, rpw, p):
    # one odd M just above what a full grid covers: 1024 blocks x 4 waves x
    # rows per wave
    for M in MS + (1024 * 4 * rpw + 1,):
        c = N.combiner_case(M, 32, E, EP)
        _bwd_checks(c, p, rpw, f"({M},{E},{EP}) rows/wave={rpw} p={p}")
        if EP == 128 and rpw == 2:
            for bf in (False, True):
                _bwd_checks(
                    c, p, 2, f"({M},{E},{EP}) recompute bf16={bf} p={p}",
                    N.recompute_inputs(M, N.RECOMPUTE_C[M], EP, bf))


@pytest.mark.parametrize("B,C,E,EP", ATTN)
def test_emulated_attention_accepted(B, C, E, EP):
    c = N.attention_case(B, C, E, EP)
    where = f"({B},{C},{E},{EP})"
    f = emu_attention_fwd(c)
    r = N.attention_fwd_ref(c.ccv, c.a, c.starts, E)
    for k in ("scores", "attn", "cv", "cvb"):
        N.check(f[k], *r[k], f"emu {k}", where)
    # the planted structure
    attn = r["attn"][0]
    if B > 1:
        assert bool((attn[1] == 1.0 / C).all())
    pad = c.starts == 0
    pad[1 if B > 1 else slice(0, 0)] = False
    assert bool((attn[pad] == 0).all()) and bool((f["attn"][pad] == 0).all())
    s = r["scores"][0]
    for b, pos in c.dominant.items():
        rest = s[b].clone()
        rest[pos] = -1e9
        rest[c.starts[b] == 0] = -1e9
        assert C == len(pos) or float(s[b, pos].min() - rest.max()) >= 10.0
        assert bool((c.starts[b, pos] > 0).all())
    for dcv, dattn in itertools.product((c.dcv, c.dcv16), (None, c.dattn)):
        e = emu_attention_bwd(c, f["attn"], dcv, dattn)
        rb = N.attention_bwd_ref(dcv, dattn, c.ccv, c.a, c.starts, f["attn"],
                                 E)
        tag = f"{where} dcv={str(dcv.dtype)[6:]} dattn={dattn is not None}"
        for k in ("ds", "dccv", "da_part", "da"):
            N.check(e[k], *rb[k], f"emu {k}", tag)


@pytest.mark.parametrize("M,KP", DGRAD)
def test_emulated_dgrad_accepted(M, KP):
    dz, _ = N.gemm_case(M, 128, 8, seed=1)
    w = (torch.randn(128, KP, generator=torch.Generator().manual_seed(KP))
         * 0.1).to(bf16)
    dx = (dz.float() @ w.float()).to(bf16)
    N.check(dx, *N.dgrad_ref(dz, w), "emu dx", f"({M},{KP})")


@pytest.mark.parametrize("KP", WGRAD_KP)
@pytest.mark.parametrize("EP", WGRAD_EP)
def test_emulated_wgrad_accepted(KP, EP):
    for M in WGRAD_M:
        x, dz = N.gemm_case(M, KP, EP)
        slabs, dw = emu_wgrad(x, dz)
        r = N.wgrad_ref(x, dz)
        N.check(slabs, *r["slabs"], "emu wgrad slabs", f"({M},{KP},{EP})")
        N.check(dw, *r["dw"], "emu dw", f"({M},{KP},{EP})")
        empty = r["rows"] == 0
        assert bool((r["slabs"][1][empty] == 0).all())
        assert int(empty.sum()) == N.WGRAD_SLABS - -(-M // N.wgrad_rows_per_block(M))
    assert N.wgrad_rows_per_block(8193) == 64 and 8193 % 64 == 1


# ---------------------------------------------------------------------------
# (b) reject: mutations of the fp64 reference


def _flagged(got, ref, tol, at=None):
    bad = N.violations(got, ref, tol)
    assert bool(bad.any())
    if at is not None:
        assert bool(bad[at].any()), at
    return bad


def test_mutations_of_combiner_forward_flagged():
    M, KP, E, EP = 300, 320, 100, 128
    c = N.combiner_case(M, KP, E, EP)
    f = emu_combiner_fwd(c)
    r = N.combiner_fwd_ref(c.x, c.w, c.gamma, c.beta, E)
    # last row of a 128-row block dropped (left unwritten: here 0)
    for k in ("z", "out"):
        ref, tol = r[k]
        mut = ref.clone()
        mut[127] = ref[126]
        _flagged(f[k], mut, tol, at=127)
        got = f[k].clone()
        got[255] = 0
        bad = _flagged(got, ref, tol, at=255)
        assert not bool(bad[:255].any()) and not bool(bad[256:].any())
    # one 32-wide k-step of ten dropped: k-step 0 carries the offset
    # direction, k-step 9 is an ordinary one
    for kstep in (0, 9):
        m = N.combiner_fwd_ref(c.x, c.w, c.gamma, c.beta, E, drop_k=kstep)
        bad = _flagged(f["z"], *m["z"])
        assert float(bad[:, :E].double().mean()) > 0.5
        print(f"k-step {kstep} dropped: relative Frobenius "
              f"{N.frobenius(f['z'], m['z'][0]):.3e}")
    _flagged(f["z"], *N.combiner_fwd_ref(c.x, c.w, c.gamma, c.beta, E,
                                         drop_k=0)["z"], at=c.offset_rows[0])
    # mean over EP instead of E: the offset rows feel it most
    m = N.combiner_fwd_ref(c.x, c.w, c.gamma, c.beta, E, mean_over=EP)
    for k in ("mean", "rstd", "out"):
        _flagged(f[k], *m[k], at=c.offset_rows[0])
    # pad column not zeroed
    got = f["out"].clone()
    got[17, E] = 2.0 ** -100
    bad = _flagged(got, *r["out"], at=(17, E))
    assert int(bad.sum()) == 1
    # a wrong score column count: column E-1 left out of the dot
    sref, stol = N.scores_ref(f["out"], c.a, E)
    o = f["out"].clone()
    o[:, E - 1] = 0
    _flagged(f["scores"], N.scores_ref(o, c.a, E)[0], stol)
    assert not bool(N.violations(f["scores"], sref, stol).any())


def test_mutations_of_combiner_backward_flagged():
    E, EP, p = 100, 128, 0.25
    c = N.combiner_case(300, 96, E, EP)
    f = emu_combiner_fwd(c, p)
    e = emu_combiner_bwd(c.dout, f, c.gamma, E, p, 2)
    args = (c.dout, f["z"], f["out"], f["mean"], f["rstd"], c.gamma, E, p)
    # tanh derivative set to 1: the saturated columns are O(1) wrong
    m = N.combiner_bwd_ref(*args, tanh_deriv=False)
    bad = _flagged(e["dz"], *m["dz"])
    assert bool(bad[:, c.sat_cols].any())
    _flagged(e["db"], *N.bwd_partials_ref(*m["db"], c.M, 2)["sum"],
             at=c.sat_cols[0])
    # dropout scale missing in backward
    m = N.combiner_bwd_ref(*args, scale=False)
    _flagged(e["dz"], *m["dz"])
    _flagged(e["dg"], *N.bwd_partials_ref(*m["dg"], c.M, 2)["sum"])
    # the partial layout tells the two kernels apart
    r = N.combiner_bwd_ref(*args)
    _flagged(e["dgp"], *N.bwd_partials_ref(*r["dg"], c.M, 1)["part"])
    # dgamma/dbeta missing the rows past one grid's coverage
    for M, rpw in ((4097, 1), (8193, 2)):
        c = N.combiner_case(M, 32, E, EP)
        f = emu_combiner_fwd(c, p)
        e = emu_combiner_bwd(c.dout, f, c.gamma, E, p, rpw)
        r = N.combiner_bwd_ref(c.dout, f["z"], f["out"], f["mean"],
                               f["rstd"], c.gamma, E, p)
        for key in ("dg", "db"):
            m = N.bwd_partials_ref(*r[key], M, rpw, drop_past_grid=True)
            ok = N.bwd_partials_ref(*r[key], M, rpw)
            bad = _flagged(e[key + "p"], *m["part"])
            # only block 0 visits row M-1
            assert bool(bad[0].any()) and not bool(bad[1:].any())
            assert not bool(N.violations(e[key + "p"], *ok["part"]).any())
            print(f"{key} tail row of M={M} dropped: sum flagged = "
                  f"{bool(N.violations(e[key], *m['sum']).any())}")
    # ds a deleted from the recomputed dout
    c = N.combiner_case(300, 96, E, EP)
    f = emu_combiner_fwd(c, p)
    attn, ds, dcv, C = N.recompute_inputs(300, 3, EP, False)
    e = emu_combiner_bwd(emu_dout(attn, ds, dcv, c.a, C), f, c.gamma, E, p, 2)
    dm, ddm = N.dout_recompute_ref(attn, ds, dcv, c.a, C, dsa=False)
    m = N.combiner_bwd_ref(dm, f["z"], f["out"], f["mean"], f["rstd"],
                           c.gamma, E, p, ddm)
    _flagged(e["dz"], *m["dz"])


@pytest.mark.parametrize("B,C", [(5, 65), (4, 200), (2, 1000)])
def test_mutations_of_attention_flagged(B, C):
    E = 100
    c = N.attention_case(B, C)
    f = emu_attention_fwd(c)
    # a dominant context dropped from the softmax: C-1, 63, 64, last valid
    for b, pos in c.dominant.items():
        for q in pos:
            st = c.starts.clone()
            st[b, q] = 0
            m = N.attention_fwd_ref(c.ccv, c.a, st, E)
            bad = _flagged(f["attn"], *m["attn"], at=(b, q))
            assert bool(bad[b][c.starts[b] > 0].all())
            _flagged(f["cv"], *m["cv"], at=b)
    assert any(C - 1 in pos or B < 3 for pos in c.dominant.values())
    # mask ignored
    m = N.attention_fwd_ref(c.ccv, c.a, c.starts, E, use_mask=False)
    _flagged(f["attn"], *m["attn"], at=1)
    for dattn in (None, c.dattn):
        e = emu_attention_bwd(c, f["attn"], c.dcv, dattn)
        kw = dict(dcv=c.dcv, dattn=dattn, ccv=c.ccv, a=c.a, starts=c.starts,
                  attn=f["attn"], E=E)
        # - sum attn g deleted
        m = N.attention_bwd_ref(**kw, center=False)
        for k in ("ds", "dccv", "da"):
            _flagged(e[k], *m[k])
        # ds a deleted from dccv
        _flagged(e["dccv"], *N.attention_bwd_ref(**kw, dsa=False)["dccv"])
        # mask ignored in ds: the all-pad method has attn = 1/C everywhere
        _flagged(e["ds"], *N.attention_bwd_ref(**kw, use_mask=False)["ds"],
                 at=1)
    # dattn ignored
    e = emu_attention_bwd(c, f["attn"], c.dcv, c.dattn)
    m = N.attention_bwd_ref(c.dcv, None, c.ccv, c.a, c.starts, f["attn"], E)
    for k in ("ds", "dccv", "da_part", "da"):
        _flagged(e[k], *m[k])


def test_mutations_of_the_gemms_flagged():
    # dgrad2: a 32-wide k-step of four dropped
    dz, _ = N.gemm_case(129, 128, 8, seed=1)
    w = (torch.randn(128, 264, generator=torch.Generator().manual_seed(3))
         * 0.1).to(bf16)
    dx = (dz.float() @ w.float()).to(bf16)
    wm = w.clone()
    wm[96:] = 0
    bad = _flagged(dx, *N.dgrad_ref(dz, wm))
    assert float(bad.double().mean()) > 0.5
    # wgrad: a row (the last of a 128-row block; the one-row last slab), a
    # slab, garbage in an empty slab
    for M, row in ((300, 127), (8193, 8192)):
        x, dzz = N.gemm_case(M, 96, 128)
        slabs, dw = emu_wgrad(x, dzz)
        r = N.wgrad_ref(x, dzz)
        m = N.wgrad_ref(x, dzz, drop_row=row)
        s = row // N.wgrad_rows_per_block(M)
        bad = _flagged(slabs, *m["slabs"], at=s)
        assert not bool(bad[:s].any()) and not bool(bad[s + 1:].any())
        print(f"row {row} of M={M} dropped: dw flagged = "
              f"{bool(N.violations(dw, *m['dw']).any())}, relative "
              f"Frobenius {N.frobenius(dw, m['dw'][0]):.3e}")
        # one slab dropped from the reduction
        ref, tol = r["dw"]
        _flagged(dw, ref - r["slabs"][0][s].t(), tol)
        # an empty slab holding garbage
        if M == 300:
            got = slabs.clone()
            got[200, 5, 7] = 1e-30
            assert int(_flagged(got, *r["slabs"], at=(200, 5, 7)).sum()) == 1
    _flagged(emu_wgrad(*N.gemm_case(300, 96, 128))[1],
             *N.wgrad_ref(*N.gemm_case(300, 96, 128), drop_row=127)["dw"])
