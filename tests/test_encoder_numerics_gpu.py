"""The encoder kernels (K3-K9, K14, K15) under the elementwise fp64 rule of
tests/encoder_numerics.py: combiner_fwd in its template variants,
combiner_fwd_scores, gather_combiner_fwd, combiner_bwd v1/v2/recompute, every
attention forward and backward entry point, dgrad2, wgrad / wgrad_pipe /
wgrad_gather with wgrad_reduce, and both autograd paths end to end.

Entry points are called directly, stage by stage, on the tensors the stage
before stored.  Every output and scratch tensor is allocated NaN-filled, so
an unwritten element is a violation, and every result is produced twice and
compared bit for bit.  Run with -s to see max |err| / tol per output.
"""

import contextlib
import itertools
import os
import subprocess
import sys

import pytest
import torch

import encoder_numerics as N

pytestmark = pytest.mark.gpu

bf16 = torch.bfloat16
f32 = torch.float32
NAN = float("nan")

MS = (5, 129, 300)
KPS = (32, 64, 96, 320, 512)
EEP = ((100, 128), (128, 128), (20, 32), (150, 160), (200, 224))
ATTN = ((3, 1, 100, 128), (5, 63, 100, 128), (5, 65, 100, 128),
        (4, 200, 100, 128), (3, 201, 100, 128), (2, 1000, 100, 128),
        (4, 50, 20, 32))
DGRAD_M = (1, 127, 129, 1023, 1025)
DGRAD_KP = (8, 40, 256, 264, 320, 512)
WGRAD_M = (40, 300, 8193)
WGRAD_KP = (32, 96, 160, 320, 352, 512)
SEED, OFFSET = 0x1234ABCD5678, 1000003
# rows one pass of the 1024-block grid covers: 4 waves x 1 row (v1) or
# x 2 rows (v2, recompute); the next odd M has a one-row grid-stride tail
FULL_GRID_V1, FULL_GRID_V2 = 1024 * 4, 1024 * 8
RECOMPUTE_C = N.RECOMPUTE_C


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
    """Run fn (-> dict of tensors) twice; the runs must agree bit for bit."""
    r1, r2 = fn(), fn()
    for k in r1:
        if torch.is_tensor(r1[k]):
            assert same_bits(r1[k], r2[k]), f"{k}: run-to-run bits differ"
    return r1


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------
# combiner forward


def run_fwd(t, M, E, EP, p, epi, dev, scores=False, gather=None):
    """One forward launch into NaN-filled outputs.  t: device tensors."""
    o = dict(out=nans((M, EP), bf16, dev), z=nans((M, EP), bf16, dev),
             mean=nans((M,), f32, dev), rstd=nans((M,), f32, dev))
    off = torch.tensor([OFFSET], dtype=torch.int64, device=dev)
    if gather is not None:
        s, pa, e, term, path, KP = gather
        ext().gather_combiner_fwd(s, pa, e, term, path, t["w"], t["gamma"],
                                  t["beta"], o["out"], o["z"], o["mean"],
                                  o["rstd"], KP, E, p, SEED, off)
    elif scores:
        o["raw"] = nans((M,), f32, dev)
        o["wrote"] = ext().combiner_fwd_scores(
            t["x"], t["w"], t["gamma"], t["beta"], t["a"], o["out"], o["z"],
            o["mean"], o["rstd"], o["raw"], E, p, SEED, off, epi)
    else:
        ext().combiner_fwd(t["x"], t["w"], t["gamma"], t["beta"], o["out"],
                           o["z"], o["mean"], o["rstd"], E, p, SEED, off, epi)
    # the device-side counter advances by M * EP per dropout launch
    assert int(off) == OFFSET + (M * EP if p > 0 else 0)
    return o


def case_to(c, dev):
    return {k: getattr(c, k).to(dev)
            for k in ("x", "w", "gamma", "beta", "a", "dout")}


def check_fwd(o, r, where, E, keep=None):
    for k in ("z", "mean", "rstd", "out"):
        N.check(o[k], *r[k], k, where)
    if keep is not None:
        assert bool(((o["out"].cpu()[:, :E] != 0) == keep).all()), where


@pytest.mark.parametrize("KP", KPS)
@pytest.mark.parametrize("E,EP", EEP)
def test_combiner_fwd(dev, KP, E, EP):
    for M, p in itertools.product(MS, (0.0, 0.25)):
        c = N.combiner_case(M, KP, E, EP)
        t = case_to(c, dev)
        keep = (N.dropout_uniform(SEED, OFFSET, M, EP)[:, :E] >= p
                if p > 0 else None)
        base = twice(lambda: run_fwd(t, M, E, EP, p, 1, dev))
        if p == 0:
            # the mask is unambiguous: no kept element of this run is 0
            assert bool((base["out"][:, :E] != 0).all())
        r = N.combiner_fwd_ref(c.x, c.w, c.gamma, c.beta, E, p, base["out"])
        check_fwd(base, r, f"({M},{KP},{E},{EP}) p={p} epi=1", E, keep)
        variants = {"epi=0": (0, {}),
                    "MT=1": (1, {"C2V_COMBINER_MT": "1"}),
                    "OCC=0": (1, {"C2V_COMBINER_OCC": "0"})}
        for name, (epi, kv) in variants.items():
            with env(**kv):
                o = twice(lambda: run_fwd(t, M, E, EP, p, epi, dev))
            check_fwd(o, r, f"({M},{KP},{E},{EP}) p={p} {name}", E, keep)
            for k in ("z", "mean", "rstd", "out"):
                assert same_bits(o[k], base[k]), (name, k)
        if EP != 128:
            continue
        s = twice(lambda: run_fwd(t, M, E, EP, p, 1, dev, scores=True))
        assert s["wrote"] is True
        for k in ("z", "mean", "rstd", "out"):
            assert same_bits(s[k], base[k]), ("scores", k)
        N.check(s["raw"], *N.scores_ref(s["out"], c.a, E), "scores",
                f"({M},{KP},{E},{EP}) p={p}")
        s0 = run_fwd(t, M, E, EP, p, 0, dev, scores=True)
        assert s0["wrote"] is False and bool(torch.isnan(s0["raw"]).all())
        assert same_bits(s0["out"], base["out"])


@pytest.mark.parametrize("KP", KPS)
@pytest.mark.parametrize("E", [100, 128])
def test_gather_combiner_fwd(dev, KP, E):
    EP = 128
    for M, p in itertools.product(MS, (0.0, 0.25)):
        c = N.combiner_case(M, KP, E, EP)
        t = case_to(c, dev)
        s, pa, e, term, path, x = N.gather_tables(KP, M)
        g = tuple(v.to(dev) for v in (s, pa, e, term, path)) + (KP,)
        keep = (N.dropout_uniform(SEED, OFFSET, M, EP)[:, :E] >= p
                if p > 0 else None)
        r = None
        for name, kv in (("MT=2", {}), ("MT=1", {"C2V_COMBINER_MT": "1"})):
            with env(**kv):
                o = twice(lambda: run_fwd(t, M, E, EP, p, 1, dev, gather=g))
            if r is None:
                assert p > 0 or bool((o["out"][:, :E] != 0).all())
                r = N.combiner_fwd_ref(x, c.w, c.gamma, c.beta, E, p,
                                       o["out"])
            check_fwd(o, r, f"gather ({M},{KP},{E},{EP}) p={p} {name}", E,
                      keep)
        # the same operands through combiner_fwd: same bits, same mask
        t2 = dict(t, x=x.to(dev))
        o2 = run_fwd(t2, M, E, EP, p, 1, dev)
        for k in ("z", "mean", "rstd", "out"):
            assert same_bits(o[k], o2[k]), k


def test_dropout_mask_is_a_function_of_seed_row_col(dev):
    KP, E, EP, p = 64, 100, 128, 0.25
    c = N.combiner_case(300, KP, E, EP)
    t = case_to(c, dev)
    full = run_fwd(t, 300, E, EP, p, 1, dev)["out"]
    tp = dict(t, x=t["x"][:129].contiguous())
    part = run_fwd(tp, 129, E, EP, p, 1, dev)["out"]
    assert torch.equal(full[:129] != 0, part != 0)
    assert same_bits(full[:128].contiguous(), part[:128].contiguous())


# ---------------------------------------------------------------------------
# combiner backward


def run_bwd(t, f, M, E, EP, p, dev, recompute=None):
    grid = min((M + 3) // 4, 1024)
    o = dict(dz=nans((M, EP), bf16, dev), dgp=nans((grid, EP), f32, dev),
             dbp=nans((grid, EP), f32, dev), dg=nans((EP,), f32, dev),
             db=nans((EP,), f32, dev))
    if recompute is None:
        ext().combiner_bwd(t["dout"], f["z"], f["out"], f["mean"], f["rstd"],
                           t["gamma"], t["beta"], o["dz"], o["dgp"], o["dbp"],
                           E, p)
    else:
        attn, ds, dcv, C = recompute
        ext().combiner_bwd_recompute(attn, ds, dcv, t["a"], C, f["z"],
                                     f["out"], f["mean"], f["rstd"],
                                     t["gamma"], t["beta"], o["dz"], o["dgp"],
                                     o["dbp"], E, p)
    ext().slab_sum2_f32(o["dgp"], o["dbp"], o["dg"], o["db"])
    return o


def check_bwd(o, r, M, rpw, where):
    N.check(o["dz"], *r["dz"], "dz", where)
    for nm, key in (("dgamma", "dg"), ("dbeta", "db")):
        pr = N.bwd_partials_ref(*r[key], M, rpw)
        N.check(o[key + "p"], *pr["part"], f"{nm} partials", where)
        N.check(o[key], *pr["sum"], nm, where)


def bwd_cases(dev, M, E, EP, p, rpw, recompute_too):
    KP = 32
    c = N.combiner_case(M, KP, E, EP)
    t = case_to(c, dev)
    f = run_fwd(t, M, E, EP, p, 1, dev)
    fc = {k: v.cpu() for k, v in f.items()}
    where = f"({M},{E},{EP}) p={p} rows/wave={rpw}"
    o = twice(lambda: run_bwd(t, f, M, E, EP, p, dev))
    r = N.combiner_bwd_ref(c.dout, fc["z"], fc["out"], fc["mean"],
                           fc["rstd"], c.gamma, E, p)
    check_bwd(o, r, M, rpw, where)
    if not recompute_too:
        return
    for dcv_bf16 in (False, True):
        rc = N.recompute_inputs(M, RECOMPUTE_C[M], EP, dcv_bf16)
        rd = tuple(v.to(dev) for v in rc[:3]) + (rc[3],)
        o = twice(lambda: run_bwd(t, f, M, E, EP, p, dev, recompute=rd))
        dout, ddout = N.dout_recompute_ref(rc[0], rc[1], rc[2], c.a, rc[3])
        r = N.combiner_bwd_ref(dout, fc["z"], fc["out"], fc["mean"],
                               fc["rstd"], c.gamma, E, p, ddout)
        check_bwd(o, r, M, 2, f"{where} recompute dcv_bf16={dcv_bf16}")


def _v2_on():
    return os.environ.get("C2V_CB_V2", "1")[:1] != "0"


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("E", [100, 128])
def test_combiner_bwd_ep128_and_recompute(dev, E, p):
    """EP = 128: v2 (two rows per wave) unless C2V_CB_V2=0 is set for the
    whole process, and the dout-recomputing modes, which are always v2."""
    rpw = 2 if _v2_on() else 1
    for M in MS + (FULL_GRID_V2 + 1,):
        bwd_cases(dev, M, E, 128, p, rpw, recompute_too=True)
    if rpw == 1:
        bwd_cases(dev, FULL_GRID_V1 + 1, E, 128, p, 1, recompute_too=False)


@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("E,EP", [(20, 32), (150, 160), (200, 224)])
def test_combiner_bwd_v1(dev, E, EP, p):
    for M in MS + (FULL_GRID_V1 + 1,):
        bwd_cases(dev, M, E, EP, p, 1, recompute_too=False)


def test_combiner_bwd_v1_at_ep128(dev):
    """C2V_CB_V2 is read once per process, so v1 at EP = 128 needs a
    process of its own: this test re-runs the EP = 128 cases in a child
    with C2V_CB_V2=0.  The partial layout (block_of_row) differs between v1
    and v2, so the child's checks fail if the gate did not take."""
    if not _v2_on():
        return  # this process already runs v1 at EP = 128
    target = f"{os.path.abspath(__file__)}::test_combiner_bwd_ep128_and_recompute"
    res = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-s", "-x", "-m", "gpu",
         "-p", "no:cacheprovider", target],
        env=dict(os.environ, C2V_CB_V2="0"), capture_output=True, text=True,
        timeout=600, cwd=os.path.dirname(os.path.dirname(
            os.path.abspath(__file__))))
    print(res.stdout.replace("rows/wave=1", "rows/wave=1 (C2V_CB_V2=0)"))
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
    assert "4 passed" in res.stdout and "rows/wave=1" in res.stdout


# ---------------------------------------------------------------------------
# attention


def run_attn_fwd(kind, t, B, C, EP, E, dev, raw=None):
    o = dict(cv=nans((B, EP), f32, dev), attn=nans((B, C), f32, dev))
    if kind == "fwd":
        ext().attention_fwd(t["ccv"], t["a"], t["starts"], o["cv"], o["attn"],
                            E)
        return o
    o["cvb"] = nans((B, EP), bf16, dev)
    if kind == "cvb":
        ext().attention_fwd_cvb(t["ccv"], t["a"], t["starts"], o["cv"],
                                o["cvb"], o["attn"], E)
    else:
        ext().attention_fwd_scores(t["ccv"], raw, t["starts"], o["cv"],
                                   o["cvb"], o["attn"], E)
    return o


def run_attn_bwd(kind, t, attn, dcv, dattn, B, C, EP, E, dev):
    has = dattn is not None
    da_ = dattn if has else torch.empty(0, dtype=f32, device=dev)
    o = dict(da_part=nans((B, EP), f32, dev), da=nans((EP,), f32, dev))
    if kind == "dense":
        o["dccv"] = nans((B, C, EP), bf16, dev)
        ext().attention_bwd(dcv, da_, t["ccv"], t["a"], t["starts"], attn,
                            o["dccv"], o["da_part"], E, has)
    else:
        o["ds"] = nans((B * C,), f32, dev)
        if kind == "compact":
            ext().attention_bwd_compact(dcv, da_, t["ccv"], t["a"],
                                        t["starts"], attn, o["ds"],
                                        o["da_part"], E, has)
        else:
            ext().attention_bwd_compact_reg(dcv, da_, t["ccv"], t["starts"],
                                            attn, o["ds"], o["da_part"], E,
                                            has)
    ext().slab_sum_f32(o["da_part"], o["da"])
    return o


@pytest.mark.parametrize("B,C,E,EP", ATTN)
def test_attention(dev, B, C, E, EP):
    c = N.attention_case(B, C, E, EP)
    t = {k: getattr(c, k).to(dev)
         for k in ("ccv", "a", "starts", "dcv", "dcv16", "dattn")}
    where = f"({B},{C},{E},{EP})"
    stream = bool(ext().attention_stream_ok(C, EP))
    assert stream == (EP == 128 and C <= 200)
    r = N.attention_fwd_ref(c.ccv, c.a, c.starts, E)
    f = twice(lambda: run_attn_fwd("fwd", t, B, C, EP, E, dev))
    for k in ("attn", "cv"):
        N.check(f[k], *r[k], f"{k} (attention_fwd)", where)
    fb = twice(lambda: run_attn_fwd("cvb", t, B, C, EP, E, dev))
    for k in ("attn", "cv", "cvb"):
        N.check(fb[k], *r[k], f"{k} (attention_fwd_cvb)", where)
        assert k == "cvb" or same_bits(fb[k], f[k])
    if stream:
        # raw scores as the combiner's flush would hand them over
        raw = r["scores"][0].to(f32)
        rs = N.attention_fwd_ref(c.ccv, c.a, c.starts, E, raw=raw)
        raw_d = raw.flatten().contiguous().to(dev)
        fs = twice(lambda: run_attn_fwd("scores", t, B, C, EP, E, dev,
                                        raw=raw_d))
        for k in ("attn", "cv", "cvb"):
            N.check(fs[k], *rs[k], f"{k} (attention_fwd_scores)", where)
    pad = c.starts == 0
    if B > 1:
        pad[1] = False
    assert bool((f["attn"].cpu()[pad] == 0).all())
    attn = f["attn"]
    kinds = [("dense", t["dcv"]), ("compact", t["dcv"]),
             ("compact", t["dcv16"])]
    if stream:
        kinds += [("reg", t["dcv"]), ("reg", t["dcv16"])]
    ds_bits = {}
    for (kind, dcv), dattn in itertools.product(kinds, (None, t["dattn"])):
        tag = (f"{where} dcv={str(dcv.dtype)[6:]} "
               f"dattn={dattn is not None}")
        o = twice(lambda: run_attn_bwd(kind, t, attn, dcv, dattn, B, C, EP,
                                       E, dev))
        rb = N.attention_bwd_ref(dcv, dattn, c.ccv, c.a, c.starts, attn, E)
        for k in ("ds", "dccv", "da_part", "da"):
            if k in o:
                got = o[k].view(B, C) if k == "ds" else o[k]
                N.check(got, *rb[k], f"{k} (attention_bwd {kind})", tag)
        if "ds" in o:   # the two compact forms promise the same bits
            key = (dcv.dtype, dattn is not None)
            if key in ds_bits:
                assert same_bits(o["ds"], ds_bits[key][0]), tag
                assert same_bits(o["da_part"], ds_bits[key][1]), tag
            ds_bits[key] = (o["ds"], o["da_part"])


# ---------------------------------------------------------------------------
# dgrad2


@pytest.mark.parametrize("KP", DGRAD_KP)
def test_dgrad2(dev, KP):
    g = torch.Generator().manual_seed(KP)
    w = (torch.randn(128, KP, generator=g) * 0.1).to(bf16)
    w2 = w.t().contiguous().to(dev)
    for M in DGRAD_M:
        dz, _ = N.gemm_case(M, 128, 8, seed=1)
        dzd = dz.to(dev)

        def run():
            dx = nans((M, KP), bf16, dev)
            ext().dgrad2(dzd, w2, dx)
            return dict(dx=dx)
        o = twice(run)
        blocks = -(-KP // 256) * -(-M // 128)
        N.check(o["dx"], *N.dgrad_ref(dz, w), "dx (dgrad2)",
                f"({M},{KP}) blocks={blocks} swizzle={blocks % 8 == 0}")
    # both XCD swizzle branches are among the shapes
    counts = {-(-k // 256) * -(-m // 128)
              for k in DGRAD_KP for m in DGRAD_M}
    assert any(n % 8 == 0 for n in counts) and any(n % 8 for n in counts)


@pytest.mark.parametrize("M,KP,EP", [(129, 36, 128), (300, 100, 128),
                                     (129, 64, 32), (300, 320, 160)])
def test_dgrad_library_fallback(dev, M, KP, EP):
    from code2vec_amd.ops import functional as Fn

    g = torch.Generator().manual_seed(M + KP)
    w = (torch.randn(EP, KP, generator=g) * 0.1).to(bf16)
    dz, _ = N.gemm_case(M, EP, 8, seed=2)
    dx = Fn._combiner_dgrad(dz.to(dev), w.to(dev))
    N.check(dx, *N.dgrad_ref(dz, w), "dx (library)", f"({M},{KP},{EP})")


# ---------------------------------------------------------------------------
# wgrad


def run_wgrad(kind, x, dz, KP, EP, dev, gather=None):
    part = nans((N.WGRAD_SLABS, KP, EP), f32, dev)
    if kind == "wgrad":
        ext().wgrad(x, dz, part)
    elif kind == "pipe":
        ext().wgrad_pipe(x, dz, part, 2)
    else:
        ext().wgrad_gather(*gather, dz, part, KP)
    dw = nans((EP, KP), bf16, dev)
    ext().wgrad_reduce(part, dw)
    return dict(slabs=part, dw=dw)


@pytest.mark.parametrize("KP", WGRAD_KP)
@pytest.mark.parametrize("EP", [32, 128])
def test_wgrad(dev, KP, EP):
    for M in WGRAD_M:
        where = f"({M},{KP},{EP})"
        x, dz = N.gemm_case(M, KP, EP)
        xd, dzd = x.to(dev), dz.to(dev)
        r = N.wgrad_ref(x, dz)
        o = twice(lambda: run_wgrad("wgrad", xd, dzd, KP, EP, dev))
        N.check(o["slabs"], *r["slabs"], "wgrad slabs (wgrad)", where)
        N.check(o["dw"], *r["dw"], "dw (wgrad)", where)
        if EP == 128 and KP <= 480:
            op = twice(lambda: run_wgrad("pipe", xd, dzd, KP, EP, dev))
            N.check(op["slabs"], *r["slabs"], "wgrad slabs (wgrad_pipe)",
                    where)
            N.check(op["dw"], *r["dw"], "dw (wgrad_pipe)", where)
            assert same_bits(op["slabs"], o["slabs"])
        elif EP == 128:
            with pytest.raises(RuntimeError, match="no instantiation"):
                run_wgrad("pipe", xd, dzd, KP, EP, dev)
        s, pa, e, term, path, xg = N.gather_tables(KP, M)
        g = tuple(v.to(dev) for v in (s, pa, e, term, path))
        rg = N.wgrad_ref(xg, dz)
        og = twice(lambda: run_wgrad("gather", None, dzd, KP, EP, dev,
                                     gather=g))
        N.check(og["slabs"], *rg["slabs"], "wgrad slabs (wgrad_gather)",
                where)
        N.check(og["dw"], *rg["dw"], "dw (wgrad_gather)", where)
        del o, og, r, rg


# ---------------------------------------------------------------------------
# end to end: what autograd actually runs, stage by stage


def _e2e(dev, B, C, KP, p, extra, fused, monkeypatch, stream=True):
    import test_backward_fusions_gpu as BF
    from code2vec_amd.ops import functional as Fn

    E, EP = BF.E, BF.EP
    M = B * C
    t = BF._inputs(B, C, KP, dev, seed=100 + B + KP)
    where = (f"e2e {'fused' if fused else 'chain'} ({B},{C},{KP}) p={p} "
             f"extra={extra} stream={stream}")
    monkeypatch.setattr(Fn, "_ATTN_STREAM_FWD", stream)
    monkeypatch.setattr(Fn, "_ATTN_STREAM_BWD", stream)
    seen = {}
    real = Fn._combiner_dx_dw

    def spy(x, w, dz):
        seen["dz"] = dz.detach().clone()
        return real(x, w, dz)
    monkeypatch.setattr(Fn, "_combiner_dx_dw", spy)

    xh, wh, gh, bh, ah = [t[k].detach().clone().requires_grad_(True)
                          for k in ("x", "w", "gamma", "beta", "a")]
    Fn.reseed_dropout_rng(1234)
    if fused:
        cv, attn, cvb = Fn.CombinerAttentionPool.apply(
            xh, wh, gh, bh, ah, t["starts"], E, p, True)
        (_, _, _, _, _, _, z, mean, rstd, out, _) = cv.grad_fn.saved_tensors
    else:
        y = Fn.CombinerLNTanh.apply(xh, wh, gh, bh, E, p, True)
        y.register_hook(lambda g: seen.__setitem__("dccv", g.detach().clone()))
        (_, _, _, _, z, mean, rstd, out) = y.grad_fn.saved_tensors
        cv, attn = Fn.AttentionPool.apply(y.view(B, C, EP), ah, t["starts"],
                                          E)
        cvb = cv.to(bf16)
    outs, grads = [cvb], [t["g_cvb"]]
    if extra:
        outs += [cv, attn]
        grads += [t["g_cv32"], t["g_attn"]]
    torch.autograd.backward(outs, grads)

    cpu = {k: v.cpu() for k, v in t.items()}
    out_c = out.detach().cpu()
    r = N.combiner_fwd_ref(cpu["x"], cpu["w"], cpu["gamma"], cpu["beta"], E,
                           p, out_c)
    for k, got in (("z", z), ("mean", mean), ("rstd", rstd), ("out", out)):
        N.check(got.detach(), *r[k], k, where)
    ra = N.attention_fwd_ref(out_c.view(B, C, EP), cpu["a"], cpu["starts"], E)
    N.check(attn.detach(), *ra["attn"], "attn", where)
    N.check(cv.detach(), *ra["cv"], "cv", where)
    if fused:
        N.check(cvb.detach(), *ra["cvb"], "cvb", where)

    # backward, each stage from what the stage before it stored
    if fused:
        dcv = (t["g_cv32"] + t["g_cvb"]) if extra else t["g_cvb"]
    else:   # autograd accumulates the cast's gradient and cv's own in fp32
        dcv = (t["g_cvb"].float() + t["g_cv32"]) if extra else t["g_cvb"].float()
    dattn = cpu["g_attn"] if extra else None
    attn_c = attn.detach().cpu()
    rb = N.attention_bwd_ref(dcv.cpu(), dattn, out_c.view(B, C, EP),
                             cpu["a"], cpu["starts"], attn_c, E)
    N.check(ah.grad, *rb["da"], "da", where)
    if fused:
        dout, ddout = N.dout_recompute_ref(attn_c, rb["ds"][0], dcv.cpu(),
                                           cpu["a"], C, ds_tol=rb["ds"][1])
    else:
        N.check(seen["dccv"].view(B, C, EP), *rb["dccv"], "dccv", where)
        dout, ddout = seen["dccv"].cpu(), None
    rc = N.combiner_bwd_ref(dout, z.cpu(), out_c, mean.cpu(), rstd.cpu(),
                            cpu["gamma"], E, p, ddout)
    N.check(seen["dz"], *rc["dz"], "dz", where)
    rpw = 2 if (fused or _v2_on()) else 1
    N.check(gh.grad, *N.bwd_partials_ref(*rc["dg"], M, rpw)["sum"], "dgamma",
            where)
    N.check(bh.grad, *N.bwd_partials_ref(*rc["db"], M, rpw)["sum"], "dbeta",
            where)
    dz_c = seen["dz"].cpu()
    N.check(xh.grad, *N.dgrad_ref(dz_c, cpu["w"]), "dx", where)
    N.check(wh.grad, *N.wgrad_ref(cpu["x"], dz_c)["dw"], "dw", where)


def _cap_cases():
    import test_backward_fusions_gpu as BF
    return BF.CAP_CASES


@pytest.mark.parametrize("B,C,KP,p,extra", _cap_cases())
def test_end_to_end_stage_by_stage(dev, monkeypatch, B, C, KP, p, extra):
    _e2e(dev, B, C, KP, p, extra, True, monkeypatch)
    _e2e(dev, B, C, KP, p, extra, False, monkeypatch)
    if C <= 200:   # the tiled kernels at the streaming kernels' shapes
        _e2e(dev, B, C, KP, p, extra, True, monkeypatch, stream=False)
