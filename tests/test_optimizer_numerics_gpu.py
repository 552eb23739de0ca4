"""The scatter and Adam kernels (K1/K2 forward gather, K13, K16, the fp32 and
multi-tensor Adam, K16b) under the elementwise fp64 rule of
tests/optimizer_numerics.py.

Entry points are called directly on planted records.  Outputs the entry point
takes are allocated NaN-filled, every call runs twice from the same state and
the two runs must agree bit for bit wherever the addition order is fixed (rows
whose run spans at most two 16-entry chunks, and everything in Adam); after
every call counts, flags and the fp32 scratch must be all-zero.  No element
is excluded from the rule.  Run with -s to see max |err| / tol per output.
"""

import os
import subprocess
import sys

import pytest
import torch

import optimizer_numerics as N

pytestmark = pytest.mark.gpu

from code2vec_amd.ops import ext
from code2vec_amd.ops import functional as Fn

bf16 = torch.bfloat16
f32 = torch.float32
NAN = float("nan")
KEYS = N.all_scatter_keys()
KEY_IDS = ["-".join(map(str, k)) for k in KEYS]
SOURCES = ("group_by_index", "group_tables bucket", "group_tables chain")
GRID1_N = 2 * 4096 + 1027  # C2V_ADAM_GRID=1: 3 trips at ILP 4, 10 at ILP 1,
#                            and a 3-element scalar tail


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    N.print_worst("MI355X")


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """Nothing more runs on the device once a kernel has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault, run ended: {e}", returncode=3)


def nans(shape, dtype, dev):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=dev)


def same_bits(a, b):
    if a.dtype == bf16:
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def all_zero(t):
    return not bool(t.any())


# ---------------------------------------------------------------------------
# records


def records(case, source, dev, monkeypatch):
    """{tag: (sorted_idx, perm, counts, cursor)} of both tables, checked
    against the plan."""
    out = {}
    if source == "group_by_index":
        for tag, tb in case.tables.items():
            out[tag] = Fn._group_by_index(tb.idx.to(dev), tb.rows,
                                          with_cursor=True)
    else:
        monkeypatch.setenv("C2V_GROUP_SORT",
                           "1" if source.endswith("bucket") else "0")
        M, T1, P1 = case.M, case.T + 1, case.P + 1
        for tag, rows, n in (("term", T1, 2 * M), ("path", P1, M)):
            out[tag] = (torch.full((n,), -7, dtype=torch.int32, device=dev),
                        torch.full((n,), -7, dtype=torch.int64, device=dev),
                        torch.zeros(rows, dtype=torch.int32, device=dev),
                        torch.full((rows,), -7, dtype=torch.int32,
                                   device=dev))
        spart = torch.empty(int(ext().group_tables_partials_len(T1, P1)),
                            dtype=torch.int32, device=dev)
        tmp = torch.empty(int(ext().group_tables_tmp_len(M, T1, P1)),
                          dtype=torch.int32, device=dev)
        t, p = out["term"], out["path"]
        on_side = ext().group_tables(
            case.starts.to(dev), case.paths.to(dev), case.ends.to(dev), t[2],
            p[2], t[3], p[3], spart, t[0], t[1], p[0], p[1], T1, P1, False,
            tmp)
        assert on_side is False
    for tag, tb in case.tables.items():
        sorted_idx, perm, counts, cursor = out[tag]
        want = torch.sort(tb.idx.long()).values
        assert torch.equal(sorted_idx.cpu().long(), want), (source, tag)
        assert torch.equal(tb.idx.long()[perm.cpu()], want), (source, tag)
        cnt = torch.bincount(tb.idx.long(), minlength=tb.rows + 1)
        assert torch.equal(counts.cpu().long(), cnt), (source, tag)
        assert torch.equal(cursor.cpu().long()[:tb.rows],
                           torch.cumsum(cnt, 0)[:tb.rows]), (source, tag)
    return out


# ---------------------------------------------------------------------------
# K13


def run_k13(case, tag, rec, gout, dev, where):
    tb = case.tables[tag]
    sorted_idx, perm, counts, _ = rec
    ref, tol, _, _ = N.table_ref(case, tag)
    scratch = torch.zeros(tb.rows, tb.S, device=dev)
    flags = torch.zeros(tb.rows, dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        cnt = counts.clone()
        dense = nans((tb.rows, tb.S), bf16, dev)
        ext().embed_scatter_sorted(sorted_idx, perm, gout, scratch, dense,
                                   flags, case.M, case.KP, tb.off0, tb.off1,
                                   16)
        ext().cast_clear_rows(scratch, cnt, flags, dense)
        assert all_zero(cnt) and all_zero(flags) and all_zero(scratch), where
        outs.append(dense)
    fixed = tb.fixed_order.to(dev)
    assert same_bits(outs[0][fixed], outs[1][fixed]), where
    for o in outs:
        N.within(o, ref, tol, f"K13 dense gradient ({tag})", where)
        if case.grad == "int":
            assert same_bits(o.cpu(), ref.float().to(bf16)), where


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_k13_scatter_sorted(dev, monkeypatch, key):
    case = N.scatter_case(*key)
    gout = case.gout.to(dev)
    for source in SOURCES:
        rec = records(case, source, dev, monkeypatch)
        for tag in ("term", "path"):
            run_k13(case, tag, rec[tag], gout, dev,
                    f"{case.name()} {source}")


def _scatter_invariants():
    seen = 0
    for key, buf in Fn._scratch_cache.items():
        if (key[0] in ("term", "path") or key[0] == "flags"
                or (key[0] == "i32" and key[1].startswith("counts_"))):
            assert all_zero(buf), key
            seen += 1
    assert seen >= 6


@pytest.mark.parametrize("key", [KEYS[1], KEYS[-4], KEYS[-2]],
                         ids=[KEY_IDS[1], KEY_IDS[-4], KEY_IDS[-2]])
def test_scatter_embedding_grads_end_to_end(dev, key):
    """Fn._scatter_embedding_grads without owner keys: counting sort, scan,
    scatter and cast_clear_rows on the persistent buffers."""
    case = N.scatter_case(*key)
    gout = case.gout.to(dev)
    s, p, e = (x.to(dev) for x in (case.starts, case.paths, case.ends))
    outs = []
    for _ in range(2):
        outs.append(Fn._scatter_embedding_grads(
            s, p, e, gout, (case.T, case.TS), (case.P, case.PS)))
        _scatter_invariants()
    for i, tag in enumerate(("term", "path")):
        tb = case.tables[tag]
        ref, tol, _, _ = N.table_ref(case, tag)
        fixed = tb.fixed_order.to(dev)
        # the counting sort's order inside a run is free: only runs of at
        # most two ENTRIES have a fixed sum across regroupings
        two = torch.bincount(tb.idx.long(), minlength=tb.rows) <= 2
        sel = fixed & two.to(dev)
        assert same_bits(outs[0][i][sel], outs[1][i][sel])
        for o in outs:
            N.within(o[i], ref, tol, f"K13 dense gradient ({tag})",
                     f"{case.name()} _scatter_embedding_grads")


# ---------------------------------------------------------------------------
# K1/K2


@pytest.mark.parametrize("TS,PS,M", [(104, 40, 1003), (136, 104, 1003),
                                     (8, 8, 16384 * 4 + 1)])
def test_gather_concat_fwd(dev, TS, PS, M):
    g = torch.Generator().manual_seed(TS + PS + M)
    T, P = N.T_ROWS, N.P_ROWS
    KP = N.round_up(2 * TS + PS, 32)
    term = torch.randn(T, TS, generator=g).to(bf16)
    path = torch.randn(P, PS, generator=g).to(bf16)
    s = torch.randint(0, T, (M,), generator=g, dtype=torch.int32)
    p = torch.randint(0, P, (M,), generator=g, dtype=torch.int32)
    e = torch.randint(0, T, (M,), generator=g, dtype=torch.int32)
    s[0], e[0], p[0] = 0, T - 1, P - 1
    s[M - 1], e[M - 1], p[M - 1] = T - 1, 0, 0
    ref = N.gather_concat_ref(s, p, e, term, path, KP)
    assert all_zero(ref[:, 2 * TS + PS:]) and KP > 2 * TS + PS
    outs = []
    for _ in range(2):
        out = nans((M, KP), bf16, dev)
        ext().gather_concat_fwd(s.to(dev), p.to(dev), e.to(dev), term.to(dev),
                                path.to(dev), out)
        outs.append(out.cpu())
    assert same_bits(outs[0], outs[1])
    assert same_bits(outs[0], ref)


# ---------------------------------------------------------------------------
# K16 and the fp32 kernels


def to_dev(st, dev):
    return {k: v.to(dev).clone() for k, v in st.items()}


def set_pow(hp, t, dev):
    return torch.tensor(hp.pow_at(t), dtype=torch.float64, device=dev)


def bf16_steps(dev, n, t, wd, where, steps=3):
    hp = N.Hyper(wd=wd)
    st = N.adam_state(n, bf16)
    cur = dict(p=st["p"], m=st["m"], v=st["v"])
    bc_pow = set_pow(hp, t, dev)
    g = st["g"].to(dev)
    for k in range(steps):
        if k:
            ext().adam_tick(bc_pow, hp.args[1], hp.args[2])
        pw = tuple(bc_pow.cpu().tolist())
        runs = []
        for _ in range(2):
            x = to_dev(cur, dev)
            param = nans((n,), bf16, dev)
            ext().adam_step_bf16(param, g, x["p"], x["m"], x["v"], bc_pow,
                                 *hp.args)
            runs.append(dict(x, param=param))
        for name in runs[0]:
            assert same_bits(runs[0][name], runs[1][name]), (where, name)
        new = {k_: v.cpu() for k_, v in runs[0].items()}
        N.adam_check(f"{where} step {t + k}", cur, new, N.d(st["g"]), pw, hp,
                     "adam_step_bf16", scalar_from=n - n % 4)
        cur = dict(p=new["p"], m=new["m"], v=new["v"])
    if wd == 0.0:
        assert cur["p"][0] == st["p"][0]  # g = 0, m = v = 0: never moved


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_bf16(dev, t, wd):
    for n in (4, 5, 1023, 4097):
        bf16_steps(dev, n, t, wd, f"n={n} t={t} wd={wd}")


@pytest.mark.parametrize("ilp", ["1", "2", "4"])
def test_adam_bf16_grid_stride_and_ilp(dev, monkeypatch, ilp):
    monkeypatch.setenv("C2V_ADAM_GRID", "1")
    monkeypatch.setenv("C2V_ADAM_ILP", ilp)
    assert GRID1_N > 2 * 256 * 4 * 4 and GRID1_N % 4
    for t, wd in ((1, 0.01), (1000, 0.0)):
        bf16_steps(dev, GRID1_N, t, wd,
                   f"n={GRID1_N} t={t} wd={wd} GRID=1 ILP={ilp}", steps=2)


def test_adam_bf16_temporal_loads(dev, monkeypatch):
    monkeypatch.setenv("C2V_ADAM_NT", "0")
    for n in (5, 4097):
        bf16_steps(dev, n, 2, 0.01, f"n={n} t=2 wd=0.01 NT=0", steps=2)
    monkeypatch.setenv("C2V_ADAM_GRID", "1")
    bf16_steps(dev, GRID1_N, 2, 0.01, f"n={GRID1_N} t=2 wd=0.01 NT=0 GRID=1",
               steps=1)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_f32(dev, t, wd):
    hp = N.Hyper(wd=wd)
    for n in (1, 5, 1000, 4096 * 256 + 77):
        st = N.adam_state(n, f32)
        cur = dict(p=st["p"], m=st["m"], v=st["v"])
        bc_pow = set_pow(hp, t, dev)
        pw = tuple(bc_pow.cpu().tolist())
        g = st["g"].to(dev)
        runs = []
        for _ in range(2):
            x = to_dev(cur, dev)
            ext().adam_step_f32(x["p"], g, x["m"], x["v"], bc_pow, *hp.args)
            runs.append(x)
        for name in runs[0]:
            assert same_bits(runs[0][name], runs[1][name]), name
        N.adam_check(f"n={n} t={t} wd={wd}", cur,
                     {k: v.cpu() for k, v in runs[0].items()}, N.d(st["g"]),
                     pw, hp, "adam_step_f32", scalar_from=0)


MULTI = ((1, 3, 255, 256, 257, 1000, 4097, 5),
         (1, 3, 255, 256, 257, 1024, 7, 4096 * 256 + 100))


@pytest.mark.parametrize("sizes", MULTI, ids=["small", "grid-stride"])
@pytest.mark.parametrize("t,wd", [(1, 0.0), (2, 0.01), (1000, 0.01)])
def test_adam_f32_multi(dev, sizes, t, wd):
    assert len(sizes) == 8
    hp = N.Hyper(wd=wd)
    states = [N.adam_state(n, f32, seed=i) for i, n in enumerate(sizes)]
    bc_pow = set_pow(hp, t, dev)
    pw = tuple(bc_pow.cpu().tolist())
    runs = []
    for _ in range(2):
        xs = [to_dev(s, dev) for s in states]
        ext().adam_step_f32_multi([x["p"] for x in xs], [x["g"] for x in xs],
                                  [x["m"] for x in xs], [x["v"] for x in xs],
                                  bc_pow, *hp.args)
        runs.append(N.multi_concat(xs))
    for name in runs[0]:
        assert same_bits(runs[0][name], runs[1][name]), name
    old = N.multi_concat(states)
    new = {k: v.cpu() for k, v in runs[0].items() if k != "g"}
    N.adam_check(f"sizes={sizes[-3:]} t={t} wd={wd}", old, new,
                 N.d(old["g"]), pw, hp, "adam_step_f32_multi", scalar_from=0)


# ---------------------------------------------------------------------------
# FusedAdam


def _fused_adam(params, wd=0.01):
    from code2vec_amd.engine.optim import FusedAdam
    return FusedAdam(params, lr=0.01, weight_decay=wd)


def _snapshot(optim, params):
    out = []
    for p in params:
        st = optim.state[p]
        master = st["master"] if st["master"] is not None else p.data.view(-1)
        out.append(dict(p=master.detach().cpu().clone(),
                        m=st["m"].cpu().clone(), v=st["v"].cpu().clone()))
    return out


def _judge_step(optim, params, before, grads64, where, kernels):
    hp = N.Hyper(lr=optim.lr, b1=optim.beta1, b2=optim.beta2, eps=optim.eps,
                 wd=optim.weight_decay)
    pw = tuple(optim.bc_pow.cpu().tolist())
    after = _snapshot(optim, params)
    for i, p in enumerate(params):
        new = dict(after[i])
        n = p.numel()
        if p.dtype == bf16:
            new["param"] = p.data.detach().cpu().view(-1)
            sf = n - n % 4
        else:
            sf = 0
        N.adam_check(f"{where} param {i}", before[i], new, grads64[i], pw, hp,
                     kernels[i], scalar_from=sf)
    return hp, pw


def test_fused_adam_step_nine_fp32_params_and_bc_pow(dev):
    g = torch.Generator().manual_seed(77)
    sizes = (1, 3, 255, 256, 257, 1000, 100, 5, 130)
    params = []
    for n in sizes:
        p = torch.nn.Parameter((torch.randn(n, generator=g) * 0.1).to(dev))
        p.grad = (torch.randn(n, generator=g) * 0.01).to(dev)
        params.append(p)
    optim = _fused_adam(params)
    kernels = ["FusedAdam.step (multi)"] * 8 + ["FusedAdam.step (single)"]
    grads64 = [N.d(p.grad).view(-1) for p in params]
    for t in (1, 2, 3):
        before = _snapshot(optim, params)
        optim.step()
        hp, pw = _judge_step(optim, params, before, grads64, f"t={t}",
                             kernels)
        for got, b in zip(pw, (hp.b1, hp.b2)):
            assert abs(got - b ** t) <= 1e-15 * b ** t, (t, got)
    assert optim.step_count == 3


def test_fused_adam_step_rows(dev):
    g = torch.Generator().manual_seed(78)
    R, W = 37, 104
    p = torch.nn.Parameter((torch.randn(R, W, generator=g) * 0.1)
                           .to(bf16).to(dev))
    other = torch.nn.Parameter(torch.randn(7, generator=g).to(dev))
    other.grad = torch.randn(7, generator=g).to(dev)
    grad = (torch.randn(R, W, generator=g) * 0.01).to(bf16).to(dev)
    optim = _fused_adam([p, other])
    ranges = ((0, 5), (5, 6), (20, 37))
    touched = torch.zeros(R, dtype=torch.bool)
    for lo, hi in ranges:
        touched[lo:hi] = True
    for t in (1, 2):
        before = _snapshot(optim, [p])[0]
        param_before = p.data.detach().cpu().clone()
        optim.step(exclude_ids={id(p)})
        for lo, hi in ranges:
            optim.step_rows(p, grad, lo, hi)
        after = _snapshot(optim, [p])[0]
        hp = N.Hyper(wd=0.01)
        pw = tuple(optim.bc_pow.cpu().tolist())
        sel = touched[:, None].expand(R, W).reshape(-1)
        old = {k: v[sel] for k, v in before.items()}
        new = {k: v[sel] for k, v in after.items()}
        new["param"] = p.data.detach().cpu().view(-1)[sel]
        N.adam_check(f"t={t}", old, new, N.d(grad).view(-1)[sel], pw, hp,
                     "FusedAdam.step_rows")
        for k in before:
            assert same_bits(before[k][~sel], after[k][~sel]), k
        assert same_bits(param_before[~touched], p.data.cpu()[~touched])


def test_fused_adam_graph_replay_advances_bias_correction(dev):
    g = torch.Generator().manual_seed(79)
    pb = torch.nn.Parameter((torch.randn(4097, generator=g) * 0.1)
                            .to(bf16).to(dev))
    pb.grad = (torch.randn(4097, generator=g) * 0.01).to(bf16).to(dev)
    fs = []
    for n in (3, 257, 1000):
        q = torch.nn.Parameter((torch.randn(n, generator=g) * 0.1).to(dev))
        q.grad = (torch.randn(n, generator=g) * 0.01).to(dev)
        fs.append(q)
    params = [pb] + fs
    optim = _fused_adam(params)
    kernels = ["graph replay (bf16)"] + ["graph replay (multi)"] * 3
    grads64 = [N.d(p.grad).view(-1) for p in params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        optim.step()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        optim.step()
    torch.cuda.synchronize()
    # neither the warm-up nor the capture is judged: start from here
    for replay in range(3):
        before = _snapshot(optim, params)
        pw0 = optim.bc_pow.cpu().tolist()
        graph.replay()
        torch.cuda.synchronize()
        hp, pw = _judge_step(optim, params, before, grads64,
                             f"replay {replay}", kernels)
        for got, was, b in zip(pw, pw0, (hp.b1, hp.b2)):
            assert got < was and abs(got - was * b) <= 1e-15 * was, replay


# ---------------------------------------------------------------------------
# K16b


def table_state(tb, seed=11):
    st = N.adam_state(tb.rows * tb.S, bf16, seed=seed)
    return dict(p=st["p"], m=st["m"], v=st["v"])


def k16b_reference(case, tag):
    """(g64, dg): the fp64 gradient and the bound on the kernel's unstored
    rounded one; exact (dg None) for integer gradients."""
    ref, tol, _, _ = N.table_ref(case, tag)
    if case.grad == "int":
        return N.d(ref.float().to(bf16)), None
    return ref, tol


def judge_k16b(case, tag, old, runs, pw, hp, kernel, where):
    tb = case.tables[tag]
    fixed = tb.fixed_order.to(runs[0]["p"].device)
    for name in runs[0]:
        a = runs[0][name].view(tb.rows, tb.S)[fixed]
        b = runs[1][name].view(tb.rows, tb.S)[fixed]
        assert same_bits(a, b), (where, name)
    g64, dg = k16b_reference(case, tag)
    for r in runs:
        new = {k: v.cpu().view(-1) for k, v in r.items()}
        N.adam_check(where, old, new, g64, pw, hp, kernel, dg=dg)


def run_k16b_single(case, tag, rec, gout, dev, thr, hp, t, where):
    tb = case.tables[tag]
    sorted_idx, perm, counts, cursor = rec
    old = table_state(tb)
    bc_pow = set_pow(hp, t, dev)
    pw = tuple(bc_pow.cpu().tolist())
    scratch = torch.zeros(tb.rows, tb.S, device=dev)
    runs = []
    for _ in range(2):
        x = to_dev(old, dev)
        cnt = counts.clone()
        param = nans((tb.rows, tb.S), bf16, dev)
        ext().embed_scatter_heavy(sorted_idx, perm, cnt, gout, scratch,
                                  case.M, case.KP, tb.off0, tb.off1, thr)
        ext().adam_table_bf16(param, gout, perm, cnt, cursor, scratch, x["p"],
                              x["m"], x["v"], bc_pow, case.M, case.KP,
                              tb.off0, tb.off1, thr, *hp.args)
        assert all_zero(cnt) and all_zero(scratch), where
        runs.append(dict(x, param=param))
    judge_k16b(case, tag, old, runs, pw, hp,
               f"K16b adam_table_bf16 ({tag})", where)


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_k16b_table_adam(dev, monkeypatch, key):
    case = N.scatter_case(*key)
    gout = case.gout.to(dev)
    rec = records(case, "group_by_index", dev, monkeypatch)
    for t, wd in ((1, 0.0), (1000, 0.01)):
        hp = N.Hyper(wd=wd)
        for tag in ("term", "path"):
            run_k16b_single(case, tag, rec[tag], gout, dev, case.thr, hp, t,
                            f"{case.name()} t={t} wd={wd}")


def test_k16b_variant_cases(dev, monkeypatch):
    """One case per width; also the body of the child process that covers
    C2V_TABLE_ADAM_ILP=2 / C2V_TABLE_ADAM_DEPTH=4 (read once per process)."""
    variant = (f"ILP={os.environ.get('C2V_TABLE_ADAM_ILP', '1')} "
               f"DEPTH={os.environ.get('C2V_TABLE_ADAM_DEPTH', '2')}")
    hp = N.Hyper(wd=0.01)
    for key in (("odd", 32, 8, 8, "real"), ("even", 64, 104, 40, "real"),
                ("odd", 64, 136, 104, "real"), ("odd", 64, 104, 40, "int")):
        case = N.scatter_case(*key)
        gout = case.gout.to(dev)
        rec = records(case, "group_by_index", dev, monkeypatch)
        for tag in ("term", "path"):
            run_k16b_single(case, tag, rec[tag], gout, dev, case.thr, hp, 2,
                            f"{case.name()} t=2 wd=0.01 {variant}")
    print(f"k16b variant {variant}")


def test_k16b_ilp2_depth4_in_a_child_process():
    if os.environ.get("C2V_TABLE_ADAM_ILP") == "2":
        return  # this process already runs that variant
    target = f"{os.path.abspath(__file__)}::test_k16b_variant_cases"
    res = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-s", "-x", "-m", "gpu",
         "-p", "no:cacheprovider", target],
        env=dict(os.environ, C2V_TABLE_ADAM_ILP="2", C2V_TABLE_ADAM_DEPTH="4"),
        capture_output=True, text=True, timeout=600,
        cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
    assert "1 passed" in res.stdout
    assert "k16b variant ILP=2 DEPTH=4" in res.stdout


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
def test_k16b_pair_form(dev, monkeypatch, key):
    """embed_scatter_heavy_pair + adam_table_bf16_keep_counts x2 +
    clear_i32_pair on group_tables records."""
    case = N.scatter_case(*key)
    gout = case.gout.to(dev)
    rec = records(case, "group_tables bucket", dev, monkeypatch)
    hp = N.Hyper(wd=0.01)
    bc_pow = set_pow(hp, 2, dev)
    pw = tuple(bc_pow.cpu().tolist())
    old = {tag: table_state(case.tables[tag]) for tag in rec}
    scratch = {tag: torch.zeros(tb.rows, tb.S, device=dev)
               for tag, tb in case.tables.items()}
    runs = {tag: [] for tag in rec}
    for _ in range(2):
        cnt = {tag: rec[tag][2].clone() for tag in rec}
        t, p = rec["term"], rec["path"]
        ext().embed_scatter_heavy_pair(
            t[0], t[1], cnt["term"], scratch["term"], p[0], p[1], cnt["path"],
            scratch["path"], gout, case.M, case.KP, case.thr)
        for tag in ("term", "path"):
            tb = case.tables[tag]
            x = to_dev(old[tag], dev)
            param = nans((tb.rows, tb.S), bf16, dev)
            ext().adam_table_bf16_keep_counts(
                param, gout, rec[tag][1], cnt[tag], rec[tag][3], scratch[tag],
                x["p"], x["m"], x["v"], bc_pow, case.M, case.KP, tb.off0,
                tb.off1, case.thr, *hp.args)
            assert torch.equal(cnt[tag], rec[tag][2])  # kept
            runs[tag].append(dict(x, param=param))
        ext().clear_i32_pair(cnt["term"], cnt["path"])
        for tag in rec:
            assert all_zero(cnt[tag]) and all_zero(scratch[tag])
    for tag in rec:
        judge_k16b(case, tag, old[tag], runs[tag], pw, hp,
                   f"K16b pair form ({tag})", f"{case.name()} t=2 wd=0.01")


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("key", [KEYS[4], KEYS[11], KEYS[12], KEYS[14]],
                         ids=[KEY_IDS[4], KEY_IDS[11], KEY_IDS[12],
                              KEY_IDS[14]])
def test_table_adam_deferred(dev, monkeypatch, key, paired):
    """Fn.table_adam_deferred on DeferredTableGrad records, alone and as the
    two records of one grouping (production threshold)."""
    case = N.scatter_case(*key)
    assert case.thr == Fn._TABLE_ADAM_HEAVY
    gout = case.gout.to(dev)
    hp = N.Hyper(wd=0.01)
    bc_pow = set_pow(hp, 2, dev)
    pw = tuple(bc_pow.cpu().tolist())
    old = {tag: table_state(tb) for tag, tb in case.tables.items()}
    runs = {tag: [] for tag in old}
    for _ in range(2):
        rec = records(case, "group_tables bucket", dev, monkeypatch)
        pair = Fn._GroupedPair() if paired else None
        drecs = {}
        for tag, tb in case.tables.items():
            sorted_idx, perm, counts, cursor = rec[tag]
            r = Fn.DeferredTableGrad(tag, gout, perm, counts, cursor,
                                     sorted_idx, case.M, case.KP, tb.off0,
                                     tb.off1, (tb.rows, tb.S))
            if paired:
                r.pair = pair
                pair.recs[tag] = r
            drecs[tag] = r
        for tag, tb in case.tables.items():
            x = to_dev(old[tag], dev)
            param = nans((tb.rows, tb.S), bf16, dev)
            Fn.table_adam_deferred(param, x["p"], x["m"], x["v"], drecs[tag],
                                   bc_pow, *hp.args)
            runs[tag].append(dict(x, param=param))
        for tag, tb in case.tables.items():
            assert all_zero(rec[tag][2]), tag
            assert all_zero(Fn._scratch_f32(tag, (tb.rows, tb.S), dev)), tag
    for tag, tb in case.tables.items():
        # the two runs regrouped: only runs of at most two entries keep
        # their addition order
        g64, dg = k16b_reference(case, tag)
        for r in runs[tag]:
            new = {k: v.cpu().view(-1) for k, v in r.items()}
            N.adam_check(f"{case.name()} t=2 wd=0.01 paired={paired}",
                         old[tag], new, g64, pw, hp,
                         f"Fn.table_adam_deferred ({tag})", dg=dg)
        two = (torch.bincount(tb.idx.long(), minlength=tb.rows) <= 2).to(dev)
        for name in runs[tag][0]:
            a = runs[tag][0][name].view(tb.rows, tb.S)[two]
            b = runs[tag][1][name].view(tb.rows, tb.S)[two]
            assert same_bits(a, b), (tag, name)
