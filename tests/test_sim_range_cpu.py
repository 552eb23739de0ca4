"""Range search on CPU: the sim_range oracle against an fp64 brute-force
loop, exclude / after, argument errors, max_pairs, the composed path,
CodeVectorIndex's range methods (duplicate pairs and groups on an index
whose scores are known by construction) and tools/similar.py --threshold /
--groups."""

import json
import os
import subprocess
import sys

import pytest
import torch

from code2vec_amd.engine.similar import CodeVectorIndex
from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R
from sim_range_rule import (assert_csr_equal, check_csr, clustered_int_index,
                            int_case)
from tools import similar as similar_cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_force(q, db, t, exclude=None, after=None):
    """CSR from fp64 scores, pair by pair (integer data: exact)."""
    S = (q.double() @ db.double().t()).tolist()
    offsets, rows, scores = [0], [], []
    for i, srow in enumerate(S):
        for j, s in enumerate(srow):
            if exclude is not None and int(exclude[i]) == j:
                continue
            if after is not None and j <= int(after[i]):
                continue
            if s >= t:
                rows.append(j)
                scores.append(s)
        offsets.append(len(rows))
    return (torch.tensor(offsets), torch.tensor(rows, dtype=torch.int64),
            torch.tensor(scores, dtype=torch.float32))


@pytest.mark.parametrize("nq,N,EP,t", [(37, 1000, 128, 40.0),
                                       (33, 4099, 128, 96.0),
                                       (20, 300, 512, 100.0)])
def test_reference_equals_brute_force(nq, N, EP, t):
    q, db = int_case(nq, N, EP)
    got = R.sim_range(q, db, t)
    assert_csr_equal(got, brute_force(q, db, t))
    check_csr(*got, nq, N)
    if (nq, N) == (37, 1000):
        # tie-rich: scores exactly at the threshold are in
        assert got[1].numel() == 7117
        assert int((got[2] == t).sum()) == 235
        assert int(got[0].diff().max()) == 222
    # fp32 input scores the same numbers
    assert_csr_equal(R.sim_range(q.float(), db.float(), t), got)


def test_exclude_and_after():
    nq, N, t = 37, 1000, 40.0
    q, db = int_case(nq, N, 128)
    g = torch.Generator().manual_seed(3)
    base = R.sim_range(q, db, t)
    # exclude: a reported row of every query that has one, -1 elsewhere
    ex = torch.full((nq,), -1, dtype=torch.int64)
    for i in range(nq):
        a, b = int(base[0][i]), int(base[0][i + 1])
        if b > a and i % 3:
            ex[i] = base[1][(a + b) // 2]
    af = torch.randint(-1, N, (nq,), generator=g)
    af[0], af[1], af[2] = -1, N - 1, N - 2
    for e, a in ((ex, None), (None, af), (ex, af)):
        got = R.sim_range(q, db, t, exclude=e, after=a)
        assert_csr_equal(got, brute_force(q, db, t, e, a))
        check_csr(*got, nq, N, e, a)
    none = torch.full((nq,), -1, dtype=torch.int64)
    assert_csr_equal(R.sim_range(q, db, t, exclude=none, after=none), base)
    got = R.sim_range(q, db, t, after=af)
    assert int(got[0][2]) == int(got[0][1])  # after = N - 1: nothing left


def test_empty_results():
    q, db = int_case(37, 1000, 128)
    S = q.float() @ db.float().t()
    assert float(S.max()) == 182.0
    off, rows, scores = R.sim_range(q, db, 183.0)
    assert off.tolist() == [0] * 38 and rows.numel() == 0 \
        and scores.numel() == 0
    assert rows.dtype == torch.int64 and scores.dtype == torch.float32
    assert R.sim_range(q, db, 182.0)[1].numel() >= 1
    # zeroed queries: empty segments among full ones
    q = q.clone()
    q[[0, 5, 36]] = 0
    got = R.sim_range(q, db, 40.0)
    assert_csr_equal(got, brute_force(q, db, 40.0))
    counts = got[0].diff()
    assert counts[[0, 5, 36]].tolist() == [0, 0, 0] and int(counts[1]) > 0
    # no queries at all
    off, rows, scores = R.sim_range(q[:0], db, 40.0)
    assert off.tolist() == [0] and rows.numel() == 0


def test_argument_errors():
    q, db = int_case(3, 16, 32)
    i64 = torch.zeros(3, dtype=torch.int64)
    bad = [
        dict(q=q[0]),                                  # not 2-D
        dict(q=torch.zeros(3, 48), db=torch.zeros(16, 48)),  # EP = 48
        dict(db=torch.zeros(16, 64)),                  # mismatched EP
        dict(db=db[:0]),                               # empty index
        dict(threshold=float("nan")),
        dict(threshold=float("inf")),
        dict(threshold=1e39),                          # inf in fp32
        dict(threshold="high"),
        dict(exclude=i64[:2]),
        dict(exclude=i64.int()),
        dict(exclude=i64.view(3, 1)),
        dict(after=i64[:2]),
        dict(after=i64.float()),
        dict(max_pairs=-1),
        dict(max_pairs=1.5),
    ]
    for fn in (R.sim_range, Fn.sim_range, Fn.sim_range_composed):
        for kw in bad:
            args = dict(q=q, db=db, threshold=0.0)
            args.update(kw)
            with pytest.raises(ValueError):
                fn(**args)
    with pytest.raises(ValueError):
        R.check_sim_range_args(q, db, float("-inf"))


def test_max_pairs():
    q, db = int_case(37, 1000, 128)
    for fn in (R.sim_range, Fn.sim_range):
        assert fn(q, db, 40.0, max_pairs=7117)[1].numel() == 7117
        with pytest.raises(ValueError) as e:
            fn(q, db, 40.0, max_pairs=7116)
        msg = str(e.value)
        assert "7117" in msg and "7116" in msg and "40.0" in msg
        assert isinstance(e.value, R.TooManyPairs) and e.value.total == 7117
        assert fn(q, db, 183.0, max_pairs=0)[1].numel() == 0
    with pytest.raises(ValueError, match="max_pairs = 100"):
        Fn.sim_range_composed(q, db, 40.0, max_pairs=100)


def test_functional_on_cpu_is_the_reference_and_composed_agrees(monkeypatch):
    g = torch.Generator().manual_seed(2)
    q = torch.randn(9, 64, generator=g)
    db = torch.randn(200, 64, generator=g)
    ex = torch.arange(9)
    for dtype in (torch.float32, torch.bfloat16):
        for e, a in ((None, None), (ex, None), (None, ex), (ex, ex + 3)):
            got = Fn.sim_range(q.to(dtype), db.to(dtype), 4.0, e, a)
            want = R.sim_range(q.to(dtype), db.to(dtype), 4.0, e, a)
            assert_csr_equal(got, want)
    assert want[1].numel() > 0
    # the composed path keeps the same contract (exact on integer data),
    # also when it has to cut the queries into chunks
    qi, dbi = int_case(37, 1000, 128)
    af = torch.arange(37) * 20
    for chunk_bytes in (1 << 30, 4 * 1000 * 5):
        monkeypatch.setattr(Fn, "_SIM_COMPOSED_SCORE_BYTES", chunk_bytes)
        for e, a in ((None, None), (af, None), (None, af), (af + 1, af)):
            assert_csr_equal(Fn.sim_range_composed(qi, dbi, 40.0, e, a),
                             R.sim_range(qi, dbi, 40.0, e, a))
        assert_csr_equal(Fn.sim_range_composed(qi[:0], dbi, 40.0),
                         R.sim_range(qi[:0], dbi, 40.0))


def test_slice_and_wave_helpers():
    assert Fn.sim_range_default_nsplit(1, 16) == 1
    assert Fn.sim_range_default_nsplit(64, 20011) > 1
    assert Fn.sim_range_slice_rows(1000, 3) == 336
    assert Fn.sim_range_wave_rows(1000, 3) == 96  # ceil(21 / 4) tiles
    assert Fn.sim_range_wave_rows(1000, 1) == 256
    for N, nsplit in ((1000, 3), (20011, 19), (17, 1), (605945, 256)):
        s, w = Fn.sim_range_slice_rows(N, nsplit), \
            Fn.sim_range_wave_rows(N, nsplit)
        assert s % Fn.SIM_ROW_TILE == 0 and w % Fn.SIM_ROW_TILE == 0
        assert s * nsplit >= N and w * Fn.SIM_RANGE_WAVES >= s


# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clustered():
    v, t, family, pair, chain = clustered_int_index()
    names = [f"m{i}" for i in range(v.shape[0])]
    index = CodeVectorIndex(v, names, "cpu", metric="dot")
    S = (v.double() @ v.double().t())
    want = [(i, j, float(S[i, j])) for i in range(len(names))
            for j in range(i + 1, len(names)) if S[i, j] >= t]
    return dict(index=index, v=v, t=t, family=family, pair=pair,
                chain=chain, names=names, S=S, pairs=want)


def test_duplicate_pairs_equal_brute_force(clustered):
    index, t = clustered["index"], clustered["t"]
    assert index.EP == 64 and index.E == 40
    i, j, s = index.duplicate_pairs(t)
    assert i.dtype == torch.int64 and j.dtype == torch.int64 \
        and s.dtype == torch.float32 and not i.is_cuda
    got = list(zip(i.tolist(), j.tolist(), s.tolist()))
    assert got == clustered["pairs"]
    assert len(got) == 190 + 1 + 2  # C(20, 2) + the pair + the chain's two
    assert bool((i < j).all())
    for chunk in (7, 1, 96, 1000):
        again = index.duplicate_pairs(t, query_chunk=chunk)
        for a, b in zip(again, (i, j, s)):
            assert torch.equal(a, b)
    with pytest.raises(ValueError) as e:
        index.duplicate_pairs(t, query_chunk=7, max_pairs=192)
    assert "192" in str(e.value) and isinstance(e.value, R.TooManyPairs)
    assert index.duplicate_pairs(t, query_chunk=7, max_pairs=193)[0].numel() \
        == 193
    with pytest.raises(ValueError):
        index.duplicate_pairs(t, query_chunk=0)
    with pytest.raises(ValueError):
        index.duplicate_pairs(float("nan"))
    empty = index.duplicate_pairs(161.0)
    assert all(x.numel() == 0 for x in empty)


def test_duplicate_groups(clustered):
    index, t = clustered["index"], clustered["t"]
    groups = index.duplicate_groups(t)
    # ordered by smallest member; single linkage puts A and C together
    # though A.C = 96 < t
    assert groups == [clustered["chain"], clustered["family"],
                      clustered["pair"]]
    a, _, c = clustered["chain"]
    assert float(clustered["S"][a, c]) < t
    assert len(groups[1]) == 20  # beyond any k <= 16
    assert index.duplicate_groups(t, query_chunk=7) == groups
    assert index.duplicate_groups(161.0) == []
    # at 96 the chain closes into a triangle; the groups stay the same
    assert index.duplicate_groups(96.0) == groups


def test_components_long_chain():
    from code2vec_amd.engine.similar import _components

    # a path 9 - 8 - ... - 0 listed against the direction of propagation,
    # plus a separate edge; node 10 has no partner
    i = torch.tensor(list(range(9)) + [11])
    j = torch.tensor(list(range(1, 10)) + [12])
    assert _components(i.flip(0), j.flip(0), 13) == [list(range(10)),
                                                     [11, 12]]
    assert _components(i[:0], j[:0], 13) == []


def test_neighbors_within_and_range_search(clustered):
    index, t, fam = clustered["index"], clustered["t"], clustered["family"]
    rows = [fam[0], fam[7], clustered["pair"][1], clustered["chain"][1], 0]
    off, r, s = index.neighbors_within(rows, t)
    seg = [r[off[k]:off[k + 1]].tolist() for k in range(len(rows))]
    assert seg[0] == fam[1:] and seg[1] == fam[:7] + fam[8:]
    assert seg[2] == [clustered["pair"][0]]
    assert seg[3] == [clustered["chain"][0], clustered["chain"][2]]
    assert seg[4] == []
    assert s[:19].tolist() == [160.0] * 19
    # the same rows as plain queries find themselves too
    off2, r2, _ = index.range_search(clustered["v"][rows], t)
    assert r2[off2[0]:off2[1]].tolist() == fam
    assert r2[off2[4]:off2[5]].tolist() == []
    # exclude_rows is neighbors_within's exclusion
    got = index.range_search(clustered["v"][rows], t,
                             exclude_rows=torch.tensor(rows))
    assert_csr_equal(got, (off, r, s))
    with pytest.raises(ValueError):
        index.neighbors_within([96], t)
    with pytest.raises(ValueError):
        index.range_search(clustered["v"][rows], t, exclude_rows=[1, 2])
    with pytest.raises(ValueError):
        index.range_search(clustered["v"][:, :39], t)
    with pytest.raises(ValueError):
        index.neighbors_within(rows, t, max_pairs=3)


def test_save_load_roundtrip(clustered, tmp_path):
    index, t = clustered["index"], clustered["t"]
    path = tmp_path / "index.pt"
    index.save(str(path))
    again = CodeVectorIndex.load(str(path), "cpu")
    assert again.metric == "dot"
    assert again.duplicate_groups(t) == index.duplicate_groups(t)
    for a, b in zip(again.duplicate_pairs(t), index.duplicate_pairs(t)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
def write_vec(path, names, vectors):
    with open(path, "w", encoding="utf-8") as f:
        f.write(f"{len(names)}\t{len(vectors[0])}\n")
        for n, v in zip(names, vectors):
            f.write(n + "\t" + " ".join(str(float(x)) for x in v) + "\n")


def run_cli(argv):
    return similar_cli.main(argv + ["--no_cuda"])


def read_jsonl(path):
    return [json.loads(ln) for ln in open(path, encoding="utf-8")
            if ln.strip()]


def cli_error(argv):
    with pytest.raises(SystemExit) as e:
        run_cli(argv)
    msg = str(e.value)
    assert msg.startswith("similar: ") and "\n" not in msg
    return msg


@pytest.fixture
def files(clustered, tmp_path):
    v, names = clustered["v"], clustered["names"]
    vec = tmp_path / "code.vec"
    write_vec(vec, names, v.tolist())
    fam, pair = clustered["family"], clustered["pair"]
    qrows = [fam[3], pair[0], 0]
    qv = tmp_path / "query.vec"
    write_vec(qv, ["qa", "qb", "qc"], v[qrows].tolist())
    preds = tmp_path / "preds.jsonl"
    with open(preds, "w", encoding="utf-8") as f:
        for k, r in enumerate(qrows):
            f.write(json.dumps({"id": k, "expected": f"p{k}",
                                "vector": v[r].tolist()}) + "\n")
    return dict(vec=str(vec), qv=str(qv), preds=str(preds), dir=tmp_path,
                qrows=qrows)


def check_lines(lines, names):
    for ln in lines:
        assert set(ln) == {"query", "name", "neighbors"}
        for n in ln["neighbors"]:
            assert set(n) == {"row", "name", "score"}
            assert names[n["row"]] == n["name"]
        key = [(-n["score"], n["row"]) for n in ln["neighbors"]]
        assert key == sorted(key)  # best first, equal scores by row


def test_cli_threshold_three_query_modes(clustered, files):
    names, fam, pair = clustered["names"], clustered["family"], \
        clustered["pair"]
    base = ["--vectors", files["vec"], "--metric", "dot", "--threshold",
            "120"]
    for src, qnames in ((["--query_vectors", files["qv"]],
                         ["qa", "qb", "qc"]),
                        (["--query_predictions", files["preds"]],
                         ["p0", "p1", "p2"])):
        out = files["dir"] / "a.jsonl"
        assert run_cli(base + src + ["--out", str(out)]) == 0
        lines = read_jsonl(out)
        check_lines(lines, names)
        assert [ln["name"] for ln in lines] == qnames
        assert [n["row"] for n in lines[0]["neighbors"]] == fam
        assert [n["score"] for n in lines[0]["neighbors"]] == [160.0] * 20
        assert [n["row"] for n in lines[1]["neighbors"]] == pair
        assert lines[2]["neighbors"] == []

    out = files["dir"] / "self.jsonl"
    assert run_cli(base + ["--self", "--out", str(out), "--max_pairs",
                           "1000"]) == 0
    lines = read_jsonl(out)
    check_lines(lines, names)
    assert [ln["query"] for ln in lines] == list(range(96))
    for i, ln in enumerate(lines):
        assert ln["name"] == names[i]
        assert i not in [n["row"] for n in ln["neighbors"]]
    assert [n["row"] for n in lines[fam[3]]["neighbors"]] \
        == fam[:3] + fam[4:]
    # the chain's middle: both ends, the better score first
    a, b, c = clustered["chain"]
    assert [n["row"] for n in lines[b]["neighbors"]] == [a, c]
    # best first: at 96 row A sees B (128) before C (96)
    out = files["dir"] / "self96.jsonl"
    assert run_cli(["--vectors", files["vec"], "--metric", "dot",
                    "--threshold", "96", "--self", "--out", str(out)]) == 0
    assert [(n["row"], n["score"])
            for n in read_jsonl(out)[a]["neighbors"]] == [(b, 128.0),
                                                          (c, 96.0)]


def test_cli_groups(clustered, files, capsys):
    out = files["dir"] / "groups.jsonl"
    assert run_cli(["--vectors", files["vec"], "--metric", "dot", "--self",
                    "--threshold", "120", "--groups", "--out",
                    str(out)]) == 0
    lines = read_jsonl(out)
    want = [clustered["chain"], clustered["family"], clustered["pair"]]
    assert len(lines) == 3
    for g, (ln, members) in enumerate(zip(lines, want)):
        assert set(ln) == {"group", "size", "representative", "members"}
        assert ln["group"] == g and ln["size"] == len(members)
        assert ln["representative"] == {"row": members[0],
                                        "name": f"m{members[0]}"}
        assert ln["members"] == [{"row": r, "name": f"m{r}"}
                                 for r in members]
    err = capsys.readouterr().err.strip().splitlines()
    assert len(err) == 1
    assert "96 methods" in err[0] and "3 groups" in err[0] \
        and "22 rows" in err[0]


def test_cli_cosine_lists_a_family_beyond_16(tmp_path):
    """The issue's command line: --self --threshold 0.95 --groups on a
    code.vec with a planted family of 24 scaled copies."""
    g = torch.Generator().manual_seed(8)
    v = torch.randn(60, 20, generator=g)
    fam = list(range(3, 60, 2))[:24]
    scale = torch.linspace(0.5, 4.0, 24).view(-1, 1)
    v[fam] = v[fam[0]].clone() * scale
    names = [f"m{i}" for i in range(60)]
    vec = tmp_path / "code.vec"
    write_vec(vec, names, v.tolist())
    out = tmp_path / "g.jsonl"
    assert run_cli(["--vectors", str(vec), "--self", "--threshold", "0.95",
                    "--groups", "--out", str(out)]) == 0
    lines = read_jsonl(out)
    assert len(lines) == 1 and lines[0]["size"] == 24
    assert [m["row"] for m in lines[0]["members"]] == fam


def test_cli_errors_and_old_command_lines(clustered, files):
    base = ["--vectors", files["vec"], "--metric", "dot"]
    msg = cli_error(base + ["--self", "--k", "3", "--threshold", "120"])
    assert "--k" in msg and "--threshold" in msg
    msg = cli_error(base + ["--query_vectors", files["qv"], "--threshold",
                            "120", "--groups"])
    assert "--groups" in msg and "--self" in msg
    assert "--threshold" in cli_error(base + ["--self", "--groups"])
    assert "--threshold" in cli_error(base + ["--self", "--max_pairs", "5"])
    cli_error(base + ["--self", "--threshold", "nan"])
    msg = cli_error(base + ["--self", "--threshold", "120", "--max_pairs",
                            "10"])
    assert "max_pairs" in msg
    msg = cli_error(base + ["--self", "--threshold", "120", "--groups",
                            "--max_pairs", "10"])
    assert "max_pairs" in msg
    # --k alone is what it was: CodeVectorIndex.search's rows and scores,
    # and 5 neighbours when --k is not given
    index = clustered["index"]
    q = clustered["v"][files["qrows"]]
    for extra, k in ((["--k", "7"], 7), ([], 5)):
        out = files["dir"] / "k.jsonl"
        assert run_cli(base + ["--query_vectors", files["qv"], "--out",
                               str(out)] + extra) == 0
        scores, rows = index.search(q, k)
        lines = read_jsonl(out)
        assert [[n["row"] for n in ln["neighbors"]] for ln in lines] \
            == rows.tolist()
        assert [[n["score"] for n in ln["neighbors"]] for ln in lines] \
            == scores.tolist()
    for k in ("0", "17"):
        assert "1..16" in cli_error(base + ["--self", "--k", k])


@pytest.mark.parametrize("tool,flag", [("bench_sim_range.py", "--hits"),
                                       ("similar.py", "--threshold")])
def test_tools_help_exits_zero(tool, flag):
    res = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", tool), "--help"],
        capture_output=True, text=True, timeout=90, cwd=REPO)
    assert res.returncode == 0, res.stderr[-400:]
    assert flag in res.stdout
