"""Nearest-neighbour search on CPU: the sim_topk oracle, code.vec parsing,
CodeVectorIndex save/load, tools/similar.py in its three query modes and
its error paths, and the train -> predict -> similar chain end to end."""

import json
import os
import subprocess
import sys

import pytest
import torch

from code2vec_amd.engine.similar import CodeVectorIndex, read_code_vec
from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R
from tools import predict as predict_cli
from tools import similar as similar_cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def int_data(nq, N, EP, seed):
    """Integers in [-3, 3]: exact in bf16, sums exact in fp32, tie-rich."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-3, 4, (nq, EP), generator=g).float()
    db = torch.randint(-3, 4, (N, EP), generator=g).float()
    return q, db


def brute_force(q, db, k, exclude=None):
    vals, idx = [], []
    for i in range(q.shape[0]):
        scored = []
        for j in range(db.shape[0]):
            if exclude is not None and int(exclude[i]) == j:
                continue
            s = sum(float(a) * float(b) for a, b in zip(q[i], db[j]))
            scored.append((-s, j))
        scored.sort()
        vals.append([-s for s, _ in scored[:k]])
        idx.append([j for _, j in scored[:k]])
    return vals, idx


def test_reference_equals_brute_force_with_ties_and_exclusion():
    q, db = int_data(5, 40, 32, 0)
    db[7] = db[3]  # exact duplicates: ties beyond the accidental ones
    db[21] = db[3]
    q[0] = db[3]
    k = 6
    vals, idx = R.sim_topk(q, db, k)
    bv, bi = brute_force(q, db, k)
    assert idx.tolist() == bi and vals.tolist() == bv
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64
    pos = {r: p for p, r in enumerate(idx[0].tolist())}
    assert pos[3] < pos[7] < pos[21]  # equal scores: ascending rows

    ex = torch.tensor([3, -1, 0, 39, 7])
    vals, idx = R.sim_topk(q, db, k, ex)
    bv, bi = brute_force(q, db, k, ex)
    assert idx.tolist() == bi and vals.tolist() == bv
    assert 3 not in idx[0].tolist()
    # bf16 input scores the same numbers
    vb, ib = R.sim_topk(q.bfloat16(), db.bfloat16(), k, ex)
    assert torch.equal(vb, vals) and torch.equal(ib, idx)


def test_reference_argument_errors():
    q, db = int_data(3, 16, 32, 1)
    for k in (0, 17):
        with pytest.raises(ValueError):
            R.sim_topk(q, db, k)
    with pytest.raises(ValueError):
        R.sim_topk(q, db[:8], 9)  # k > N
    with pytest.raises(ValueError):
        R.sim_topk(q, db, 16, torch.full((3,), -1))  # k == N with exclude
    with pytest.raises(ValueError):
        R.sim_topk(q, db, 2, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        R.sim_topk(torch.zeros(3, 48), torch.zeros(16, 48), 2)  # EP = 48
    with pytest.raises(ValueError):
        R.sim_topk(q, torch.zeros(16, 64), 2)  # mismatched EP
    with pytest.raises(ValueError):
        R.sim_topk(q[0], db, 2)


def test_functional_on_cpu_is_the_reference():
    g = torch.Generator().manual_seed(2)
    q = torch.randn(9, 64, generator=g)
    db = torch.randn(200, 64, generator=g)
    ex = torch.arange(9)
    for dtype in (torch.float32, torch.bfloat16):
        for e in (None, ex):
            got = Fn.sim_topk(q.to(dtype), db.to(dtype), 7, e)
            want = R.sim_topk(q.to(dtype), db.to(dtype), 7, e)
            assert torch.equal(got[0], want[0])
            assert torch.equal(got[1], want[1])
    # the composed path keeps the same contract (exact on integer data)
    qi, dbi = int_data(9, 200, 64, 3)
    for e in (None, ex, torch.full((9,), -1)):
        got = Fn.sim_topk_composed(qi, dbi, 7, e)
        want = R.sim_topk(qi, dbi, 7, e)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError):
        Fn.sim_topk(q, db, 17)
    assert Fn.sim_topk_default_nsplit(1, 16) == 1
    assert Fn.sim_topk_default_nsplit(64, 20011) > 1
    assert Fn.sim_topk_slice_rows(1000, 3) == 336


# ---------------------------------------------------------------------------
def write_vec(path, names, vectors, count=None):
    with open(path, "w", encoding="utf-8") as f:
        f.write(f"{len(names) if count is None else count}\t"
                f"{len(vectors[0])}\n")
        for n, v in zip(names, vectors):
            f.write(n + "\t" + " ".join(str(float(x)) for x in v) + "\n")


def test_read_code_vec(tmp_path):
    p = tmp_path / "a.vec"
    p.write_text("48\t3\nget|name\t1.0 2.0 3.0\nset\t-0.5 0.25 1e-3\n\n")
    names, vecs = read_code_vec(str(p))
    assert names == ["get|name", "set"]  # 2 rows, whatever the header says
    assert vecs.dtype == torch.float32 and vecs.shape == (2, 3)
    assert torch.equal(vecs, torch.tensor([[1.0, 2.0, 3.0],
                                           [-0.5, 0.25, 1e-3]]))
    bad = tmp_path / "b.vec"
    bad.write_text("2\t3\nget\t1.0 2.0 3.0\nset\t1.0 2.0\n")
    with pytest.raises(ValueError, match="line 3") as e:
        read_code_vec(str(bad))
    assert "2 components" in str(e.value) and "3" in str(e.value)
    with pytest.raises(ValueError, match="line 3"):
        CodeVectorIndex.from_code_vec(str(bad), "cpu")


def make_vectors(N, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, E, generator=g)


def test_index_normalizes_pads_and_rejects():
    v = make_vectors(30, 20, 4)
    v[5] = 0.0
    index = CodeVectorIndex(v, [f"m{i}" for i in range(30)], "cpu")
    assert index.matrix.dtype == torch.bfloat16
    assert index.matrix.shape == (30, 32) and index.E == 20 and index.EP == 32
    assert bool((index.matrix[:, 20:] == 0).all())
    assert bool((index.matrix[5] == 0).all())  # zero stays zero, no NaN
    norms = index.matrix.float().norm(dim=1)
    keep = torch.arange(30) != 5
    assert bool(((norms[keep] - 1).abs() < 0.01).all())
    dot = CodeVectorIndex(v, index.names, "cpu", metric="dot")
    assert torch.equal(dot.matrix[:, :20], v.bfloat16())

    # a scaled copy of a row finds that row first under cosine
    scores, rows = index.search(v[[7, 11]] * 3.5, 3)
    assert rows[:, 0].tolist() == [7, 11]
    assert bool((scores[:, 0] > 0.99).all())
    # scaling by a power of two normalizes to the row's own bits, so the
    # self-excluding search sees the same neighbours one place earlier
    scores, rows = index.search(v[[7, 11]] * 4.0, 3)
    assert rows[:, 0].tolist() == [7, 11]
    s2, r2 = index.neighbors_of_rows([7, 11], 3)
    assert 7 not in r2[0].tolist() and 11 not in r2[1].tolist()
    assert torch.equal(r2[0, :2], rows[0, 1:]) \
        and torch.equal(s2[0, :2], scores[0, 1:])

    bad = v.clone()
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        CodeVectorIndex(bad, index.names, "cpu")
    with pytest.raises(ValueError, match="non-finite"):
        index.search(bad[:4], 2)
    with pytest.raises(ValueError):
        CodeVectorIndex(v, index.names[:-1], "cpu")
    with pytest.raises(ValueError):
        CodeVectorIndex(v, index.names, "cpu", metric="l2")
    with pytest.raises(ValueError):
        index.search(v[:, :19], 2)
    for k in (0, 17):
        with pytest.raises(ValueError):
            index.search(v[:2], k)
    small = CodeVectorIndex(v[:4], index.names[:4], "cpu")
    with pytest.raises(ValueError):
        small.search(v[:2], 5)
    with pytest.raises(ValueError):
        small.neighbors_of_rows([0], 4)


def test_from_code_vec_save_load_roundtrip(tmp_path):
    v = make_vectors(40, 20, 5)
    names = [f"method{i}" for i in range(40)]
    p = tmp_path / "code.vec"
    write_vec(p, names, v.tolist(), count=999)
    index = CodeVectorIndex.from_code_vec(str(p), "cpu")
    assert len(index) == 40 and index.names == names
    q = make_vectors(6, 20, 6)
    want = index.search(q, 5)
    saved = tmp_path / "index.pt"
    index.save(str(saved))
    again = CodeVectorIndex.load(str(saved), "cpu")
    assert again.names == names and again.E == 20 \
        and again.metric == "cosine"
    assert torch.equal(again.matrix, index.matrix)
    got = again.search(q, 5)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    torch.save({"x": 1}, str(tmp_path / "other.pt"))
    with pytest.raises(ValueError):
        CodeVectorIndex.load(str(tmp_path / "other.pt"), "cpu")


# ---------------------------------------------------------------------------
def run_cli(argv):
    return similar_cli.main(argv + ["--no_cuda"])


def read_jsonl(path):
    return [json.loads(ln) for ln in open(path, encoding="utf-8")
            if ln.strip()]


@pytest.fixture
def vec_files(tmp_path):
    v = make_vectors(25, 20, 7)
    names = [f"m{i}" for i in range(25)]
    idx = tmp_path / "code.vec"
    write_vec(idx, names, v.tolist(), count=31)
    qv = tmp_path / "query.vec"
    write_vec(qv, ["qa", "qb", "qc"], (v[[4, 9, 20]] * 2.0).tolist())
    preds = tmp_path / "preds.jsonl"
    with open(preds, "w", encoding="utf-8") as f:
        f.write(json.dumps({"id": 0, "expected": "pa",
                            "vector": v[3].tolist()}) + "\n")
        f.write(json.dumps({"id": 17, "vector": v[8].tolist()}) + "\n")
    return {"index": str(idx), "query": str(qv), "preds": str(preds),
            "dir": tmp_path, "names": names}


def check_rows(rows, nq, k, names):
    assert [r["query"] for r in rows] == list(range(nq))
    for r in rows:
        assert set(r) == {"query", "name", "neighbors"}
        assert len(r["neighbors"]) == k
        sc = [n["score"] for n in r["neighbors"]]
        assert sc == sorted(sc, reverse=True)
        for n in r["neighbors"]:
            assert set(n) == {"row", "name", "score"}
            assert names[n["row"]] == n["name"]


def test_cli_three_query_modes(vec_files):
    d = vec_files["dir"]
    out = d / "a.jsonl"
    assert run_cli(["--vectors", vec_files["index"], "--query_vectors",
                    vec_files["query"], "--k", "4", "--out", str(out),
                    "--save_index", str(d / "idx.pt")]) == 0
    rows = read_jsonl(out)
    check_rows(rows, 3, 4, vec_files["names"])
    assert [r["name"] for r in rows] == ["qa", "qb", "qc"]
    assert [r["neighbors"][0]["row"] for r in rows] == [4, 9, 20]

    out = d / "b.jsonl"
    assert run_cli(["--index", str(d / "idx.pt"), "--query_predictions",
                    vec_files["preds"], "--out", str(out)]) == 0
    rows = read_jsonl(out)
    check_rows(rows, 2, 5, vec_files["names"])  # default k
    assert [r["name"] for r in rows] == ["pa", "17"]
    assert [r["neighbors"][0]["row"] for r in rows] == [3, 8]

    out = d / "c.jsonl"
    assert run_cli(["--vectors", vec_files["index"], "--self", "--k", "16",
                    "--metric", "dot", "--out", str(out)]) == 0
    rows = read_jsonl(out)
    check_rows(rows, 25, 16, vec_files["names"])
    for i, r in enumerate(rows):
        assert r["name"] == f"m{i}"
        assert i not in [n["row"] for n in r["neighbors"]]


def cli_error(argv):
    with pytest.raises(SystemExit) as e:
        run_cli(argv)
    msg = str(e.value)
    assert msg.startswith("similar: ") and "\n" not in msg
    return msg


def test_cli_error_paths(vec_files):
    d = vec_files["dir"]
    base = ["--vectors", vec_files["index"]]
    # no query source, two query sources
    assert "query source" in cli_error(base)
    msg = cli_error(base + ["--self", "--query_vectors", vec_files["query"]])
    assert "--self" in msg and "--query_vectors" in msg
    # no index, two indexes
    cli_error(["--self"])
    cli_error(base + ["--index", "x.pt", "--self"])
    # k out of range; k not below N with --self; k above N
    for k in ("0", "17"):
        assert "1..16" in cli_error(base + ["--self", "--k", k])
    small = d / "small.vec"
    write_vec(small, ["a", "b", "c"], [[1.0] * 20, [2.0] * 20, [0.5] * 20])
    msg = cli_error(["--vectors", str(small), "--self", "--k", "3"])
    assert "3" in msg and "--self" in msg
    msg = cli_error(["--vectors", str(small), "--query_vectors",
                     vec_files["query"], "--k", "4"])
    assert "4" in msg and "3" in msg
    # dimension mismatch names both numbers
    other = d / "wide.vec"
    write_vec(other, ["w"], [[1.0] * 24])
    msg = cli_error(base + ["--query_vectors", str(other)])
    assert "dimension mismatch" in msg and "24" in msg and "20" in msg
    # malformed files
    bad = d / "bad.vec"
    bad.write_text("2\t20\nm\t1.0 2.0\n")
    assert "line 2" in cli_error(["--vectors", str(bad), "--self"])
    nov = d / "nov.jsonl"
    nov.write_text(json.dumps({"id": 0, "expected": "x"}) + "\n")
    assert "--with_vector" in cli_error(base + ["--query_predictions",
                                                str(nov)])
    assert "similar: " in cli_error(
        ["--vectors", str(d / "missing.vec"), "--self"])


@pytest.mark.parametrize("tool,flag", [("similar.py", "--query_predictions"),
                                       ("bench_sim.py", "--shapes")])
def test_tools_help_exits_zero(tool, flag):
    res = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", tool), "--help"],
        capture_output=True, text=True, timeout=90, cwd=REPO)
    assert res.returncode == 0, res.stderr[-400:]
    assert flag in res.stdout


# ---------------------------------------------------------------------------
SHAPE = ["--terminal_embed_size", "12", "--path_embed_size", "12",
         "--encode_size", "16", "--max_path_length", "24"]


def test_train_predict_similar_end_to_end(tmp_path, tiny_corpus):
    """The checkpoint and code.vec come from the same export, so a vector
    predicted for a training method agrees with its code.vec row up to
    summation order; bf16 rounding moves a unit row's squared norm by at
    most 2 * 2^-9 ~ 0.004, hence the 0.99 bound on the best neighbour."""
    import main as cli

    out_dir = tmp_path / "out"
    # --max_path_length 24: no method of the tiny corpus is subsampled
    cli.main([
        "--corpus_path", tiny_corpus["corpus_path"],
        "--path_idx_path", tiny_corpus["path_idx_path"],
        "--terminal_idx_path", tiny_corpus["terminal_idx_path"],
        "--model_path", str(out_dir),
        "--vectors_path", str(out_dir / "code.vec"),
        "--test_result_path", str(out_dir / "test_results.tsv"),
        "--max_epoch", "2", "--batch_size", "16", *SHAPE,
        "--no_cuda", "--print_sample_cycle", "0",
    ])
    preds = tmp_path / "preds.jsonl"
    assert predict_cli.main([
        "--model", str(out_dir / "code2vec.model"),
        "--corpus_path", tiny_corpus["corpus_path"],
        "--path_idx_path", tiny_corpus["path_idx_path"],
        "--terminal_idx_path", tiny_corpus["terminal_idx_path"],
        "--query_corpus", tiny_corpus["corpus_path"], "--out", str(preds),
        "--no_cuda", "--batch_size", "16", "--with_vector", *SHAPE]) == 0
    out = tmp_path / "similar.jsonl"
    assert run_cli(["--vectors", str(out_dir / "code.vec"),
                    "--query_predictions", str(preds), "--k", "3",
                    "--out", str(out)]) == 0
    rows = read_jsonl(out)
    assert len(rows) == 48
    index_names, _ = read_code_vec(str(out_dir / "code.vec"))
    assert len(index_names) == 48
    expected = [json.loads(ln)["expected"] for ln in open(preds)]
    for r, exp in zip(rows, expected):
        assert r["name"] == exp
        assert len(r["neighbors"]) == 3
        best = r["neighbors"][0]
        print(f"query {r['query']}: best {best['score']:.5f}")
        assert best["score"] >= 0.99
