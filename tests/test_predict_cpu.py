"""Top-k prediction on CPU: the row_topk oracle, the Predictor on a
checkpoint trained through the CLI, and tools/predict.py end to end."""

import json
import os
import re
import subprocess
import sys

import pytest
import torch

import main as cli
from code2vec_amd.data.builder import DatasetBuilder
from code2vec_amd.data.reader import CorpusReader
from code2vec_amd.engine.predict import Predictor
from code2vec_amd.models.code2vec import (
    build_model, logical_from_reference_state_dict)
from code2vec_amd.ops import functional as Fn
from code2vec_amd.ops import reference as R
from code2vec_amd.utils.options import Option
from tools import predict as predict_cli

SHAPE = ["--terminal_embed_size", "12", "--path_embed_size", "12",
         "--encode_size", "16", "--max_path_length", "24"]


def train_checkpoint(tmp_path, tiny_corpus):
    """run_cli's flags (tests/test_train_cpu.py) with --max_path_length 24:
    the tiny corpus has at most 24 contexts per method, so none is
    subsampled."""
    out_dir = tmp_path / "out"
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
    return str(out_dir / "code2vec.model")


def predict_argv(ckpt, tiny_corpus, query, out):
    return ["--model", ckpt,
            "--corpus_path", tiny_corpus["corpus_path"],
            "--path_idx_path", tiny_corpus["path_idx_path"],
            "--terminal_idx_path", tiny_corpus["terminal_idx_path"],
            "--query_corpus", query, "--out", str(out),
            "--no_cuda", "--batch_size", "16", *SHAPE]


def unseen_name(i):
    return "zzunseen" + chr(97 + i % 26) + chr(97 + i // 26)


def write_relabelled(tiny_corpus, path):
    """The tiny corpus with every label replaced by a name no training
    run has seen (letters only, lowercase: normalization keeps them)."""
    n = [0]

    def sub(_):
        n[0] += 1
        return "label:" + unseen_name(n[0] - 1)

    with open(tiny_corpus["corpus_path"], encoding="utf-8") as f:
        text = re.sub(r"^label:.*$", sub, f.read(), flags=re.M)
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    return n[0]


# ---------------------------------------------------------------------------
def test_reference_row_topk_tie_rule_and_lse():
    x = torch.tensor([[1.0, 3.0, 3.0, -1.0, 3.0, 0.0],
                      [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    vals, idx, lse = R.row_topk(x, 4)
    assert idx.tolist() == [[1, 2, 4, 0], [0, 1, 2, 3]]
    assert vals.tolist() == [[3.0, 3.0, 3.0, 1.0], [0.0] * 4]
    assert vals.dtype == torch.float32 and idx.dtype == torch.int64
    assert torch.allclose(lse, torch.logsumexp(x, dim=1))
    # bf16 input: values come back as exact fp32 images
    vb, ib, lb = R.row_topk(x.to(torch.bfloat16), 2)
    assert ib.tolist() == [[1, 2], [0, 1]] and vb.dtype == torch.float32
    for bad in (0, 17, 7):
        with pytest.raises(ValueError):
            R.row_topk(x, bad)


def test_functional_row_topk_on_cpu_is_the_reference():
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(7, 300, generator=g).to(dtype)
        got = Fn.row_topk(x, 10)
        want = R.row_topk(x, 10)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        probs = Fn.topk_probs(got[0], got[2])
        assert torch.allclose(
            probs, torch.softmax(x.float(), 1).gather(1, got[1]), rtol=1e-5)
    for bad in (0, 17, 301):
        with pytest.raises(ValueError):
            Fn.row_topk(x, bad)


def test_predictor_rejects_bad_options():
    from code2vec_amd.models.code2vec import Code2VecTorch

    opt = Option(terminal_count=20, path_count=20, label_count=8,
                 max_path_length=4, terminal_embed_size=8,
                 path_embed_size=8, encode_size=8, dropout_prob=0.0,
                 angular_margin_loss=True, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="angular"):
        Predictor(Code2VecTorch(opt), None, torch.device("cpu"))
    opt.angular_margin_loss = False
    model = Code2VecTorch(opt)
    for kw in ({"topk": 17}, {"topk": 0}, {"top_contexts": 17},
               {"topk": 9}):  # 9 > the model's 8 labels
        with pytest.raises(ValueError):
            Predictor(model, None, torch.device("cpu"), **kw)


def test_predictor_matches_model_outputs(tmp_path, tiny_corpus):
    ckpt = train_checkpoint(tmp_path, tiny_corpus)
    reader = CorpusReader(tiny_corpus["corpus_path"],
                          tiny_corpus["path_idx_path"],
                          tiny_corpus["terminal_idx_path"])
    sd = torch.load(ckpt, weights_only=True)
    opt = Option(terminal_count=len(reader.terminal_vocab),
                 path_count=len(reader.path_vocab),
                 label_count=len(reader.label_vocab),
                 max_path_length=24, terminal_embed_size=12,
                 path_embed_size=12, encode_size=16, dropout_prob=0.0,
                 batch_size=16, device=torch.device("cpu"))
    model = build_model(opt, backend="torch",
                        logical=logical_from_reference_state_dict(sd, opt))
    k = 5
    predictor = Predictor(model, reader, torch.device("cpu"), topk=k,
                          top_contexts=3, batch_size=16)
    preds = list(predictor.predict_items(reader.items))
    assert [p.id for p in preds] == [it.id for it in reader.items]

    # the same rows the predictor built (same seed, no subsampling at
    # C = 24), through the same model
    data = DatasetBuilder(reader, opt, split_ratio=0.0,
                          seed=predictor.seed).build_data(reader.items, 24)
    with torch.no_grad():
        outputs, cv, attn = model(
            torch.from_numpy(data.starts), torch.from_numpy(data.paths),
            torch.from_numpy(data.ends),
            torch.zeros(len(data), dtype=torch.int64))
    top_val, top_idx = torch.max(outputs, dim=1)
    itos = reader.label_vocab.itos
    for i, pred in enumerate(preds):
        assert pred.names[0][0] == itos[int(top_idx[i])]
        probs = [p for _, p in pred.names]
        assert len(probs) == k
        assert all(0.0 < p <= 1.0 for p in probs)
        assert probs == sorted(probs, reverse=True)
        assert sum(probs) <= 1.0 + 1e-5
        assert torch.equal(pred.code_vector, cv[i])
        n_real = int((data.starts[i] != 0).sum())
        assert len(pred.contexts) == min(3, n_real)
        att = [a for _, _, _, a in pred.contexts]
        assert att == sorted(att, reverse=True)
        assert all(s != "<PAD/>" for s, _, _, _ in pred.contexts)


def test_cli_writes_one_json_line_per_method(tmp_path, tiny_corpus):
    ckpt = train_checkpoint(tmp_path, tiny_corpus)
    reader = CorpusReader(tiny_corpus["corpus_path"],
                          tiny_corpus["path_idx_path"],
                          tiny_corpus["terminal_idx_path"])
    known = set(reader.label_vocab.stoi)

    out = tmp_path / "pred.jsonl"
    assert predict_cli.main(
        predict_argv(ckpt, tiny_corpus, tiny_corpus["corpus_path"], out)
        + ["--with_vector"]) == 0
    rows = [json.loads(ln) for ln in out.read_text().splitlines()]
    assert len(rows) == 48
    assert [r["id"] for r in rows] == [it.id for it in reader.items]
    for r, it in zip(rows, reader.items):
        assert set(r) == {"id", "expected", "predictions", "contexts",
                          "vector"}
        assert r["expected"] == it.normalized_label
        assert len(r["predictions"]) == 5
        for p in r["predictions"]:
            assert set(p) == {"name", "prob"} and p["name"] in known
            assert 0.0 < p["prob"] <= 1.0
        assert 1 <= len(r["contexts"]) <= 5
        for c in r["contexts"]:
            assert set(c) == {"start", "path", "end", "attention"}
        assert len(r["vector"]) == 16

    # labels the model never saw: still predicts, echoes them as expected
    query = tmp_path / "unseen.txt"
    assert write_relabelled(tiny_corpus, query) == 48
    out2 = tmp_path / "pred2.jsonl"
    assert predict_cli.main(
        predict_argv(ckpt, tiny_corpus, str(query), out2)) == 0
    rows2 = [json.loads(ln) for ln in out2.read_text().splitlines()]
    assert len(rows2) == 48
    for i, (r2, r) in enumerate(zip(rows2, rows)):
        assert set(r2) == {"id", "expected", "predictions", "contexts"}
        assert r2["expected"] == unseen_name(i) and r2["expected"] not in known
        assert r2["predictions"] == r["predictions"]
        assert r2["contexts"] == r["contexts"]


def test_cli_error_paths(tmp_path, tiny_corpus, capsys):
    ckpt = train_checkpoint(tmp_path, tiny_corpus)
    reader = CorpusReader(tiny_corpus["corpus_path"],
                          tiny_corpus["path_idx_path"],
                          tiny_corpus["terminal_idx_path"])
    n_labels = len(reader.label_vocab)
    # a "training" corpus whose label count differs from the checkpoint's
    other = tmp_path / "other.txt"
    assert write_relabelled(tiny_corpus, other) == 48 != n_labels
    argv = predict_argv(ckpt, tiny_corpus, tiny_corpus["corpus_path"],
                        tmp_path / "x.jsonl")
    argv[argv.index("--corpus_path") + 1] = str(other)
    with pytest.raises(SystemExit) as e:
        predict_cli.main(argv)
    msg = str(e.value)
    assert "\n" not in msg and "label count" in msg
    assert "48" in msg and str(n_labels) in msg
    assert "output_linear.weight" in msg

    # a wrong model-shape flag names both numbers too
    argv = predict_argv(ckpt, tiny_corpus, tiny_corpus["corpus_path"],
                        tmp_path / "x.jsonl")
    argv[argv.index("--encode_size") + 1] = "32"
    with pytest.raises(SystemExit) as e:
        predict_cli.main(argv)
    assert "encode_size" in str(e.value) and "32" in str(e.value) \
        and "16" in str(e.value)

    with pytest.raises(SystemExit) as e:
        predict_cli.main(predict_argv(
            ckpt, tiny_corpus, tiny_corpus["corpus_path"],
            tmp_path / "x.jsonl") + ["--topk", "17"])
    assert e.value.code == 2
    assert "--topk" in capsys.readouterr().err

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run(
        [sys.executable, os.path.join(repo, "tools", "predict.py"),
         "--help"], capture_output=True, text=True, timeout=90, cwd=repo)
    assert res.returncode == 0, res.stderr[-400:]
    assert "--query_corpus" in res.stdout
