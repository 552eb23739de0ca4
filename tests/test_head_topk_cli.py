"""tools/predict.py --fused_head end to end on the CPU (default-head and
angular-margin checkpoints written by main.py), and tools/bench_head_topk.py
as a command."""

import json
import os
import subprocess
import sys

import pytest

import main as cli
from code2vec_amd.data.reader import CorpusReader
from tools import predict as predict_cli

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--terminal_embed_size", "12", "--path_embed_size", "12",
         "--encode_size", "16", "--max_path_length", "24"]


def train_checkpoint(tmp_path, tiny_corpus, *extra):
    out_dir = tmp_path / "out"
    cli.main([
        "--corpus_path", tiny_corpus["corpus_path"],
        "--path_idx_path", tiny_corpus["path_idx_path"],
        "--terminal_idx_path", tiny_corpus["terminal_idx_path"],
        "--model_path", str(out_dir),
        "--vectors_path", str(out_dir / "code.vec"),
        "--test_result_path", str(out_dir / "test_results.tsv"),
        "--max_epoch", "2", "--batch_size", "16", *SHAPE,
        "--no_cuda", "--print_sample_cycle", "0", *extra,
    ])
    return str(out_dir / "code2vec.model")


def predict_argv(ckpt, tiny_corpus, out):
    return ["--model", ckpt,
            "--corpus_path", tiny_corpus["corpus_path"],
            "--path_idx_path", tiny_corpus["path_idx_path"],
            "--terminal_idx_path", tiny_corpus["terminal_idx_path"],
            "--query_corpus", tiny_corpus["corpus_path"], "--out", str(out),
            "--no_cuda", "--batch_size", "16", *SHAPE]


def read_rows(path):
    return [json.loads(ln) for ln in path.read_text().splitlines()]


def test_cli_fused_head_default_checkpoint(tmp_path, tiny_corpus):
    ckpt = train_checkpoint(tmp_path, tiny_corpus)
    base, fused, packed = (tmp_path / n for n in
                           ("base.jsonl", "fused.jsonl", "packed.jsonl"))
    argv = predict_argv(ckpt, tiny_corpus, base)
    assert predict_cli.main(argv) == 0
    argv = predict_argv(ckpt, tiny_corpus, fused) + ["--fused_head"]
    assert predict_cli.main(argv) == 0
    argv = predict_argv(ckpt, tiny_corpus, packed) + ["--fused_head",
                                                      "--all_contexts"]
    assert predict_cli.main(argv) == 0
    rb, rf, rp = read_rows(base), read_rows(fused), read_rows(packed)
    assert len(rb) == len(rf) == len(rp) == 48
    for a, b, c in zip(rb, rf, rp):
        assert set(b) == {"id", "expected", "predictions", "contexts"}
        assert a["id"] == b["id"] == c["id"]
        assert a["contexts"] == b["contexts"]
        for x in (b, c):
            assert [p["name"] for p in x["predictions"]] \
                == [p["name"] for p in a["predictions"]]
            for pa, px in zip(a["predictions"], x["predictions"]):
                assert abs(pa["prob"] - px["prob"]) <= 1e-4 * pa["prob"] + 1e-7


def test_cli_fused_head_angular_checkpoint(tmp_path, tiny_corpus):
    ckpt = train_checkpoint(tmp_path, tiny_corpus, "--angular_margin_loss")
    reader = CorpusReader(tiny_corpus["corpus_path"],
                          tiny_corpus["path_idx_path"],
                          tiny_corpus["terminal_idx_path"])
    known = set(reader.label_vocab.stoi)
    # without the flags: the one-line message that names them
    for extra in ([], ["--fused_head"], ["--angular_margin_loss"]):
        with pytest.raises(SystemExit) as e:
            predict_cli.main(predict_argv(ckpt, tiny_corpus,
                                          tmp_path / "x.jsonl") + extra)
        msg = str(e.value)
        assert "\n" not in msg and "angular" in msg
        assert "--angular_margin_loss --fused_head" in msg
    out = tmp_path / "ang.jsonl"
    assert predict_cli.main(
        predict_argv(ckpt, tiny_corpus, out)
        + ["--angular_margin_loss", "--fused_head", "--inverse_temp", "30"]
    ) == 0
    rows = read_rows(out)
    assert len(rows) == 48
    for r in rows:
        assert len(r["predictions"]) == 5
        probs = [p["prob"] for p in r["predictions"]]
        assert all(p["name"] in known for p in r["predictions"])
        assert all(0.0 < p <= 1.0 for p in probs)
        assert probs == sorted(probs, reverse=True)
        assert sum(probs) <= 1.0 + 1e-5
        assert 1 <= len(r["contexts"]) <= 5
    # a colder head is sharper: the scale reaches the model
    out2 = tmp_path / "ang2.jsonl"
    assert predict_cli.main(
        predict_argv(ckpt, tiny_corpus, out2)
        + ["--angular_margin_loss", "--fused_head", "--inverse_temp", "60"]
    ) == 0
    rows2 = read_rows(out2)
    assert [[p["name"] for p in r["predictions"]] for r in rows2] \
        == [[p["name"] for p in r["predictions"]] for r in rows]
    assert sum(r["predictions"][0]["prob"] for r in rows2) \
        > sum(r["predictions"][0]["prob"] for r in rows)
    # a label count that disagrees names the angular tensor
    with pytest.raises(SystemExit) as e:
        argv = predict_argv(ckpt, tiny_corpus, tmp_path / "x.jsonl") \
            + ["--angular_margin_loss", "--fused_head"]
        other = tmp_path / "other.txt"
        text = open(tiny_corpus["corpus_path"], encoding="utf-8").read()
        other.write_text(text.replace("label:", "label:zz", 1))
        argv[argv.index("--corpus_path") + 1] = str(other)
        predict_cli.main(argv)
    assert "label count" in str(e.value)
    assert "output_linear.shape[0]" in str(e.value)


def test_default_checkpoint_with_angular_flag_is_rejected(tmp_path,
                                                          tiny_corpus):
    ckpt = train_checkpoint(tmp_path, tiny_corpus)
    with pytest.raises(SystemExit) as e:
        predict_cli.main(predict_argv(ckpt, tiny_corpus, tmp_path / "x.jsonl")
                         + ["--angular_margin_loss", "--fused_head"])
    assert "default head" in str(e.value)


def test_bench_head_topk_cli():
    tool = os.path.join(REPO, "tools", "bench_head_topk.py")
    res = subprocess.run([sys.executable, tool, "--help"],
                         capture_output=True, text=True, timeout=90, cwd=REPO)
    assert res.returncode == 0, res.stderr[-400:]
    assert "--nsplit" in res.stdout and "--tiny" in res.stdout
    res = subprocess.run([sys.executable, tool, "--device", "cpu", "--tiny"],
                         capture_output=True, text=True, timeout=90, cwd=REPO)
    assert res.returncode == 0, res.stderr[-400:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("|")]
    assert len(lines) == 3 and "fused med (min) us" in lines[0]
    assert lines[2].startswith("| 3 | 200 | 64 |")
