#!/usr/bin/env python3
"""Predict method names with a trained code2vec.model.

Loads a checkpoint written by main.py, rebuilds the vocabularies from the
TRAINING corpus triplet (labels in first-occurrence order, exactly as a
warm start does), and writes one JSON object per method of the query
corpus, in corpus order:

    {"id", "expected", "predictions": [{"name", "prob"}],
     "contexts": [{"start", "path", "end", "attention"}]}

The query corpus uses the same format and the same path/terminal index
files.  Its labels may be names the model never saw; they only appear as
the "expected" string (normalized like the training labels, so it can be
compared with a predicted name).

By default a method goes through the training layout: padded to
--max_path_length contexts, a longer one subsampled (seeded by
--random_seed).  --all_contexts predicts from every context of every
method instead (packed batches, no padding, no subsampling, no seed).

--fused_head takes the names straight from the code vectors (K23): the
[methods, labels] logits matrix is never allocated, and a model trained
with --angular_margin_loss can predict (give both flags, and the run's
--inverse_temp); it is scored by its margin-free logits.

    python tools/predict.py --model output/code2vec.model \\
        --corpus_path dataset/corpus.txt \\
        --path_idx_path dataset/path_idxs.txt \\
        --terminal_idx_path dataset/terminal_idxs.txt \\
        --query_corpus new_methods.txt --topk 5
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MAX_K = 16


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(
        description=__doc__,
        formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--model", type=str, required=True,
                   help="code2vec.model checkpoint (reference state_dict)")
    p.add_argument("--corpus_path", type=str, default="./dataset/corpus.txt",
                   help="TRAINING corpus (defines the label vocabulary)")
    p.add_argument("--path_idx_path", type=str,
                   default="./dataset/path_idxs.txt")
    p.add_argument("--terminal_idx_path", type=str,
                   default="./dataset/terminal_idxs.txt")
    p.add_argument("--query_corpus", type=str, required=True,
                   help="methods to predict, same format and index files")
    p.add_argument("--topk", type=int, default=5,
                   help=f"names per method (1..{MAX_K})")
    p.add_argument("--top_contexts", type=int, default=5,
                   help=f"most-attended contexts per method (1..{MAX_K})")
    p.add_argument("--out", type=str, default=None,
                   help="output file (default: stdout)")
    p.add_argument("--with_vector", action="store_true", default=False,
                   help='add the code vector as "vector"')
    p.add_argument("--no_cuda", action="store_true", default=False)
    p.add_argument("--gpu", type=str, default="cuda:0")
    p.add_argument("--backend", type=str, default="auto",
                   choices=["auto", "hip", "torch"])
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--random_seed", type=int, default=123,
                   help="seeds the context subsampling of methods with more "
                        "than --max_path_length contexts (unused with "
                        "--all_contexts)")
    p.add_argument("--all_contexts", action="store_true", default=False,
                   help="predict from ALL of a method's contexts (packed "
                        "variable-length batches): no padding, no "
                        "subsampling, one answer per method whatever the "
                        "seed and the batch")
    p.add_argument("--max_batch_contexts", type=int, default=None,
                   help="with --all_contexts: path-contexts per batch "
                        "(default: batch_size * max_path_length); a larger "
                        "method runs alone")
    # model shape: main.py's names and defaults
    p.add_argument("--terminal_embed_size", type=int, default=100)
    p.add_argument("--path_embed_size", type=int, default=100)
    p.add_argument("--encode_size", type=int, default=300)
    p.add_argument("--max_path_length", type=int, default=200)
    p.add_argument("--angular_margin_loss", action="store_true",
                   default=False)
    p.add_argument("--inverse_temp", type=float, default=30.0,
                   help="the angular-margin head's logit scale (main.py's)")
    p.add_argument("--fused_head", action="store_true", default=False,
                   help="names through the fused head + top-k kernel: no "
                        "[methods, labels] logits; required for an "
                        "--angular_margin_loss model")
    return p


def _mismatch(what: str, have: int, tensor: str, want: int) -> SystemExit:
    return SystemExit(
        f"predict: {what} mismatch: arguments/corpus give {have}, "
        f"checkpoint {tensor} has {want}")


def check_checkpoint(sd, reader, args) -> None:
    """One-line error naming both numbers for every size that disagrees
    with the checkpoint tensors."""
    angular = "output_linear" in sd and "output_linear.weight" not in sd
    if angular and not (args.angular_margin_loss and args.fused_head):
        raise SystemExit(
            "predict: the checkpoint has an angular-margin head, which "
            "the default path cannot score without labels; add "
            "--angular_margin_loss --fused_head")
    if args.angular_margin_loss and not angular:
        raise SystemExit(
            "predict: --angular_margin_loss given, but the checkpoint has "
            "a default head (output_linear.weight)")
    term = sd["terminal_embedding.weight"]
    path = sd["path_embedding.weight"]
    w_in = sd["input_linear.weight"]
    out_name = "output_linear" if angular else "output_linear.weight"
    w_out = sd[out_name]
    checks = [
        ("terminal_embed_size", args.terminal_embed_size,
         "terminal_embedding.weight.shape[1]", term.shape[1]),
        ("path_embed_size", args.path_embed_size,
         "path_embedding.weight.shape[1]", path.shape[1]),
        ("encode_size", args.encode_size,
         "input_linear.weight.shape[0]", w_in.shape[0]),
        ("terminal count", len(reader.terminal_vocab),
         "terminal_embedding.weight.shape[0]", term.shape[0]),
        ("path count", len(reader.path_vocab),
         "path_embedding.weight.shape[0]", path.shape[0]),
        ("label count", len(reader.label_vocab),
         f"{out_name}.shape[0]", w_out.shape[0]),
    ]
    for what, have, tensor, want in checks:
        if int(have) != int(want):
            raise _mismatch(what, int(have), tensor, int(want))


def main(argv=None) -> int:
    parser = build_parser()
    args = parser.parse_args(argv)
    for flag in ("topk", "top_contexts"):
        v = getattr(args, flag)
        if not 1 <= v <= MAX_K:
            parser.error(f"--{flag} must be in 1..{MAX_K}, got {v}")
    if args.max_batch_contexts is not None and args.max_batch_contexts < 1:
        parser.error("--max_batch_contexts must be >= 1")

    import torch

    from code2vec_amd.data.reader import CorpusReader
    from code2vec_amd.engine.predict import Predictor
    from code2vec_amd.models.code2vec import (
        build_model, logical_from_reference_state_dict)
    from code2vec_amd.utils.options import Option

    use_cuda = not args.no_cuda and torch.cuda.is_available()
    device = torch.device(args.gpu if use_cuda else "cpu")
    if use_cuda:
        torch.cuda.set_device(device)
    torch.manual_seed(args.random_seed)

    reader = CorpusReader(args.corpus_path, args.path_idx_path,
                          args.terminal_idx_path)
    sd = torch.load(args.model, map_location="cpu", weights_only=True)
    check_checkpoint(sd, reader, args)
    if args.topk > len(reader.label_vocab):
        parser.error(f"--topk {args.topk} exceeds the "
                     f"{len(reader.label_vocab)} labels of the model")

    option = Option(
        terminal_count=len(reader.terminal_vocab),
        path_count=len(reader.path_vocab),
        label_count=len(reader.label_vocab),
        max_path_length=args.max_path_length,
        terminal_embed_size=args.terminal_embed_size,
        path_embed_size=args.path_embed_size,
        encode_size=args.encode_size,
        dropout_prob=0.0,
        batch_size=args.batch_size,
        angular_margin_loss=args.angular_margin_loss,
        inverse_temp=args.inverse_temp,
        device=device,
    )
    backend = args.backend
    if backend == "auto":
        backend = "hip" if device.type == "cuda" else "torch"
    model = build_model(option, backend=backend,
                        logical=logical_from_reference_state_dict(sd, option),
                        device=device)
    try:
        predictor = Predictor(model, reader, device, topk=args.topk,
                              top_contexts=args.top_contexts,
                              batch_size=args.batch_size,
                              seed=args.random_seed,
                              all_contexts=args.all_contexts,
                              max_batch_contexts=args.max_batch_contexts,
                              fused_head=args.fused_head)
    except ValueError as e:
        raise SystemExit(f"predict: {e}") from e

    query = CorpusReader(args.query_corpus, args.path_idx_path,
                         args.terminal_idx_path)
    out = open(args.out, "w", encoding="utf-8") if args.out else sys.stdout
    try:
        preds = predictor.predict_items(query.items, reader=query)
        for item, pred in zip(query.items, preds):
            row = {
                "id": pred.id,
                "expected": item.normalized_label,
                "predictions": [
                    {"name": n, "prob": p} for n, p in pred.names],
                "contexts": [
                    {"start": s, "path": pa, "end": e, "attention": a}
                    for s, pa, e, a in pred.contexts],
            }
            if args.with_vector:
                row["vector"] = [float(v) for v in pred.code_vector]
            out.write(json.dumps(row) + "\n")
    finally:
        if args.out:
            out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
