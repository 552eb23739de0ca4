"""Top-k name prediction with a trained model.

``Predictor`` is the inference path for methods that were not part of a
training run: it forwards index batches through the model (hipGraph
replay on the HIP backend, as the export loop does), selects the k most
likely names with softmax probabilities and the n most-attended
path-contexts with the K19 ``row_topk`` kernel, and resolves indexes to
names through the training reader's vocab tables exactly as
``export.print_sample`` does.

The label tensor handed to ``forward`` is zeros: the default output head
never reads it.  The angular-margin head does (its forward bakes the true
label's margin into the logits), so it is rejected at construction.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, List, Tuple

import torch

from ..data.builder import DatasetBuilder
from ..ops import functional as Fn
from ..ops import reference as R
from .infer import graphed_export_forward
from .loader import BatchIterator


@dataclass
class Prediction:
    id: int
    # k entries, descending probability
    names: List[Tuple[str, float]]
    # up to n (start, path, end, attention) entries, descending attention;
    # PAD contexts are never reported
    contexts: List[Tuple[str, str, str, float]]
    code_vector: torch.Tensor  # [E] fp32, CPU


class Predictor:
    def __init__(self, model, vocab_reader, device, topk: int = 5,
                 top_contexts: int = 5, batch_size: int = 32,
                 use_graph: bool = True, seed: int = 123) -> None:
        option = model.option
        if option.angular_margin_loss:
            raise ValueError(
                "Predictor does not support the angular-margin head: its "
                "forward needs the true label, which prediction does not "
                "have")
        for name, v in (("topk", topk), ("top_contexts", top_contexts)):
            if not 1 <= v <= R.ROW_TOPK_MAX_K:
                raise ValueError(
                    f"{name} must be in 1..{R.ROW_TOPK_MAX_K}, got {v}")
        if topk > option.label_count:
            raise ValueError(
                f"topk = {topk} exceeds the model's {option.label_count} "
                "labels")
        self.model = model
        self.reader = vocab_reader
        self.device = torch.device(device)
        self.topk = topk
        self.top_contexts = top_contexts
        self.batch_size = batch_size
        # seeds the subsampling of bags larger than max_path_length
        self.seed = seed
        model.eval()
        self.graphed = (
            graphed_export_forward(model, batch_size, self.device)
            if use_graph else None
        )
        self._builders = {}

    # ------------------------------------------------------------------
    @torch.no_grad()
    def _forward(self, starts, paths, ends):
        label = torch.zeros(starts.shape[0], dtype=torch.int64,
                            device=self.device)
        if (self.graphed is not None and starts.shape[0] <= self.graphed.B
                and starts.shape[1] == self.graphed.C):
            return self.graphed.run(starts, paths, ends, label)
        return self.model(starts, paths, ends, label)

    @torch.no_grad()
    def predict_batch(self, batch) -> List[Prediction]:
        """``batch``: a BatchIterator dict; its ``label`` is ignored."""
        starts = batch["starts"].to(self.device)
        paths = batch["paths"].to(self.device)
        ends = batch["ends"].to(self.device)
        outputs, code_vector, attn = self._forward(starts, paths, ends)

        vals, idx, lse = Fn.row_topk(outputs.detach().contiguous(), self.topk)
        probs = Fn.topk_probs(vals, lse)
        # PAD positions sort below every real context (attention >= 0), so
        # a PAD never displaces one; they are dropped on the host below
        masked = attn.detach().float().masked_fill(starts == 0, -1.0)
        kc = min(self.top_contexts, masked.shape[1])
        cvals, cidx, _ = Fn.row_topk(masked.contiguous(), kc)

        idx_c, probs_c = idx.cpu(), probs.cpu()
        cvals_c, cidx_c = cvals.cpu(), cidx.cpu()
        cv_c = code_vector.detach().float().cpu()
        starts_c, paths_c, ends_c = starts.cpu(), paths.cpu(), ends.cpu()
        ids = batch["id"]

        label_itos = self.reader.label_vocab.itos
        term_itos = self.reader.terminal_vocab.itos
        path_itos = self.reader.path_vocab.itos
        preds = []
        for i in range(starts_c.shape[0]):
            names = [
                (label_itos[int(idx_c[i, j])], float(probs_c[i, j]))
                for j in range(self.topk)
            ]
            contexts = []
            for j in range(kc):
                c = int(cidx_c[i, j])
                if int(starts_c[i, c]) == 0:
                    break  # only PADs follow
                contexts.append((
                    term_itos.get(int(starts_c[i, c]), ""),
                    path_itos.get(int(paths_c[i, c]), ""),
                    term_itos.get(int(ends_c[i, c]), ""),
                    float(cvals_c[i, j]),
                ))
            preds.append(Prediction(int(ids[i]), names, contexts, cv_c[i]))
        return preds

    def predict_items(self, items, reader=None) -> Iterator[Prediction]:
        """Predict for ``CodeItem``s in order.  ``reader`` is the reader
        that parsed them (default: the vocab reader); it must share the
        vocab reader's terminal/path index files.  Its labels may be
        unknown to the model — they are never looked up here."""
        reader = reader or self.reader
        builder = self._builders.get(id(reader))
        if builder is None:
            builder = DatasetBuilder(reader, self.model.option,
                                     split_ratio=0.0, seed=self.seed)
            self._builders[id(reader)] = builder
        data = builder.build_data(
            list(items), self.model.option.max_path_length)
        loader = BatchIterator(data, self.batch_size, shuffle=False,
                               device=self.device)
        for batch in loader:
            yield from self.predict_batch(batch)
