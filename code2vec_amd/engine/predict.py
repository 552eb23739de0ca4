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

With ``all_contexts=True`` methods are predicted from ALL their
path-contexts: batches are packed (``DatasetBuilder.build_packed``,
``PackedBatchIterator``) and go through ``model.forward_packed`` (K21),
eagerly, because their shapes vary.  Nothing is padded, subsampled or
drawn from an RNG, and a method's code vector and attention do not depend
on which other methods share its batch.

With ``fused_head=True`` names come from ``model.encode`` +
``model.head_topk`` (K23): the [B, L] logits are never allocated, on the
padded, the graphed and the packed path alike, and the angular-margin head
is accepted, scored by its margin-free logits inverse_temp * cosine.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, List, Optional, Tuple

import torch

from ..data.builder import DatasetBuilder
from ..models.code2vec import ANGULAR_PREDICT_ERROR
from ..ops import functional as Fn
from ..ops import reference as R
from .infer import graphed_export_forward
from .loader import BatchIterator, PackedBatchIterator


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
    """``seed`` seeds the subsampling of bags larger than max_path_length
    on the padded path; with ``all_contexts=True`` nothing is subsampled
    and it is unused.  ``max_batch_contexts`` is the packed path's row
    budget per batch (default ``batch_size * max_path_length``, the padded
    path's activation footprint)."""

    def __init__(self, model, vocab_reader, device, topk: int = 5,
                 top_contexts: int = 5, batch_size: int = 32,
                 use_graph: bool = True, seed: int = 123,
                 all_contexts: bool = False,
                 max_batch_contexts: Optional[int] = None,
                 fused_head: bool = False) -> None:
        option = model.option
        if option.angular_margin_loss and not fused_head:
            raise ValueError(ANGULAR_PREDICT_ERROR)
        for name, v in (("topk", topk), ("top_contexts", top_contexts)):
            if not 1 <= v <= R.ROW_TOPK_MAX_K:
                raise ValueError(
                    f"{name} must be in 1..{R.ROW_TOPK_MAX_K}, got {v}")
        if topk > option.label_count:
            raise ValueError(
                f"topk = {topk} exceeds the model's {option.label_count} "
                "labels")
        if max_batch_contexts is None:
            max_batch_contexts = batch_size * option.max_path_length
        if max_batch_contexts < 1:
            raise ValueError(
                f"max_batch_contexts must be >= 1, got {max_batch_contexts}")
        self.model = model
        self.reader = vocab_reader
        self.device = torch.device(device)
        self.topk = topk
        self.top_contexts = top_contexts
        self.batch_size = batch_size
        # seeds the subsampling of bags larger than max_path_length
        self.seed = seed
        self.all_contexts = all_contexts
        self.max_batch_contexts = max_batch_contexts
        self.fused_head = fused_head
        model.eval()
        self.graphed = (
            graphed_export_forward(model, batch_size, self.device,
                                   topk=topk if fused_head else None)
            if use_graph and not all_contexts else None
        )
        self._builders = {}

    # ------------------------------------------------------------------
    @torch.no_grad()
    def _forward(self, starts, paths, ends):
        """(outputs, code_vector, attention); with ``fused_head`` outputs
        is head_topk's (vals, idx, lse) instead of the logits."""
        label = torch.zeros(starts.shape[0], dtype=torch.int64,
                            device=self.device)
        if (self.graphed is not None and starts.shape[0] <= self.graphed.B
                and starts.shape[1] == self.graphed.C):
            return self.graphed.run(starts, paths, ends, label)
        if self.fused_head:
            cv, cvb, attn = self.model.encode(starts, paths, ends)
            return self.model.head_topk(cvb, self.topk), cv, attn
        return self.model(starts, paths, ends, label)

    def _names(self, outputs):
        """(label index, probability) tensors [B, topk] on the CPU."""
        if self.fused_head:
            vals, idx, lse = outputs
        else:
            vals, idx, lse = Fn.row_topk(outputs.detach().contiguous(),
                                         self.topk)
        return idx.cpu(), Fn.topk_probs(vals, lse).cpu()

    @torch.no_grad()
    def predict_batch(self, batch) -> List[Prediction]:
        """``batch``: a BatchIterator dict; its ``label`` is ignored."""
        starts = batch["starts"].to(self.device)
        paths = batch["paths"].to(self.device)
        ends = batch["ends"].to(self.device)
        outputs, code_vector, attn = self._forward(starts, paths, ends)

        idx_c, probs_c = self._names(outputs)
        # PAD positions sort below every real context (attention >= 0), so
        # a PAD never displaces one; they are dropped on the host below
        masked = attn.detach().float().masked_fill(starts == 0, -1.0)
        kc = min(self.top_contexts, masked.shape[1])
        cvals, cidx, _ = Fn.row_topk(masked.contiguous(), kc)

        cvals_c, cidx_c = cvals.cpu(), cidx.cpu()
        cv_c = code_vector.detach().float().cpu()
        starts_c, paths_c, ends_c = starts.cpu(), paths.cpu(), ends.cpu()
        ids = batch["id"]

        preds = []
        for i in range(starts_c.shape[0]):
            contexts = []
            for j in range(kc):
                c = int(cidx_c[i, j])
                if int(starts_c[i, c]) == 0:
                    break  # only PADs follow
                contexts.append(self._context(
                    starts_c[i, c], paths_c[i, c], ends_c[i, c],
                    cvals_c[i, j]))
            preds.append(Prediction(int(ids[i]), self._name_list(
                idx_c[i], probs_c[i]), contexts, cv_c[i]))
        return preds

    @torch.no_grad()
    def predict_packed_batch(self, batch) -> List[Prediction]:
        """``batch``: a PackedBatchIterator dict (flat ``starts``/``paths``/
        ``ends``, CPU ``lengths``); its ``label`` is ignored."""
        starts = batch["starts"].to(self.device)
        paths = batch["paths"].to(self.device)
        ends = batch["ends"].to(self.device)
        lens = batch["lengths"]
        if self.fused_head:
            code_vector, cvb, attn = self.model.encode_packed(
                starts, paths, ends, lens)
            outputs = self.model.head_topk(cvb, self.topk)
        else:
            outputs, code_vector, attn = self.model.forward_packed(
                starts, paths, ends, lens)

        idx_c, probs_c = self._names(outputs)
        # per-method top contexts in K19's order: the ragged attention
        # goes into a [B, longest] matrix filled with -1, below every real
        # context's weight (>= 0); PAD rows are set to -1 as well
        B, width = lens.numel(), int(lens.max())
        offs = torch.zeros(B, dtype=torch.int64)
        offs[1:] = torch.cumsum(lens, 0)[:-1]
        col = torch.arange(int(lens.sum())) - torch.repeat_interleave(
            offs, lens)
        flat = (torch.repeat_interleave(torch.arange(B), lens) * width
                + col).to(self.device)
        matrix = torch.full((B * width,), -1.0, dtype=torch.float32,
                            device=self.device)
        matrix[flat] = attn.detach().float().masked_fill(starts == 0, -1.0)
        kc = min(self.top_contexts, width)
        cvals, cidx, _ = Fn.row_topk(matrix.view(B, width), kc)

        cvals_c, cidx_c = cvals.cpu(), cidx.cpu()
        cv_c = code_vector.detach().float().cpu()
        starts_c, paths_c, ends_c = starts.cpu(), paths.cpu(), ends.cpu()
        ids = batch["id"]

        preds = []
        for i in range(B):
            lo = int(offs[i])
            contexts = []
            for j in range(kc):
                if float(cvals_c[i, j]) < 0.0:
                    break  # only PADs and filler follow
                r = lo + int(cidx_c[i, j])
                contexts.append(self._context(
                    starts_c[r], paths_c[r], ends_c[r], cvals_c[i, j]))
            preds.append(Prediction(int(ids[i]), self._name_list(
                idx_c[i], probs_c[i]), contexts, cv_c[i]))
        return preds

    def _name_list(self, idx_row, probs_row):
        label_itos = self.reader.label_vocab.itos
        return [(label_itos[int(idx_row[j])], float(probs_row[j]))
                for j in range(self.topk)]

    def _context(self, s, p, e, weight):
        return (self.reader.terminal_vocab.itos.get(int(s), ""),
                self.reader.path_vocab.itos.get(int(p), ""),
                self.reader.terminal_vocab.itos.get(int(e), ""),
                float(weight))

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
        if self.all_contexts:
            packed = builder.build_packed(list(items))
            for batch in PackedBatchIterator(packed, self.max_batch_contexts,
                                             device=self.device):
                yield from self.predict_packed_batch(batch)
            return
        data = builder.build_data(
            list(items), self.model.option.max_path_length)
        loader = BatchIterator(data, self.batch_size, shuffle=False,
                               device=self.device)
        for batch in loader:
            yield from self.predict_batch(batch)
