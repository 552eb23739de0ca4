"""Batch iterator — array-sliced batching with async H2D double-buffering.

Replaces the reference's ``DataLoader(num_workers=4)`` (reference
main.py:162,180): our epoch data is already dense int32 arrays (builder.py),
so batching is tensor slicing — no worker processes, no per-sample collate.
On GPU, batches are staged through pinned memory and copied on a dedicated
HIP stream one batch ahead of compute.
"""

from __future__ import annotations

from typing import Iterator, Optional

import numpy as np
import torch

from ..data.builder import EpochData, PackedData


def stripped_lengths(starts: np.ndarray) -> np.ndarray:
    """Row count of every method of a padded [N, C] ``starts`` array once
    its trailing pads are stripped: the position of the last ``starts > 0``
    plus one, at least 1 (an all-pad row keeps one PAD context)."""
    real = starts > 0
    C = starts.shape[1]
    last = C - np.argmax(real[:, ::-1], axis=1)
    return np.where(real.any(axis=1), last, 1).astype(np.int64)


class BatchIterator:
    """Iterates dict batches {'id','starts','paths','ends','label'}.

    ``pack=True`` (training on packed batches) yields the same methods in
    the same order — same seed, same permutation, same sampled contexts —
    with each method's trailing pads stripped: ``starts``/``paths``/``ends``
    are flat int32 [M] tensors holding the methods' rows back to back,
    ``lengths`` (int64 [B]) stays on the CPU, and on the GPU ``offsets``
    (int32 [B+1], the exclusive prefix sum of ``lengths``) arrives with the
    batch.  A batch never has more than ``row_capacity`` = batch_size * C
    rows."""

    def __init__(
        self,
        data: EpochData,
        batch_size: int,
        shuffle: bool = True,
        seed: int = 0,
        device: Optional[torch.device] = None,
        prefetch: bool = True,
        pack: bool = False,
    ) -> None:
        self.data = data
        self.pack = bool(pack)
        self.row_capacity = batch_size * int(data.starts.shape[1])
        # once per epoch (an iterator serves one epoch's data), in numpy
        self.lengths = stripped_lengths(data.starts) if self.pack else None
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.seed = seed
        self.device = device or torch.device("cpu")
        self.prefetch = prefetch and self.device.type == "cuda"
        self._epoch = 0

        self.starts = torch.from_numpy(data.starts)
        self.paths = torch.from_numpy(data.paths)
        self.ends = torch.from_numpy(data.ends)
        self.labels = torch.from_numpy(data.labels)
        self.ids = torch.as_tensor(
            [i if i is not None else -1 for i in data.ids], dtype=torch.int64
        )
        if self.prefetch:
            self._copy_stream = torch.cuda.Stream(self.device)
            # Double-buffered PINNED staging: a fancy-indexed gather
            # (self.starts[idx]) materializes a *pageable* tensor, which
            # silently degrades the non_blocking H2D copy to a staged
            # synchronous one.  Instead each batch is gathered into one of
            # two persistent pinned buffers and copied from there; a
            # per-slot event keeps the host from overwriting a slot whose
            # copy is still in flight.
            C = self.starts.shape[1]
            # packed batches are staged flat, at capacity (batch_size * C
            # rows), plus their offsets
            rows = (batch_size * C,) if self.pack else (batch_size, C)
            self._stage = [
                {
                    "starts": torch.empty(*rows, dtype=torch.int32,
                                          pin_memory=True),
                    "paths": torch.empty(*rows, dtype=torch.int32,
                                         pin_memory=True),
                    "ends": torch.empty(*rows, dtype=torch.int32,
                                        pin_memory=True),
                    "label": torch.empty(batch_size, dtype=torch.int64,
                                         pin_memory=True),
                }
                for _ in range(2)
            ]
            if self.pack:
                for st in self._stage:
                    st["offsets"] = torch.empty(batch_size + 1,
                                                dtype=torch.int32,
                                                pin_memory=True)
            self._stage_ev = [torch.cuda.Event(), torch.cuda.Event()]
            self._stage_used = [False, False]

    def __len__(self) -> int:
        n = self.starts.shape[0]
        return (n + self.batch_size - 1) // self.batch_size

    def _order(self) -> np.ndarray:
        n = self.starts.shape[0]
        if not self.shuffle:
            return np.arange(n)
        rng = np.random.default_rng([self.seed, self._epoch, 0xBA7C])
        return rng.permutation(n)

    def __iter__(self) -> Iterator[dict]:
        order = torch.from_numpy(self._order().astype(np.int64))
        self._epoch += 1
        n = self.starts.shape[0]
        bs = self.batch_size

        def host_batch(lo: int, hi: int) -> dict:
            idx = order[lo:hi]
            if self.pack:
                lens = torch.from_numpy(self.lengths[idx.numpy()])
                C = self.starts.shape[1]
                real = torch.arange(C)[None, :] < lens[:, None]
                return {
                    "id": self.ids[idx],
                    "starts": self.starts[idx][real],
                    "paths": self.paths[idx][real],
                    "ends": self.ends[idx][real],
                    "lengths": lens,
                    "label": self.labels[idx],
                }
            return {
                "id": self.ids[idx],
                "starts": self.starts[idx],
                "paths": self.paths[idx],
                "ends": self.ends[idx],
                "label": self.labels[idx],
            }

        if not self.prefetch:
            for lo in range(0, n, bs):
                yield host_batch(lo, min(lo + bs, n))
            return

        # double-buffered async H2D on a copy stream, staged through the
        # persistent pinned buffers (a pinned source is what makes the
        # non_blocking copy actually asynchronous).  The gather runs in
        # NUMPY into the pinned buffers' views: torch's CPU index_select
        # is ~70x slower (7.9 vs 0.11 ms per field at the top11 shape)
        # and made the input pipeline the bottleneck.
        order_np = order.numpy()
        src_np = {
            "starts": self.starts.numpy(), "paths": self.paths.numpy(),
            "ends": self.ends.numpy(), "label": self.labels.numpy(),
        }
        stage_np = [
            {k: v.numpy() for k, v in s.items()} for s in self._stage
        ]

        if self.pack:
            C = self.starts.shape[1]
            rect = np.empty((bs, C), dtype=np.int32)  # one field's rectangle
            cols = np.arange(C)[None, :]

        def stage_and_copy_packed(slot: int, lo: int, hi: int):
            if self._stage_used[slot]:
                self._stage_ev[slot].synchronize()  # copy out of this slot done
            self._stage_used[slot] = True
            idx = order[lo:hi]
            idx_np = order_np[lo:hi]
            k = hi - lo
            st = self._stage[slot]
            sn = stage_np[slot]
            lens = self.lengths[idx_np]
            m = int(lens.sum())
            real = (cols < lens[:, None]).ravel()
            for key in ("starts", "paths", "ends"):
                np.take(src_np[key], idx_np, axis=0, out=rect[:k])
                np.compress(real, rect[:k].ravel(), out=sn[key][:m])
            np.take(src_np["label"], idx_np, axis=0, out=sn["label"][:k])
            sn["offsets"][0] = 0
            np.cumsum(lens, out=sn["offsets"][1:k + 1])
            ev = self._stage_ev[slot]
            with torch.cuda.stream(self._copy_stream):
                db = {
                    "id": self.ids[idx],
                    "starts": st["starts"][:m].to(self.device, non_blocking=True),
                    "paths": st["paths"][:m].to(self.device, non_blocking=True),
                    "ends": st["ends"][:m].to(self.device, non_blocking=True),
                    "offsets": st["offsets"][:k + 1].to(self.device,
                                                        non_blocking=True),
                    "lengths": torch.from_numpy(lens),
                    "label": st["label"][:k].to(self.device, non_blocking=True),
                }
                ev.record(self._copy_stream)
            return db, ev

        def stage_and_copy(slot: int, lo: int, hi: int):
            if self.pack:
                return stage_and_copy_packed(slot, lo, hi)
            if self._stage_used[slot]:
                self._stage_ev[slot].synchronize()  # copy out of this slot done
            self._stage_used[slot] = True
            idx = order[lo:hi]
            idx_np = order_np[lo:hi]
            k = hi - lo
            st = self._stage[slot]
            sn = stage_np[slot]
            for key in ("starts", "paths", "ends", "label"):
                np.take(src_np[key], idx_np, axis=0, out=sn[key][:k])
            ev = self._stage_ev[slot]
            with torch.cuda.stream(self._copy_stream):
                db = {
                    "id": self.ids[idx],
                    "starts": st["starts"][:k].to(self.device, non_blocking=True),
                    "paths": st["paths"][:k].to(self.device, non_blocking=True),
                    "ends": st["ends"][:k].to(self.device, non_blocking=True),
                    "label": st["label"][:k].to(self.device, non_blocking=True),
                }
                ev.record(self._copy_stream)
            return db, ev

        def hand_over(db, ev):
            # the batch tensors were ALLOCATED on the copy stream; tell the
            # caching allocator they are consumed on the compute stream, or
            # their memory can be reused by a later copy while compute still
            # reads it (GPU memory fault at scale)
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            for k, v in db.items():
                if v.is_cuda:  # "id" (and a packed batch's lengths) are host
                    v.record_stream(cur)
            return db

        pending = None
        for i, lo in enumerate(range(0, n, bs)):
            nxt = stage_and_copy(i % 2, lo, min(lo + bs, n))
            if pending is not None:
                yield hand_over(*pending)
            pending = nxt
        if pending is not None:
            yield hand_over(*pending)


class PackedBatchIterator:
    """Iterates packed dict batches {'id', 'starts', 'paths', 'ends',
    'lengths', 'label'} over a ``PackedData`` in input order.

    A batch takes consecutive methods while its total rows stay within
    ``max_batch_contexts``; a method larger than the budget forms a batch
    on its own.  ``starts``/``paths``/``ends`` are flat int32 tensors on
    ``device``; ``lengths`` (int64) stays on the CPU, where
    ``forward_packed`` checks it and builds the device offsets."""

    def __init__(self, data: PackedData, max_batch_contexts: int,
                 device: Optional[torch.device] = None) -> None:
        if max_batch_contexts < 1:
            raise ValueError(
                f"max_batch_contexts must be >= 1, got {max_batch_contexts}")
        self.data = data
        self.max_batch_contexts = int(max_batch_contexts)
        self.device = device or torch.device("cpu")
        # (first method, end method, first row, end row) of every batch
        self.spans = []
        lo = row_lo = rows = 0
        for i, n in enumerate(data.lengths.tolist()):
            if i > lo and rows + n > self.max_batch_contexts:
                self.spans.append((lo, i, row_lo, row_lo + rows))
                lo, row_lo, rows = i, row_lo + rows, 0
            rows += n
        if len(data.lengths) > lo:
            self.spans.append((lo, len(data.lengths), row_lo, row_lo + rows))

    def __len__(self) -> int:
        return len(self.spans)

    def __iter__(self) -> Iterator[dict]:
        d = self.data
        for lo, hi, r0, r1 in self.spans:
            yield {
                "id": torch.as_tensor(
                    [i if i is not None else -1 for i in d.ids[lo:hi]],
                    dtype=torch.int64),
                "starts": torch.from_numpy(d.starts[r0:r1]).to(self.device),
                "paths": torch.from_numpy(d.paths[r0:r1]).to(self.device),
                "ends": torch.from_numpy(d.ends[r0:r1]).to(self.device),
                "lengths": torch.from_numpy(d.lengths[lo:hi]),
                "label": torch.from_numpy(d.labels[lo:hi]),
            }
