"""Autograd wrappers around the HIP kernels.

Each ``torch.autograd.Function`` here pairs a hand-written CDNA4 forward
kernel with its backward kernels.  Nearly every
hot GEMM ended up custom after A/B against the tuned libraries: the
combiner forward (fused LN/tanh/dropout epilogue), combiner dgrad
(dgrad2) and wgrad (split-K — the skinny big-K shape where hipBLASLt is
~3.5x off), the head forward (+online-softmax stats epilogue) and the
fused recompute-G head backward (dW/dbias/dcv).  rocBLAS/hipBLASLt
remain only where they measured faster or equal: the head forward above
the vocab gate with C2V_HF_AIMG=0.

Numerical contracts are defined by ops/reference.py; tests compare against
it in fp32.
"""

from __future__ import annotations

import os
from typing import Optional

import torch

# epilogue store scheme for combiner_fwd: 0 = per-element stores,
# 1 = per-wave LDS bounce + coalesced 16-B flush (kbench-selected)
_FWD_EPI = int(os.environ.get("C2V_FWD_EPI", "1"))
_SCATTER_R = int(os.environ.get("C2V_SCATTER_R", "16"))
# Fused gather+combiner forward, opt-in via C2V_FUSE=1.  Measured OFF-better
# on top11 (1.415 vs 1.478 ms/step): fusing saves the 61 us gather kernel but
# costs +16 us in combiner_fwd (scattered row loads inside the MFMA loop) and
# +109 us in wgrad (GATHER=1 re-gathers X every split-K pass), net +64 us.
# The split gather kernel streams at HBM BW, so there is no bandwidth win to
# recover.  Kept (correct, GPU-tested) for small-table configs where the
# gather output (B*C*KP bf16) no longer fits comfortably.
FUSE_GATHER_COMBINER = os.environ.get("C2V_FUSE") == "1"
# custom output-head forward (+ fused loss statistics); C2V_HEAD_FWD=0
# falls back to hipBLASLt linear + full-pass loss forward.  Measured
# faster through the derived top11 vocab (with normal stores + the fused
# backward: 1.403 vs 1.412 ms/step at L=72,416) but still slower at
# java-large's L=261k (strided W fragment reads stream from HBM), so
# vocabs past C2V_HEAD_FWD_MAXL take the library path.
_HEAD_FWD = os.environ.get("C2V_HEAD_FWD", "1") == "1"
_HEAD_FWD_MAXL = int(os.environ.get("C2V_HEAD_FWD_MAXL", "98304"))
# above MAXL: custom head forward consuming a swizzle_a W fragment image
# (contiguous A reads; re-enables the fused stats epilogue at java-large
# scale).  C2V_HF_AIMG=0 falls back to hipBLASLt + lsm_partial there.
_HF_AIMG = os.environ.get("C2V_HF_AIMG", "1") == "1"
# hipCUB decoupled-lookback scan for the counting-sort cursor (one launch
# vs the 3-kernel partials/spine/apply chain); C2V_SCAN_CUB=0 reverts
_SCAN_CUB = os.environ.get("C2V_SCAN_CUB", "1") == "1"
_CUB_TEMP_BYTES: dict = {}
# streaming head backward: recompute logits by MFMA inside dcv instead of
# reading the [B, L] tensor (C2V_HB_RC=0 reverts to the logits-reading
# kernel)
_HB_RC = os.environ.get("C2V_HB_RC", "0") == "1"
# custom split-K dcv in the head backward (C2V_HEAD_DGRAD=0 -> rocBLAS)
_HEAD_DGRAD = os.environ.get("C2V_HEAD_DGRAD", "1") == "1"
# combiner dgrad through dgrad2.hip (C2V_DGRAD2=0 -> rocBLAS)
_DGRAD2 = os.environ.get("C2V_DGRAD2", "1") == "1"
# fused head+loss backward (recompute-G; dlogits never materialized).
# C2V_FUSED_HEAD=0 falls back to the unfused OutputHead+FusedLogSoftmaxNLL
# chain (kept for A/B and as the general-shape path).
FUSED_HEAD = os.environ.get("C2V_FUSED_HEAD", "1") == "1"
# combiner + attention pool as ONE autograd node whose backward never
# writes the attention gradient dccv (compact attention_bwd + recomputing
# combiner_bwd) and whose forward also emits cv in bf16.  C2V_FUSED_CAP=0
# reverts to the CombinerLNTanh -> AttentionPool -> .to(bf16) chain.
FUSED_CAP = os.environ.get("C2V_FUSED_CAP", "1") == "1"
# one-launch reductions; each =0 reverts to the chain it replaced
_WGRAD_REDUCE = os.environ.get("C2V_WGRAD_REDUCE", "1") == "1"  # sum+t+cast
# Pipelined head backward (head_bwd_dw_pipe / head_bwd_dcv_pipe) and
# split-K wgrad (wgrad_pipe): the same arithmetic in the same order as the
# kernels they replace — bit-identical outputs — with the loads kept in
# flight across the MFMAs.  Only the dW/dbias kernel measured faster
# (83 -> 60 us at top11) and is on by default; the dcv and wgrad variants
# measured 2-4% SLOWER than their kernels on the same buffers (PERF.md) and
# ship off.  C2V_HB_PIPE=0 reverts every head kernel, C2V_HB_PIPE_DW /
# C2V_HB_PIPE_DCV / C2V_WGRAD_PIPE = 0 | 1 select each part.
_HB_PIPE = os.environ.get("C2V_HB_PIPE", "1") == "1"
_HB_PIPE_DW = _HB_PIPE and os.environ.get("C2V_HB_PIPE_DW", "1") == "1"
_HB_PIPE_DCV = _HB_PIPE and os.environ.get("C2V_HB_PIPE_DCV", "0") == "1"
_WGRAD_PIPE = os.environ.get("C2V_WGRAD_PIPE", "0") == "1"
_SLAB_SUM2 = os.environ.get("C2V_SLAB_SUM2", "1") == "1"  # dgamma+dbeta
# loss partials -> acc and acc[0]/acc[1] in one launch.  Same bits, one
# launch fewer, but its step-time gain could not be told from the
# run-to-run spread (PERF.md, "Backward fusions"), so it is opt-in.
_LOSS_REDUCE = os.environ.get("C2V_LOSS_REDUCE", "0") == "1"
# streaming attention pool inside CombinerAttentionPool (EP = 128, C <= 200):
# the forward takes its raw scores from combiner_fwd's flush and reads the
# combiner output once, from registers (attention_fwd_scores); the compact
# backward holds a method's rows in registers (attention_bwd_compact_reg).
# Same bits as the tiled kernels.  C2V_ATTN_STREAM=0 reverts both halves,
# C2V_ATTN_STREAM_FWD=0 / C2V_ATTN_STREAM_BWD=0 one of them.
_ATTN_STREAM = os.environ.get("C2V_ATTN_STREAM", "1") == "1"
_ATTN_STREAM_FWD = (_ATTN_STREAM
                    and os.environ.get("C2V_ATTN_STREAM_FWD", "1") == "1")
_ATTN_STREAM_BWD = (_ATTN_STREAM
                    and os.environ.get("C2V_ATTN_STREAM_BWD", "1") == "1")
_NONE_T = torch.Tensor()  # "not provided" sentinel for optional kernel args

# Owner-buffer gradient flow for the embedding tables (parallel/ddp.py):
# when a param's data_ptr is in OWNED_GRAD_KEYS, the embedding backward
# hands its finished grad tensor to EARLY_GRAD_CALLBACKS[key] the moment
# its cast_clear completes and returns None to autograd.  Autograd then
# never adopts (and possibly CLONES) the tensor — the round-1 hazard that
# made in-place early all-reduce unsafe — so the DDP layer can launch
# chunked async all-reduces on a buffer it owns while the REST of backward
# (the other table's sort/scatter chain) still runs.
EARLY_GRAD_CALLBACKS = {}
OWNED_GRAD_KEYS = set()
# Deferred table gradients (single-GPU fused step): for an owned key also
# listed here the backward runs ONLY the counting sort and hands the owner
# a DeferredTableGrad record instead of a dense bf16 table; the optimizer's
# row-gathering table Adam (adam_table_bf16) rebuilds each row's gradient
# from the record.  C2V_FUSED_TABLE_ADAM=0 is the A/B switch (read by
# parallel/ddp.py); C2V_TABLE_ADAM_HEAVY is the run length above which a
# row is pre-reduced into the fp32 scratch instead of gathered in-kernel.
DEFERRED_GRAD_KEYS = set()
_TABLE_ADAM_HEAVY = int(os.environ.get("C2V_TABLE_ADAM_HEAVY", "64"))
# Where both tables are deferred, one group_tables chain (index_group.hip)
# groups both index lists at FORWARD time — they depend on the batch only —
# and the backward adopts the result (see _launch_table_grouping).
# C2V_GROUP_TABLES=0 keeps the per-table chain inside backward.
# C2V_GROUP_SORT=0 keeps the merged chain's global-atomic kernels instead of
# the two-level sort by LDS buckets (read in index_group.hip, as are the
# sweep switches C2V_GROUP_R and C2V_GROUP_TILE).
# C2V_GROUP_STREAM=1 launches the merged chain on a side stream so that it
# overlaps the step; measured SLOWER than launching it on the forward's own
# stream (1.160-1.176 against 1.128-1.136 ms/step at top11, parent
# 1.151-1.158: the two cross-stream waits cost more than the ~75 us chain
# they hide, see PERF.md), so it is off by default.
_GROUP_TABLES = os.environ.get("C2V_GROUP_TABLES", "1") == "1"
_GROUP_STREAM = os.environ.get("C2V_GROUP_STREAM", "0") == "1"

from . import ext, round_up

_rng_state = {"seed": None, "dev_off": {}}


def _philox_state(device):
    """(seed, device offset scalar) for the counter-based dropout RNG.
    The offset lives in DEVICE memory and is advanced by the consuming
    kernel launch chain, so a hipGraph-captured training step keeps
    drawing fresh masks on every replay."""
    if _rng_state["seed"] is None:
        _rng_state["seed"] = torch.initial_seed() & 0x7FFFFFFFFFFFFFFF
    key = str(device)
    off = _rng_state["dev_off"].get(key)
    if off is None:
        off = torch.zeros(1, dtype=torch.int64, device=device)
        _rng_state["dev_off"][key] = off
    return _rng_state["seed"], off


def reseed_dropout_rng(seed: int) -> None:
    _rng_state["seed"] = seed & 0x7FFFFFFFFFFFFFFF
    for off in _rng_state["dev_off"].values():
        off.zero_()


class GatherConcat(torch.autograd.Function):
    """K1/K2 + K13: fused triple embedding gather+concat; scatter-add bwd.

    out[b*C+c] = [term[starts] (TS cols) | path[paths] (PS) | term[ends] (TS)]
    """

    @classmethod
    def apply(cls, starts, paths, ends, term_w, path_w, training=True,
              row_capacity=None):
        # forward() itself always runs with grad mode off: whether a
        # backward can follow is only visible out here
        track = bool(training) and torch.is_grad_enabled()
        return super().apply(starts, paths, ends, term_w, path_w, track,
                             row_capacity)

    @staticmethod
    def forward(ctx, starts, paths, ends, term_w, path_w, track=False,
                row_capacity=None):
        B, C = starts.shape
        TS = term_w.shape[1]
        PS = path_w.shape[1]
        out = torch.empty(
            B * C, round_up(2 * TS + PS, 32), dtype=torch.bfloat16,
            device=starts.device
        )
        # the grouping goes first so that, on its side stream, it runs
        # under the gather and everything after it
        ctx.group_ticket = (
            _launch_table_grouping(starts, paths, ends, term_w, path_w,
                                   row_capacity)
            if track else None)
        ext().gather_concat_fwd(starts, paths, ends, term_w, path_w, out)
        ctx.save_for_backward(starts, paths, ends)
        ctx.shapes = (term_w.shape, path_w.shape)
        ctx.param_keys = (term_w.data_ptr(), path_w.data_ptr())
        return out

    @staticmethod
    def backward(ctx, grad_out):
        starts, paths, ends = ctx.saved_tensors
        term_shape, path_shape = ctx.shapes
        dterm, dpath = _scatter_embedding_grads(
            starts, paths, ends, grad_out.contiguous(), term_shape,
            path_shape, ctx.param_keys[0], ctx.param_keys[1],
            ticket=ctx.group_ticket
        )
        return None, None, None, dterm, dpath, None, None


def _scatter_embedding_grads(starts, paths, ends, gout, term_shape,
                             path_shape, term_key=None, path_key=None,
                             ticket=None):
    """K13 v4: sort-based segmented scatter of a [M, KP] grad into bf16
    dense embedding grads.  Counting-sort groups the index lists; run-owner
    waves write interior rows' bf16 grads directly; boundary-crossing runs
    (heavy hitters) combine via flagged persistent fp32 scratch in
    cast_clear_rows (which also re-zeroes what it consumed).

    Deferred form: for an owned key listed in DEFERRED_GRAD_KEYS only the
    grouping runs; the owner's callback gets a DeferredTableGrad record and
    autograd gets None (see table_adam_deferred).  ``ticket`` names the
    grouping the forward launched for this batch (_launch_table_grouping):
    if it is the outstanding one, both records come from it and nothing is
    grouped here."""
    M = starts.numel()
    TS, PS = term_shape[1], path_shape[1]
    KP = gout.shape[1]

    grouping = _adopt_table_grouping(ticket, M, term_shape, path_shape,
                                     term_key, path_key)
    if grouping is not None:
        pair = _GroupedPair()
        for tag, shape, key, off0, off1 in (
                ("term", term_shape, term_key, 0, TS + PS),
                ("path", path_shape, path_key, TS, TS)):
            sorted_idx, perm, counts, cursor = grouping.tables[tag]
            rec = DeferredTableGrad(tag, gout, perm, counts, cursor,
                                    sorted_idx, M, KP, off0, off1,
                                    tuple(shape))
            rec.pair = pair
            pair.recs[tag] = rec
            _PENDING_DEFERRED[counts.data_ptr()] = rec
        # term first, as in the per-table chain below
        EARLY_GRAD_CALLBACKS[term_key](pair.recs["term"])
        EARLY_GRAD_CALLBACKS[path_key](pair.recs["path"])
        return None, None

    def one_table(tag, idx, shape, key, off0, off1):
        sorted_idx, perm, counts, cursor = _group_by_index(
            idx, shape[0], pool_tag=tag, with_cursor=True)
        rec = DeferredTableGrad(tag, gout, perm, counts, cursor, sorted_idx,
                                M, KP, off0, off1, tuple(shape))
        cb = EARLY_GRAD_CALLBACKS.get(key) if key is not None else None
        if (cb is not None and key in OWNED_GRAD_KEYS
                and key in DEFERRED_GRAD_KEYS):
            # deferred: the owner's optimizer step consumes the record
            _PENDING_DEFERRED[counts.data_ptr()] = rec
            cb(rec)
            return None
        grad = materialize_deferred(rec)
        if cb is not None:
            cb(grad)
        # the callback owner keeps the buffer; autograd must not adopt
        # (or clone) it
        return None if key in OWNED_GRAD_KEYS else grad

    # term's FULL chain (sort+scatter+cast) runs before path's STARTS, so
    # the early callback can put term's all-reduce on the wire while
    # path's ~100 us of scatter kernels still execute (DP overlap)
    idx_se = torch.cat([starts.view(-1), ends.view(-1)])
    dterm = one_table("term", idx_se, term_shape, term_key, 0, TS + PS)
    dpath = one_table("path", paths.view(-1), path_shape, path_key, TS, TS)
    return dterm, dpath


class DeferredTableGrad:
    """One embedding table's gradient as the counting sort left it: the
    sorted run of row r is [cursor[r] - counts[r], cursor[r]) and entry k
    of it is gout row perm[k] (o < M at column off0, else row o - M at
    off1).  ``counts`` is the persistent histogram, so exactly one of
    table_adam_deferred / materialize_deferred / discard_deferred must
    consume the record before the next backward regroups that table;
    ``gout`` stays alive through the record until then."""

    __slots__ = ("tag", "gout", "perm", "counts", "cursor", "sorted_idx",
                 "M", "KP", "off0", "off1", "shape", "consumed", "pair")

    def __init__(self, tag, gout, perm, counts, cursor, sorted_idx, M, KP,
                 off0, off1, shape):
        self.tag, self.gout, self.perm = tag, gout, perm
        self.counts, self.cursor, self.sorted_idx = counts, cursor, sorted_idx
        self.M, self.KP, self.off0, self.off1 = M, KP, off0, off1
        self.shape = shape
        self.consumed = False
        self.pair = None  # _GroupedPair of a group_tables record

    def _consume(self):
        if self.consumed:
            raise RuntimeError("deferred table gradient consumed twice")
        self.consumed = True
        key = self.counts.data_ptr()
        if _PENDING_DEFERRED.get(key) is self:
            del _PENDING_DEFERRED[key]

    def _release(self):
        self.gout = self.perm = self.sorted_idx = None


# counts buffer address -> record handed out and not yet consumed (the
# histogram it describes is still in that buffer)
_PENDING_DEFERRED = {}


class _GroupedPair:
    """The two records of one group_tables call.  While both go through
    table_adam_deferred, the heavy-row pre-pass runs once for both tables
    (before the first Adam) and both histograms are cleared in one launch
    (after the second Adam: several threads of an Adam kernel read each
    row's count, so no clear may overtake it).  A record consumed any other
    way breaks the pair (_leave_pair) and what is left runs per table."""

    __slots__ = ("recs", "prepassed", "stepped", "broken")

    def __init__(self):
        self.recs = {}
        self.prepassed = False
        self.stepped = []
        self.broken = False


def _leave_pair(rec: "DeferredTableGrad") -> None:
    """``rec`` is about to be materialized or discarded, not stepped."""
    pair = rec.pair
    if pair is None:
        return
    if pair.prepassed:
        # its heavy rows sit in the scratch for an Adam that will not run
        _scratch_f32(rec.tag, rec.shape, rec.counts.device).zero_()
    if not pair.broken:
        pair.broken = True
        # an Adam that already ran left its histogram for the merged clear
        for other in pair.stepped:
            other.counts.zero_()


def materialize_deferred(rec: DeferredTableGrad) -> torch.Tensor:
    """Dense bf16 gradient table from a record: the sorted scatter plus
    cast_clear_rows (which consumes counts/flags and re-zeroes the fp32
    scratch rows it read)."""
    rec._consume()
    _leave_pair(rec)
    dev = rec.gout.device
    d32 = _scratch_f32(rec.tag, rec.shape, dev)
    flags = _scratch_flags(rec.tag, rec.shape[0], dev)
    grad = torch.empty(rec.shape, dtype=torch.bfloat16, device=dev)
    ext().embed_scatter_sorted(rec.sorted_idx, rec.perm, rec.gout, d32, grad,
                               flags, rec.M, rec.KP, rec.off0, rec.off1,
                               _SCATTER_R)
    ext().cast_clear_rows(d32, rec.counts, flags, grad)
    rec._release()
    return grad


def discard_deferred(rec: DeferredTableGrad) -> None:
    """Drop an unconsumed record (a backward with no optimizer step).  Only
    the histogram was written so far: flags and the fp32 scratch are still
    all-zero, so re-zeroing counts restores every invariant."""
    if rec.consumed:
        return
    rec._consume()
    _leave_pair(rec)
    rec.counts.zero_()
    rec._release()


def table_adam_deferred(param, master, m, v, rec: DeferredTableGrad, bc_pow,
                        lr, beta1, beta2, eps, weight_decay) -> None:
    """K16b: Adam on a whole bf16 table straight from a deferred record —
    heavy rows pre-reduced into the fp32 scratch, every other row's
    gradient gathered inside the Adam kernel.  Leaves counts and the
    scratch all-zero (flags are never set on this path)."""
    rec._consume()
    assert tuple(param.shape) == rec.shape and master is not None
    scratch = _scratch_f32(rec.tag, rec.shape, param.device)
    pair = rec.pair
    if pair is not None and not pair.broken:
        # records of one group_tables call: one pre-pass and one clear for
        # both tables
        t, p = pair.recs["term"], pair.recs["path"]
        if not pair.prepassed:
            ext().embed_scatter_heavy_pair(
                t.sorted_idx, t.perm, t.counts,
                _scratch_f32("term", t.shape, param.device),
                p.sorted_idx, p.perm, p.counts,
                _scratch_f32("path", p.shape, param.device),
                rec.gout, rec.M, rec.KP, _TABLE_ADAM_HEAVY)
            pair.prepassed = True
        ext().adam_table_bf16_keep_counts(
            param, rec.gout, rec.perm, rec.counts, rec.cursor, scratch,
            master, m, v, bc_pow, rec.M, rec.KP, rec.off0, rec.off1,
            _TABLE_ADAM_HEAVY, lr, beta1, beta2, eps, weight_decay)
        pair.stepped.append(rec)
        if len(pair.stepped) == 2:
            ext().clear_i32_pair(t.counts, p.counts)
            pair.recs = {}
        rec._release()
        return
    if pair is None or not pair.prepassed:
        ext().embed_scatter_heavy(rec.sorted_idx, rec.perm, rec.counts,
                                  rec.gout, scratch, rec.M, rec.KP, rec.off0,
                                  rec.off1, _TABLE_ADAM_HEAVY)
    ext().adam_table_bf16(param, rec.gout, rec.perm, rec.counts, rec.cursor,
                          scratch, master, m, v, bc_pow, rec.M, rec.KP,
                          rec.off0, rec.off1, _TABLE_ADAM_HEAVY, lr, beta1,
                          beta2, eps, weight_decay)
    rec._release()


class _TableGrouping:
    """One group_tables call whose records no backward has taken yet."""

    __slots__ = ("ticket", "index_tensors", "tables", "on_side", "M",
                 "shapes", "keys")


_group_state = {"outstanding": None, "next_ticket": 1}


def _grouping_applies(term_key, path_key) -> bool:
    return all(k is not None and k in OWNED_GRAD_KEYS
               and k in DEFERRED_GRAD_KEYS and k in EARLY_GRAD_CALLBACKS
               for k in (term_key, path_key))


def _launch_table_grouping(starts, paths, ends, term_w, path_w,
                           row_capacity=None):
    """Group both tables' indices for the backward of this forward and
    return the ticket that backward adopts them with, or None where the
    deferred table gradient does not apply (then backward groups per table
    as before).  At most one grouping is outstanding: one that no backward
    adopted is retired first.

    ``row_capacity`` (packed batches, whose row count M differs from step
    to step): the row-sized buffers are allocated once for that many rows
    and the kernels get [:n] views, so the scratch cache does not grow by a
    set of buffers per distinct M.  None keeps the padded path's keys."""
    if row_capacity is not None and starts.numel() > row_capacity:
        raise ValueError(
            f"packed batch has {starts.numel()} rows, over the row capacity "
            f"{row_capacity} its scratch was sized for")
    if not (_GROUP_TABLES and starts.is_cuda and term_w.requires_grad
            and path_w.requires_grad
            and _grouping_applies(term_w.data_ptr(), path_w.data_ptr())
            and starts.dtype == paths.dtype == ends.dtype == torch.int32
            and starts.is_contiguous() and paths.is_contiguous()
            and ends.is_contiguous() and starts.numel() > 0):
        return None
    retire_table_grouping()
    dev = starts.device
    M = starts.numel()
    g = _TableGrouping()
    g.tables = {}
    bufs = {}
    for tag, rows, n in (("term", term_w.shape[0] + 1, 2 * M),
                         ("path", path_w.shape[0] + 1, M)):
        counts = _scratch_i32(f"counts_{tag}", rows, dev)
        # a deferred record nobody consumed still holds its histogram here
        stale = _PENDING_DEFERRED.get(counts.data_ptr())
        if stale is not None:
            discard_deferred(stale)
        cursor = _scratch_i32(f"cursor_{tag}", rows, dev, zero=False)
        if row_capacity is None:
            sorted_idx = _scratch_i32(f"gsorted_{tag}", n, dev, zero=False)
            perm = _scratch_i64(f"gperm_{tag}", n, dev)
        else:
            cap = (n // M) * int(row_capacity)
            sorted_idx = _scratch_i32(f"gsorted_cap_{tag}", cap, dev,
                                      zero=False)[:n]
            perm = _scratch_i64(f"gperm_cap_{tag}", cap, dev)[:n]
        g.tables[tag] = (sorted_idx, perm, counts, cursor)
        bufs[tag] = rows
    spart = _scratch_i32(
        "gscanp", int(ext().group_tables_partials_len(bufs["term"],
                                                      bufs["path"])),
        dev, zero=False)
    # the two-level sort's M-sized scratch: persistent like the records,
    # one buffer per row capacity on the packed path
    tmp_n = int(ext().group_tables_tmp_len(M, bufs["term"], bufs["path"]))
    if row_capacity is None:
        gtmp = _scratch_i32("gtmp", tmp_n, dev, zero=False)
    else:
        gtmp = _scratch_i32(
            "gtmp_cap", int(ext().group_tables_tmp_len(
                int(row_capacity), bufs["term"], bufs["path"])),
            dev, zero=False)[:tmp_n]
    st, sp = g.tables["term"], g.tables["path"]
    g.on_side = bool(ext().group_tables(
        starts, paths, ends, st[2], sp[2], st[3], sp[3], spart, st[0], st[1],
        sp[0], sp[1], bufs["term"], bufs["path"], _GROUP_STREAM, gtmp))
    # the side-stream kernels read these: they stay alive here until a
    # backward adopts the grouping (whose ctx holds them too) or it is
    # retired, both of which order the current stream after the kernels
    g.index_tensors = (starts, paths, ends)
    g.M = M
    g.shapes = (tuple(term_w.shape), tuple(path_w.shape))
    g.keys = (term_w.data_ptr(), path_w.data_ptr())
    g.ticket = _group_state["next_ticket"]
    _group_state["next_ticket"] += 1
    _group_state["outstanding"] = g
    return g.ticket


def _adopt_table_grouping(ticket, M, term_shape, path_shape, term_key,
                          path_key):
    """The outstanding grouping if ``ticket`` names it and it still fits
    this backward, with the current stream ordered after its kernels; else
    None, after retiring whatever was outstanding."""
    g = _group_state["outstanding"]
    if g is None:
        return None
    if (ticket is None or g.ticket != ticket or g.M != M
            or g.shapes != (tuple(term_shape), tuple(path_shape))
            or g.keys != (term_key, path_key)
            or not _grouping_applies(term_key, path_key)):
        retire_table_grouping()
        return None
    _group_state["outstanding"] = None
    if g.on_side:
        ext().group_tables_wait()
    return g


def retire_table_grouping() -> None:
    """Drop a grouping no backward adopted (a training forward without a
    backward, a second forward before the first backward): wait for its
    kernels and re-zero both histograms, which is all it wrote that carries
    an invariant."""
    g = _group_state["outstanding"]
    if g is None:
        return
    _group_state["outstanding"] = None
    if g.on_side:
        ext().group_tables_wait()
    for tag in ("term", "path"):
        g.tables[tag][2].zero_()


_scratch_cache = {}


def _scratch_f32(tag: str, shape, device) -> torch.Tensor:
    """Persistent fp32 scatter scratch (invariant: all-zero between steps —
    maintained by cast_clear_rows).  ``tag`` keeps the term/path buffers
    distinct even when both tables have identical shapes."""
    key = (tag, tuple(shape), str(device))
    buf = _scratch_cache.get(key)
    if buf is None:
        buf = torch.zeros(shape, dtype=torch.float32, device=device)
        _scratch_cache[key] = buf
    return buf


def _scratch_bf16(tag: str, shape, device) -> torch.Tensor:
    """Persistent bf16 scratch (fully overwritten by its producer)."""
    key = ("bf16", tag, tuple(shape), str(device))
    buf = _scratch_cache.get(key)
    if buf is None:
        buf = torch.empty(shape, dtype=torch.bfloat16, device=device)
        _scratch_cache[key] = buf
    return buf


def _scratch_i32(tag: str, n: int, device, zero: bool = True) -> torch.Tensor:
    """Persistent int32 scratch; ``zero=True`` buffers carry an all-zero
    invariant between steps (maintained by their consumer)."""
    key = ("i32", tag, n, str(device))
    buf = _scratch_cache.get(key)
    if buf is None:
        maker = torch.zeros if zero else torch.empty
        buf = maker(n, dtype=torch.int32, device=device)
        _scratch_cache[key] = buf
    return buf


def _scratch_i64(tag: str, n: int, device) -> torch.Tensor:
    """Persistent int64 scratch (fully overwritten by its producer)."""
    key = ("i64", tag, n, str(device))
    buf = _scratch_cache.get(key)
    if buf is None:
        buf = torch.empty(n, dtype=torch.int64, device=device)
        _scratch_cache[key] = buf
    return buf


def _scratch_u8(tag: str, n: int, device) -> torch.Tensor:
    key = ("u8", tag, n, str(device))
    buf = _scratch_cache.get(key)
    if buf is None:
        buf = torch.empty(n, dtype=torch.uint8, device=device)
        _scratch_cache[key] = buf
    return buf


def _scratch_flags(tag: str, rows: int, device) -> torch.Tensor:
    key = ("flags", tag, rows, str(device))
    buf = _scratch_cache.get(key)
    if buf is None:
        buf = torch.zeros(rows, dtype=torch.uint8, device=device)
        _scratch_cache[key] = buf
    return buf


def _combiner_dgrad(dz: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dx = dz @ w ([M, EP] @ [EP, KP], K = EP = 128) — a 131-MB
    streaming write that hipBLASLt runs 3x off its floor (MT64x256x64,
    91 us at top11).  dgrad2.hip computes it transposed-orientation with
    the weight re-transposed to [KP, EP]: both fragments contiguous,
    dz tiles staged block-cooperatively, packed full-line nontemporal
    stores; 128-row batch tiles keep per-wave overhead half of a naive
    head_fwd reuse (which measured a wash — see PERF.md)."""
    M, EP = dz.shape
    KP = w.shape[1]
    if not (_DGRAD2 and dz.is_cuda and EP == 128 and KP % 8 == 0):
        return dz @ w
    w2 = w.t().contiguous()  # [KP, EP], 82 KB at top11
    dx = torch.empty(M, KP, dtype=torch.bfloat16, device=w.device)
    ext().dgrad2(dz, w2, dx)
    return dx


def _slab_sum(p: torch.Tensor) -> torch.Tensor:
    """Sum reduction-partial slabs [S, N] -> [N] f32 (block-per-column
    kernel; torch's generic reduce costs ~10 us per call at these tiny
    shapes)."""
    out = torch.empty(p.shape[-1], dtype=torch.float32, device=p.device)
    ext().slab_sum_f32(p, out)
    return out


def _slab_sum_pair(p0: torch.Tensor, p1: torch.Tensor):
    """Two equal-shape partial slabs [S, N] -> two [N] f32 sums in ONE
    launch (the dgamma/dbeta pair); same per-column tree, same bits as
    two _slab_sum calls."""
    if not _SLAB_SUM2:
        return _slab_sum(p0), _slab_sum(p1)
    out0 = torch.empty(p0.shape[-1], dtype=torch.float32, device=p0.device)
    out1 = torch.empty_like(out0)
    ext().slab_sum2_f32(p0, p1, out0, out1)
    return out0, out1


def _wgrad_reduce(partials: torch.Tensor) -> torch.Tensor:
    """Split-K wgrad slabs [S, KP, EP] f32 -> dw [EP, KP] bf16.  One
    kernel sums, transposes and casts (fixed summation order, see
    wgrad_reduce_kernel); C2V_WGRAD_REDUCE=0 is the torch
    sum -> .t().contiguous() -> .to(bf16) chain it replaced, whose reduce
    order differs in the last bits."""
    S, KP, EP = partials.shape
    if not (_WGRAD_REDUCE and partials.is_cuda and KP % 4 == 0
            and EP % 32 == 0):
        return partials.sum(dim=0).t().contiguous().to(torch.bfloat16)
    dw = torch.empty(EP, KP, dtype=torch.bfloat16, device=partials.device)
    ext().wgrad_reduce(partials, dw)
    return dw


def _group_by_index(idx: torch.Tensor, table_rows: int,
                    pool_tag: Optional[str] = None,
                    with_cursor: bool = False):
    """Counting sort: returns (sorted_idx i32, perm i64, counts i32)
    grouping equal indexes contiguously (ascending); ``with_cursor`` also
    returns the cursor, which scatter_group leaves at each run's END.

    With ``pool_tag`` (the training hot path) the histogram lives in a
    PERSISTENT all-zero buffer whose invariant cast_clear_rows restores
    by consuming the counts it reads, and the cursor comes from the
    custom 3-kernel exclusive scan — this removes two torch.zeros fills
    and a rocprim lookback scan (+init) per table per step (~21 us each).
    Callers that do NOT route the counts through cast_clear_rows (or the
    table Adam, which clears them too) must use the default (fresh-buffer)
    form.
    """
    N = idx.numel()
    dev = idx.device
    if pool_tag is not None:
        # a forward-time grouping nobody adopted may hold this histogram
        retire_table_grouping()
        counts = _scratch_i32(f"counts_{pool_tag}", table_rows + 1, dev)
        # a deferred record nobody consumed (backward without a step)
        # still holds its histogram in this buffer
        stale = _PENDING_DEFERRED.get(counts.data_ptr())
        if stale is not None:
            discard_deferred(stale)
        cursor = _scratch_i32(f"cursor_{pool_tag}", table_rows + 1, dev,
                              zero=False)
        spart = _scratch_i32(f"scanp_{pool_tag}",
                             (table_rows + 1 + 1023) // 1024, dev,
                             zero=False)
    else:
        counts = torch.zeros(table_rows + 1, dtype=torch.int32, device=dev)
        cursor = None
    empty_i = torch.empty(0, dtype=torch.int32, device=dev)
    empty_l = torch.empty(0, dtype=torch.int64, device=dev)
    ext().group_by_index(idx, counts, empty_i, empty_i, empty_l, True)
    if pool_tag is not None:
        if _SCAN_CUB:
            tb = _CUB_TEMP_BYTES.get(table_rows + 1)
            if tb is None:
                tb = int(ext().cub_scan_temp_bytes(table_rows + 1))
                _CUB_TEMP_BYTES[table_rows + 1] = tb
            temp = _scratch_u8(f"cubscan_{pool_tag}", max(tb, 16), dev)
            ext().cub_exclusive_scan(counts, temp, cursor)
        else:
            ext().exclusive_scan(counts, spart, cursor)
    else:
        cursor = torch.zeros_like(counts)
        cursor[1:] = torch.cumsum(counts[:-1], 0)
    sorted_idx = torch.empty(N, dtype=torch.int32, device=dev)
    perm = torch.empty(N, dtype=torch.int64, device=dev)
    ext().group_by_index(idx, counts, cursor, sorted_idx, perm, False)
    if with_cursor:
        return sorted_idx, perm, counts, cursor
    return sorted_idx, perm, counts


def _combiner_dx_dw(x, w, dz):
    """dx and dw of the combiner GEMM from dz (shared by CombinerLNTanh and
    CombinerAttentionPool backward)."""
    M, EP = dz.shape
    # dgrad: plain GEMM -> rocBLAS (TunableOp-tuned).  A hand-written
    # direct-fragment kernel (ops/csrc/dgrad.hip) measured 192 us vs
    # rocBLAS's 64 us at the top11 shape (8-wave full-KP duplicates B
    # L2 traffic) and is kept only as a reference; re-enable via
    # C2V_CUSTOM_DGRAD=1 for experiments.
    if os.environ.get("C2V_CUSTOM_DGRAD") == "1":
        w2 = w.t().contiguous()
        dx = torch.empty(M, w.shape[1], dtype=torch.bfloat16,
                         device=w.device)
        ext().dgrad(dz, w2, dx)
    else:
        dx = _combiner_dgrad(dz, w)
    # wgrad: custom split-K MFMA kernel for the skinny big-K shape
    # (hipBLASLt is ~3.5x off there); partial slabs summed here.
    KP = x.shape[1]
    if EP <= 128 and KP <= 512:
        nsplit = 256
        partials = torch.empty(nsplit, KP, EP, dtype=torch.float32,
                               device=x.device)
        # two 32-row K-steps of fragment images must fit the 160-KB LDS
        if _WGRAD_PIPE and EP == 128 and KP % 16 == 0 and KP <= 480:
            ext().wgrad_pipe(x, dz, partials, 0)
        else:
            ext().wgrad(x, dz, partials)
        dw = _wgrad_reduce(partials)
    else:
        dw = (x.t() @ dz).t().contiguous()
    return dx, dw


class CombinerLNTanh(torch.autograd.Function):
    """K3-K6: MFMA GEMM (x @ w) -> LayerNorm(E) -> tanh -> dropout, fused.

    x: bf16 [M, KP]; w: bf16 [EP, KP] (TRANSPOSED so the MFMA B fragment
    is memory-contiguous); gamma/beta: f32 [EP]; E = valid cols.
    Saves z (pre-LN GEMM output, bf16) + per-row mean/rstd for backward;
    the dropout mask is recomputed from the counter RNG, never stored.
    """

    @staticmethod
    def forward(ctx, x, w, gamma, beta, E: int, p: float, training: bool):
        M = x.shape[0]
        EP = w.shape[0]
        out = torch.empty(M, EP, dtype=torch.bfloat16, device=x.device)
        z = torch.empty(M, EP, dtype=torch.bfloat16, device=x.device)
        mean = torch.empty(M, dtype=torch.float32, device=x.device)
        rstd = torch.empty(M, dtype=torch.float32, device=x.device)
        p_eff = float(p) if training else 0.0
        seed, off_t = (_philox_state(x.device) if p_eff > 0.0
                       else (0, _philox_state(x.device)[1]))
        ext().combiner_fwd(x, w, gamma, beta, out, z, mean, rstd, E, p_eff,
                           seed, off_t, _FWD_EPI)
        ctx.save_for_backward(x, w, gamma, beta, z, mean, rstd, out)
        ctx.meta = (E, p_eff)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, gamma, beta, z, mean, rstd, out = ctx.saved_tensors
        E, p = ctx.meta
        M, EP = z.shape
        dz = torch.empty(M, EP, dtype=torch.bfloat16, device=z.device)
        # per-block partials (kernel grid cap = 1024): summed here, which is
        # deterministic and avoids same-address atomic serialization
        nblocks = min((M + 4 - 1) // 4, 1024)
        dgamma_p = torch.empty(nblocks, EP, dtype=torch.float32, device=z.device)
        dbeta_p = torch.empty(nblocks, EP, dtype=torch.float32, device=z.device)
        ext().combiner_bwd(
            dout.contiguous(), z, out, mean, rstd, gamma, beta, dz, dgamma_p,
            dbeta_p, E, p,
        )
        dgamma, dbeta = _slab_sum_pair(dgamma_p, dbeta_p)
        dx, dw = _combiner_dx_dw(x, w, dz)
        return dx, dw, dgamma, dbeta, None, None, None


class FusedGatherCombiner(torch.autograd.Function):
    """K1-K6 fully fused: embedding gather + MFMA combiner GEMM + LN + tanh
    + dropout in ONE kernel — the [M, KP] concat tensor is never
    materialized on the forward path.  Backward: fused LN/tanh/dropout
    chain -> dz; dW via the re-gathering split-K wgrad; dX (for the
    embedding scatter) via one rocBLAS GEMM; embedding grads via the
    sort-based scatter."""

    @staticmethod
    def forward(ctx, starts, paths, ends, term_w, path_w, w, gamma, beta,
                E: int, p: float, training: bool):
        M = starts.numel()
        EP, KP = w.shape
        dev = starts.device
        out = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        z = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        mean = torch.empty(M, dtype=torch.float32, device=dev)
        rstd = torch.empty(M, dtype=torch.float32, device=dev)
        p_eff = float(p) if training else 0.0
        seed, off_t = (_philox_state(dev) if p_eff > 0.0
                       else (0, _philox_state(dev)[1]))
        ext().gather_combiner_fwd(starts, paths, ends, term_w, path_w, w,
                                  gamma, beta, out, z, mean, rstd, KP, E,
                                  p_eff, seed, off_t)
        ctx.save_for_backward(starts, paths, ends, term_w, path_w, w, gamma,
                              beta, z, mean, rstd, out)
        ctx.meta = (E, p_eff)
        return out

    @staticmethod
    def backward(ctx, dout):
        (starts, paths, ends, term_w, path_w, w, gamma, beta, z, mean, rstd,
         out) = ctx.saved_tensors
        E, p = ctx.meta
        M, EP = z.shape
        KP = w.shape[1]
        dz = torch.empty(M, EP, dtype=torch.bfloat16, device=z.device)
        nblocks = min((M + 4 - 1) // 4, 1024)
        dgamma_p = torch.empty(nblocks, EP, dtype=torch.float32, device=z.device)
        dbeta_p = torch.empty(nblocks, EP, dtype=torch.float32, device=z.device)
        ext().combiner_bwd(dout.contiguous(), z, out, mean, rstd, gamma,
                           beta, dz, dgamma_p, dbeta_p, E, p)
        dgamma, dbeta = _slab_sum_pair(dgamma_p, dbeta_p)
        # dW: re-gathering split-K wgrad (X is never materialized)
        if EP <= 128 and KP <= 512:
            partials = torch.empty(256, KP, EP, dtype=torch.float32,
                                   device=z.device)
            ext().wgrad_gather(starts, paths, ends, term_w, path_w, dz,
                               partials, KP)
            dw = _wgrad_reduce(partials)
        else:
            x = GatherConcat.apply(starts, paths, ends, term_w, path_w)
            dw = (x.t() @ dz).t().contiguous()
        # dX for the embedding scatter
        dx = _combiner_dgrad(dz, w)
        dterm, dpath = _scatter_embedding_grads(
            starts, paths, ends, dx, term_w.shape, path_w.shape,
            term_w.data_ptr(), path_w.data_ptr()
        )
        return (None, None, None, dterm, dpath, dw, dgamma, dbeta,
                None, None, None)


class AttentionPool(torch.autograd.Function):
    """K7-K9 fused: masked single-query attention + weighted pool.

    ccv: bf16 [B, C, EP]; a: f32 [EP]; starts: i32 [B, C] (mask = starts>0).
    Returns cv f32 [B, EP] and attn f32 [B, C].
    """

    @staticmethod
    def forward(ctx, ccv, a, starts, E: int):
        B, C, EP = ccv.shape
        cv = torch.empty(B, EP, dtype=torch.float32, device=ccv.device)
        attn = torch.empty(B, C, dtype=torch.float32, device=ccv.device)
        ext().attention_fwd(ccv, a, starts, cv, attn, E)
        ctx.save_for_backward(ccv, a, starts, attn)
        ctx.E = E
        ctx.set_materialize_grads(False)
        return cv, attn

    @staticmethod
    def backward(ctx, dcv, dattn):
        ccv, a, starts, attn = ctx.saved_tensors
        B, C, EP = ccv.shape
        if dcv is None:
            dcv = torch.zeros(B, EP, dtype=torch.float32, device=ccv.device)
        dccv = torch.empty_like(ccv)
        # per-block partials [B, EP], summed here (deterministic, no atomics)
        da_p = torch.empty(B, EP, dtype=torch.float32, device=ccv.device)
        has_dattn = dattn is not None
        if not has_dattn:
            dattn = torch.empty(0, dtype=torch.float32, device=ccv.device)
        ext().attention_bwd(
            dcv.contiguous(), dattn.contiguous() if has_dattn else dattn,
            ccv, a, starts, attn, dccv, da_p, ctx.E, has_dattn,
        )
        return dccv, _slab_sum(da_p), None, None


# rows up to which K21 keeps a method's scores in LDS (longer methods park
# them in their attn slice); the extension checks it against the compiled
# value.  Exposed so tests can plant lengths on the boundary.
ATTN_PACKED_CHUNK = 256


def attention_pool_packed(ccv: torch.Tensor, a: torch.Tensor,
                          starts: torch.Tensor, lengths, E: int, out=None):
    """K21: masked attention pool over a packed batch, forward only.

    ccv: bf16 [M, EP], the rows of all methods back to back; a: f32 [EP];
    starts: i32 [M] (mask = starts > 0); lengths: the methods' row counts
    as a list or a CPU int32/int64 tensor.  They are checked here on the
    host (every n >= 1, sum == M; ValueError before anything is launched)
    and the device offsets the kernel trusts are built from them here and
    nowhere else.  Returns (cv f32 [B, EP], cvb bf16 [B, EP], attn f32
    [M]).  A method's result depends on its own rows only, bit for bit.
    ``out`` = (cv, cvb, attn) writes into the caller's buffers (the
    binding checks them).  CPU tensors take
    ops/reference.py::attention_pool_packed."""
    from . import reference as R

    if ccv.dim() != 2:
        raise ValueError(
            f"attention_pool_packed: ccv must be [M, EP], got "
            f"{tuple(ccv.shape)}")
    M, EP = ccv.shape
    lens = R.check_packed_lengths(lengths, M)
    if starts.numel() != M:
        raise ValueError(
            f"attention_pool_packed: starts has {starts.numel()} entries "
            f"for {M} rows")
    if not ccv.is_cuda:
        return R.attention_pool_packed(ccv, a, starts, lens, E)
    B = lens.numel()
    dev = ccv.device
    offsets = torch.zeros(B + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(lens, 0)
    offsets = offsets.to(dev)
    if out is not None:
        cv, cvb, attn = out
    else:
        cv = torch.empty(B, EP, dtype=torch.float32, device=dev)
        cvb = torch.empty(B, EP, dtype=torch.bfloat16, device=dev)
        attn = torch.empty(M, dtype=torch.float32, device=dev)
    ext().attention_pool_packed(ccv, a, starts.reshape(-1), offsets, cv, cvb,
                                attn, int(E), ATTN_PACKED_CHUNK)
    return cv, cvb, attn


def packed_offsets(lengths, M: int, device, offsets=None):
    """Host check of a packed batch's lengths (every n >= 1, sum == M;
    ValueError before anything is launched) and the device offsets [B+1]
    i32 the segmented kernels trust.  ``offsets`` may hand in device
    offsets a loader already built from these same lengths (then no
    host-to-device copy happens here); only their place and size are
    checked.  Returns (lens CPU i64, offsets)."""
    from . import reference as R

    lens = R.check_packed_lengths(lengths, M)
    B = lens.numel()
    if offsets is None:
        offsets = torch.zeros(B + 1, dtype=torch.int32)
        offsets[1:] = torch.cumsum(lens, 0)
        offsets = offsets.to(device)
    elif (offsets.device != torch.device(device)
          or offsets.dtype != torch.int32 or offsets.numel() != B + 1
          or not offsets.is_contiguous()):
        raise ValueError(
            f"packed offsets must be a contiguous int32 tensor of "
            f"{B + 1} entries on {device}")
    return lens, offsets


class AttentionPoolPacked(torch.autograd.Function):
    """K21 forward + dense K22 backward: the attention pool over a packed
    batch as an autograd node, for any EP (a multiple of 32, <= 384).

    ccv: bf16 [M, EP]; a: f32 [EP]; starts: i32 [M]; offsets: i32 [B+1] on
    the device (packed_offsets).  Returns cv f32 [B, EP] and attn f32 [M].
    """

    @staticmethod
    def forward(ctx, ccv, a, starts, offsets, E: int):
        M, EP = ccv.shape
        B = offsets.numel() - 1
        dev = ccv.device
        cv = torch.empty(B, EP, dtype=torch.float32, device=dev)
        cvb = torch.empty(B, EP, dtype=torch.bfloat16, device=dev)
        attn = torch.empty(M, dtype=torch.float32, device=dev)
        ext().attention_pool_packed(ccv, a, starts, offsets, cv, cvb, attn,
                                    int(E), ATTN_PACKED_CHUNK)
        ctx.save_for_backward(ccv, a, starts, offsets, attn)
        ctx.E = int(E)
        ctx.set_materialize_grads(False)
        return cv, attn

    @staticmethod
    def backward(ctx, dcv, dattn):
        ccv, a, starts, offsets, attn = ctx.saved_tensors
        M, EP = ccv.shape
        B = offsets.numel() - 1
        dev = ccv.device
        if dcv is None:
            dcv = torch.zeros(B, EP, dtype=torch.float32, device=dev)
        dccv = torch.empty_like(ccv)
        # where a method longer than the LDS chunk parks its g/ds
        ds_ws = torch.empty(M, dtype=torch.float32, device=dev)
        da_p = torch.empty(B, EP, dtype=torch.float32, device=dev)
        has_dattn = dattn is not None
        ext().attention_packed_bwd(
            dcv.contiguous(), dattn.contiguous() if has_dattn else _NONE_T,
            ccv, a, starts, offsets, attn, dccv, ds_ws, da_p, ctx.E,
            has_dattn, ATTN_PACKED_CHUNK)
        return dccv, _slab_sum(da_p), None, None, None


class CombinerAttentionPoolPacked(torch.autograd.Function):
    """CombinerAttentionPool over a packed batch (EP = 128): combiner_fwd
    on the M rows (dropout in training), then K21; returns (cv f32 [B, EP],
    attn [M], cvb bf16 [B, EP]).  Backward is the compact K22 (ds [M], the
    row -> method map seg [M] and the da partials), then
    combiner_bwd_recompute_packed, which rebuilds each dccv element in
    registers through dccv_elem with the method taken from seg, then the
    shared dx/dw.  dccv [M, EP] is never written."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, a, starts, offsets, E: int, p: float,
                training: bool):
        M = x.shape[0]
        EP = w.shape[0]
        B = offsets.numel() - 1
        assert EP == 128 and starts.numel() == M
        dev = x.device
        out = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        z = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        mean = torch.empty(M, dtype=torch.float32, device=dev)
        rstd = torch.empty(M, dtype=torch.float32, device=dev)
        p_eff = float(p) if training else 0.0
        seed, off_t = (_philox_state(dev) if p_eff > 0.0
                       else (0, _philox_state(dev)[1]))
        ext().combiner_fwd(x, w, gamma, beta, out, z, mean, rstd, E, p_eff,
                           seed, off_t, _FWD_EPI)
        cv = torch.empty(B, EP, dtype=torch.float32, device=dev)
        cvb = torch.empty(B, EP, dtype=torch.bfloat16, device=dev)
        attn = torch.empty(M, dtype=torch.float32, device=dev)
        ext().attention_pool_packed(out, a, starts, offsets, cv, cvb, attn,
                                    int(E), ATTN_PACKED_CHUNK)
        ctx.save_for_backward(x, w, gamma, beta, a, starts, offsets, z, mean,
                              rstd, out, attn)
        ctx.meta = (int(E), p_eff)
        ctx.set_materialize_grads(False)
        return cv, attn, cvb

    @staticmethod
    def backward(ctx, dcv32, dattn, dcvb):
        (x, w, gamma, beta, a, starts, offsets, z, mean, rstd, out,
         attn) = ctx.saved_tensors
        E, p = ctx.meta
        M, EP = z.shape
        B = offsets.numel() - 1
        dev = z.device
        if dcv32 is not None and dcvb is not None:
            dcv = dcv32 + dcvb  # f32 sum, as autograd's accumulation did
        elif dcvb is not None:
            dcv = dcvb          # bf16, read by the kernels as is
        elif dcv32 is not None:
            dcv = dcv32
        else:
            dcv = torch.zeros(B, EP, dtype=torch.float32, device=dev)
        dcv = dcv.contiguous()
        ds = torch.empty(M, dtype=torch.float32, device=dev)
        seg = torch.empty(M, dtype=torch.int32, device=dev)
        da_p = torch.empty(B, EP, dtype=torch.float32, device=dev)
        has_dattn = dattn is not None
        ext().attention_packed_bwd_compact(
            dcv, dattn.contiguous() if has_dattn else _NONE_T, out, a,
            starts, offsets, attn, ds, seg, da_p, E, has_dattn,
            ATTN_PACKED_CHUNK)
        da = _slab_sum(da_p)
        dz = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        nblocks = min((M + 4 - 1) // 4, 1024)
        dgamma_p = torch.empty(nblocks, EP, dtype=torch.float32, device=dev)
        dbeta_p = torch.empty(nblocks, EP, dtype=torch.float32, device=dev)
        ext().combiner_bwd_recompute_packed(attn, ds, dcv, a, seg, z, out,
                                            mean, rstd, gamma, beta, dz,
                                            dgamma_p, dbeta_p, E, p)
        dgamma, dbeta = _slab_sum_pair(dgamma_p, dbeta_p)
        dx, dw = _combiner_dx_dw(x, w, dz)
        return dx, dw, dgamma, dbeta, da, None, None, None, None, None


def _check_packed_pool_args(name, rows, EP, starts):
    if EP % 32 != 0 or not 32 <= EP <= 384:
        raise ValueError(
            f"{name}: EP must be a multiple of 32 in 32..384, got {EP}")
    if starts.numel() != rows:
        raise ValueError(
            f"{name}: starts has {starts.numel()} entries for {rows} rows")


def attention_pool_packed_train(ccv, a, starts, lengths, E: int,
                                offsets=None):
    """Differentiable attention_pool_packed (AttentionPoolPacked): the
    lengths are checked on the host first, as there.  Returns (cv f32
    [B, EP], attn f32 [M])."""
    if ccv.dim() != 2:
        raise ValueError(
            f"attention_pool_packed_train: ccv must be [M, EP], got "
            f"{tuple(ccv.shape)}")
    M, EP = ccv.shape
    _, offsets = packed_offsets(lengths, M, ccv.device, offsets)
    _check_packed_pool_args("attention_pool_packed_train", M, EP, starts)
    return AttentionPoolPacked.apply(ccv, a, starts.reshape(-1).contiguous(),
                                     offsets, int(E))


def combiner_attention_pool_packed(x, w, gamma, beta, a, starts, lengths,
                                   E: int, p: float, training: bool,
                                   offsets=None):
    """CombinerAttentionPoolPacked behind the host check of the lengths
    (EP = 128).  Returns (cv f32 [B, EP], attn f32 [M], cvb bf16)."""
    M = x.shape[0]
    _, offsets = packed_offsets(lengths, M, x.device, offsets)
    if w.shape[0] != 128:
        raise ValueError(
            f"combiner_attention_pool_packed: EP must be 128, got "
            f"{w.shape[0]}")
    _check_packed_pool_args("combiner_attention_pool_packed", M, 128, starts)
    return CombinerAttentionPoolPacked.apply(
        x, w, gamma, beta, a, starts.reshape(-1).contiguous(), offsets,
        int(E), float(p), bool(training))


class CombinerAttentionPool(torch.autograd.Function):
    """K3-K9 as one autograd node (EP = 128): combiner_fwd, then
    attention_fwd, returning cv (f32), attn and cv rounded to bf16 (what
    the output head consumes; the kernel emits it, so no cast kernel runs).

    Backward never materializes dccv [B*C, EP], the attention pool's
    gradient w.r.t. the combiner output: the compact attention_bwd writes
    only ds [B*C] (plus the da partials) and the recomputing combiner_bwd
    rebuilds each element bf16(attn*dcv + ds*a) in registers, through the
    same device function the dense kernel uses, so every result has the
    bits of the CombinerLNTanh -> AttentionPool -> .to(bf16) chain.  The
    bf16 gradient of the bf16 cv output is read by the kernels directly;
    a gradient on the f32 cv output, if there is one as well, is added
    first.

    At C <= 200 both attention kernels are the streaming forms (see
    _ATTN_STREAM above): combiner_fwd's flush emits the raw scores, the
    forward and the compact backward keep a method's rows in registers.
    Longer bags, or a switch at 0, take the tiled kernels; same bits."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, a, starts, E: int, p: float,
                training: bool):
        B, C = starts.shape
        M = x.shape[0]
        EP = w.shape[0]
        assert EP == 128 and M == B * C
        starts = starts.contiguous()
        dev = x.device
        out = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        z = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        mean = torch.empty(M, dtype=torch.float32, device=dev)
        rstd = torch.empty(M, dtype=torch.float32, device=dev)
        p_eff = float(p) if training else 0.0
        seed, off_t = (_philox_state(dev) if p_eff > 0.0
                       else (0, _philox_state(dev)[1]))
        cv = torch.empty(B, EP, dtype=torch.float32, device=dev)
        cvb = torch.empty(B, EP, dtype=torch.bfloat16, device=dev)
        attn = torch.empty(B, C, dtype=torch.float32, device=dev)
        stream_ok = ext().attention_stream_ok(C, EP)
        have_scores = False
        if _ATTN_STREAM_FWD and stream_ok and _FWD_EPI == 1:
            raw = torch.empty(M, dtype=torch.float32, device=dev)
            # False (raw untouched) if the combiner took a kernel without
            # the score flush; a host-side decision, no sync
            have_scores = ext().combiner_fwd_scores(
                x, w, gamma, beta, a, out, z, mean, rstd, raw, E, p_eff,
                seed, off_t, _FWD_EPI)
        else:
            ext().combiner_fwd(x, w, gamma, beta, out, z, mean, rstd, E,
                               p_eff, seed, off_t, _FWD_EPI)
        if have_scores:
            ext().attention_fwd_scores(out.view(B, C, EP), raw, starts, cv,
                                       cvb, attn, E)
        else:
            ext().attention_fwd_cvb(out.view(B, C, EP), a, starts, cv, cvb,
                                    attn, E)
        ctx.save_for_backward(x, w, gamma, beta, a, starts, z, mean, rstd,
                              out, attn)
        ctx.meta = (E, p_eff)
        ctx.set_materialize_grads(False)
        return cv, attn, cvb

    @staticmethod
    def backward(ctx, dcv32, dattn, dcvb):
        (x, w, gamma, beta, a, starts, z, mean, rstd, out,
         attn) = ctx.saved_tensors
        E, p = ctx.meta
        B, C = starts.shape
        M, EP = z.shape
        dev = z.device
        if dcv32 is not None and dcvb is not None:
            dcv = dcv32 + dcvb  # f32 sum, as autograd's accumulation did
        elif dcvb is not None:
            dcv = dcvb          # bf16, read by the kernels as is
        elif dcv32 is not None:
            dcv = dcv32
        else:
            dcv = torch.zeros(B, EP, dtype=torch.float32, device=dev)
        dcv = dcv.contiguous()
        ds = torch.empty(M, dtype=torch.float32, device=dev)
        da_p = torch.empty(B, EP, dtype=torch.float32, device=dev)
        has_dattn = dattn is not None
        dattn = dattn.contiguous() if has_dattn else _NONE_T
        if _ATTN_STREAM_BWD and ext().attention_stream_ok(C, EP):
            ext().attention_bwd_compact_reg(dcv, dattn, out.view(B, C, EP),
                                            starts, attn, ds, da_p, E,
                                            has_dattn)
        else:
            ext().attention_bwd_compact(dcv, dattn, out.view(B, C, EP), a,
                                        starts, attn, ds, da_p, E, has_dattn)
        da = _slab_sum(da_p)
        dz = torch.empty(M, EP, dtype=torch.bfloat16, device=dev)
        nblocks = min((M + 4 - 1) // 4, 1024)
        dgamma_p = torch.empty(nblocks, EP, dtype=torch.float32, device=dev)
        dbeta_p = torch.empty(nblocks, EP, dtype=torch.float32, device=dev)
        ext().combiner_bwd_recompute(attn.view(-1), ds, dcv, a, C, z, out,
                                     mean, rstd, gamma, beta, dz, dgamma_p,
                                     dbeta_p, E, p)
        dgamma, dbeta = _slab_sum_pair(dgamma_p, dbeta_p)
        dx, dw = _combiner_dx_dw(x, w, dz)
        return dx, dw, dgamma, dbeta, da, None, None, None, None


def combiner_attention_pool_supported(x, w) -> bool:
    """Gates for CombinerAttentionPool: device tensors, EP = 128, grad
    mode on (eval/export/predict keep the separate Functions)."""
    return (FUSED_CAP and x.is_cuda and w.shape[0] == 128
            and torch.is_grad_enabled() and x.shape[0] < (1 << 31))


class OutputHead(torch.autograd.Function):
    """K10: label projection logits = cv @ W^T + b with a custom backward:
    dW/dcv via rocBLAS, dbias via the colsum kernel (torch's reduce is ~4x
    off HBM bandwidth on [B, 30k+] bf16)."""

    @staticmethod
    def forward(ctx, cv_bf16, w, bias):
        B, EP = cv_bf16.shape
        L = w.shape[0]
        if (_HEAD_FWD and cv_bf16.is_cuda and EP % 32 == 0
                and L <= _HEAD_FWD_MAXL):
            # custom MFMA forward: both fragments are contiguous in memory
            # (K = EP is the fast axis of both cv and w), so this streams at
            # the C-write bound where hipBLASLt runs a K=128 GEMM pipeline.
            # When grads are on (training), the epilogue also emits the
            # per-row online-softmax partials the NLL loss consumes, saving
            # the loss kernel's full re-read of logits.
            logits = torch.empty(B, L, dtype=torch.bfloat16,
                                 device=cv_bf16.device)
            if cv_bf16.requires_grad or w.requires_grad:
                gx = (L + 255) // 256  # one partial per 256-label block
                pm = torch.empty(gx, B, dtype=torch.float32, device=w.device)
                ps = torch.empty_like(pm)
            else:
                pm = ps = _NONE_T
            ext().head_fwd(cv_bf16, w, bias.float(), logits, pm, ps)
            if pm is not _NONE_T:
                logits._c2v_lsm_partials = (pm, ps)
        else:
            logits = torch.nn.functional.linear(
                cv_bf16, w, bias.to(torch.bfloat16))
        ctx.save_for_backward(cv_bf16, w)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        cv, w = ctx.saved_tensors
        dlogits = dlogits.contiguous()
        B, L = dlogits.shape
        EP = cv.shape[1]
        if (_HEAD_DGRAD and EP == 128 and L % 8 == 0 and dlogits.is_cuda
                and L <= _HEAD_FWD_MAXL):  # big L: slab traffic dominates
            # split-K MFMA dcv (head_dgrad.hip): hipBLASLt runs this
            # skinny-output huge-K GEMM ~6x off the traffic floor.  W is
            # transposed once so both fragments are contiguous loads.
            wt = _scratch_bf16("head_wt", (128, L), w.device)
            ext().transpose_w(w, wt)
            split = (L + 511) // 512
            partials = _scratch_f32("head_dgrad", (split, B, 128), w.device)
            ext().head_dgrad(dlogits, wt, partials)
            dcv = torch.empty(B, 128, dtype=torch.bfloat16,
                              device=w.device)
            ext().slab_sum_bf16(partials, dcv)
        else:
            dcv = dlogits @ w                  # [B, EP] bf16 (rocBLAS)
        # default OFF: measured slower than TunableOp rocBLAS at the
        # top11 shape (single-buffered staging; see PERF.md)
        if (os.environ.get("C2V_HEAD_WGRAD", "0") == "1"
                and B % 32 == 0 and L % 8 == 0 and EP % 32 == 0
                and EP <= 128):
            dw = torch.empty(L, EP, dtype=torch.bfloat16, device=w.device)
            ext().head_wgrad(dlogits, cv, dw)
        else:
            dw = dlogits.t() @ cv              # [L, EP] bf16 (rocBLAS)
        dbias = torch.zeros(w.shape[0], dtype=torch.float32,
                            device=w.device)
        ext().colsum_bf16(dlogits, dbias)
        return dcv, dw, dbias


def _acc_reduce(acc_part):
    """Deterministic (fixed-order) reduction of per-block loss partials
    [S, 2] -> (acc[2] = (sum w_y*nll, sum w_y), loss = acc[0] / acc[1]).
    The previous atomic-add accumulation was ordering-nondeterministic at
    the fp32 ulp level and made identical runs diverge after two steps of
    bf16 rounding.  One kernel writes acc and the quotient (same column
    tree as slab_sum_f32, correctly rounded division) with
    C2V_LOSS_REDUCE=1; the default is slab_sum_f32 + the torch
    select/divide."""
    acc = torch.empty(2, dtype=torch.float32, device=acc_part.device)
    if _LOSS_REDUCE:
        loss = torch.empty((), dtype=torch.float32, device=acc_part.device)
        ext().loss_reduce(acc_part, acc, loss)
        return acc, loss
    ext().slab_sum_f32(acc_part, acc)
    return acc, acc[0] / acc[1]


def _finalize_stats(logits, pm, ps, label, weight, lse):
    B = logits.shape[0]
    acc_p = torch.empty((B + 15) // 16, 2, dtype=torch.float32,
                        device=logits.device)
    ext().logsoftmax_nll_finalize(logits, pm, ps, label, weight, lse, acc_p)
    return _acc_reduce(acc_p)


def _lsm_stats(logits, label, weight, lse):
    """Fill lse and return (acc, loss) from a full pass over logits.  Large L
    takes the 2-D-grid partials kernel + finalize (the one-block-per-row
    walk is latency-bound at ~3.6 TB/s at L = 261k: 150 -> ~75 us)."""
    B, L = logits.shape
    if L >= 32768:
        gx = (L + 16383) // 16384
        pm = torch.empty(gx, B, dtype=torch.float32, device=logits.device)
        ps = torch.empty_like(pm)
        ext().lsm_partial(logits, pm, ps)
        return _finalize_stats(logits, pm, ps, label, weight, lse)
    acc_p = torch.empty(B, 2, dtype=torch.float32, device=logits.device)
    ext().logsoftmax_nll_fwd(logits, label, weight, lse, acc_p)
    return _acc_reduce(acc_p)


class FusedLogSoftmaxNLL(torch.autograd.Function):
    """K12: full-vocab log-softmax + weighted NLL, fused fwd and bwd.

    logits: bf16 [B, L]; label: i64 [B]; weight: f32 [L] (1/freq weights,
    reference main.py:129-130) or None for w = 1.
    loss = sum(w_y*(lse - logit_y)) / sum(w_y).
    """

    @staticmethod
    def forward(ctx, logits, label, weight):
        B, L = logits.shape
        if weight is None:  # unweighted: the kernels take w_y = 1
            weight = _NONE_T
        lse = torch.empty(B, dtype=torch.float32, device=logits.device)
        # acc[0] = sum(w_y * nll), acc[1] = sum(w_y)
        partials = getattr(logits, "_c2v_lsm_partials", None)
        if partials is not None:
            # the head-forward epilogue already reduced per-row (max, sum)
            # partials over the logits — merge them instead of re-reading
            # the whole [B, L] matrix
            pm, ps = partials
            del logits._c2v_lsm_partials
            acc, loss = _finalize_stats(logits, pm, ps, label, weight, lse)
        else:
            acc, loss = _lsm_stats(logits, label, weight, lse)
        ctx.save_for_backward(logits, label, weight, lse, acc)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, label, weight, lse, acc = ctx.saved_tensors
        dlogits = torch.empty_like(logits)
        ext().logsoftmax_nll_bwd(
            logits, label, weight, lse, acc, dloss.contiguous().float(), dlogits
        )
        return dlogits, None, None


class AngularMarginHead(torch.autograd.Function):
    """K11: ArcFace-style head fully on HIP kernels (angular.hip).

    Forward: per-row inverse norms -> unit matrices -> MFMA cosine GEMM
    with the margin epilogue (emits scaled outputs AND the raw cosine for
    backward).  Backward: dcos elementwise kernel; du = dcos @ U_w via the
    split-K head_dgrad kernel; dv = dcos^T @ U_cv via head_wgrad; both
    projected through the normalize backward (norm_project kernel).
    Reference math: model/model.py:71-80 (th/mm computed-but-unused there).
    EP = 128 only; callers gate and fall back to ops/reference.py.
    """

    @staticmethod
    def forward(ctx, cv_bf16, w, label, cos_m, sin_m, s):
        B = cv_bf16.shape[0]
        L = w.shape[0]
        dev = w.device
        inv_c = torch.empty(B, dtype=torch.float32, device=dev)
        inv_w = torch.empty(L, dtype=torch.float32, device=dev)
        ext().inv_rownorm(cv_bf16, inv_c)
        ext().inv_rownorm(w, inv_w)
        ucv = torch.empty_like(cv_bf16)
        uw = _scratch_bf16("ang_uw", (L, 128), dev)
        ext().rowscale(cv_bf16, inv_c, ucv)
        ext().rowscale(w, inv_w, uw)
        out = torch.empty(B, L, dtype=torch.bfloat16, device=dev)
        cos = torch.empty(B, L, dtype=torch.bfloat16, device=dev)
        ext().angular_fwd(ucv, uw, label, out, cos, cos_m, sin_m, s)
        ctx.save_for_backward(ucv, uw, inv_c, inv_w, cos, label)
        ctx.consts = (cos_m, sin_m, s)
        return out

    @staticmethod
    def backward(ctx, dout):
        ucv, uw, inv_c, inv_w, cos, label = ctx.saved_tensors
        cos_m, sin_m, s = ctx.consts
        B, L = cos.shape
        dev = cos.device
        dcos = torch.empty_like(cos)
        ext().angular_dcos(dout.contiguous().to(torch.bfloat16), cos, label,
                           dcos, cos_m, sin_m, s)
        # du = dcos @ U_w  (split-K head_dgrad; rocBLAS fallback off-shape)
        if L % 8 == 0:
            uwt = _scratch_bf16("ang_uwt", (128, L), dev)
            ext().transpose_w(uw, uwt)
            split = (L + 511) // 512
            partials = _scratch_f32("ang_dcv", (split, B, 128), dev)
            ext().head_dgrad(dcos, uwt, partials)
            du = torch.empty(B, 128, dtype=torch.bfloat16, device=dev)
            ext().slab_sum_bf16(partials, du)
        else:
            du = dcos @ uw
        # dv = dcos^T @ U_cv  (head_wgrad; rocBLAS fallback off-shape)
        dv = torch.empty(L, 128, dtype=torch.bfloat16, device=dev)
        if B % 32 == 0 and L % 8 == 0:
            ext().head_wgrad(dcos, ucv, dv)
        else:
            dv.copy_(dcos.t() @ ucv)
        dcv = torch.empty_like(du)
        dw = torch.empty_like(dv)
        ext().norm_project(du, ucv, inv_c, dcv)
        ext().norm_project(dv, uw, inv_w, dw)
        return dcv, dw, None, None, None, None


def angular_margin_head_hip(cv_bf16, w, label, cos_m, sin_m, s):
    """Gated entry: HIP kernels when the shape fits, torch reference
    otherwise (CPU, EP != 128)."""
    from . import reference as R

    if cv_bf16.is_cuda and cv_bf16.shape[1] == 128 and w.shape[1] == 128:
        return AngularMarginHead.apply(cv_bf16, w, label, cos_m, sin_m, s)
    return R.angular_margin_head(cv_bf16, w, label, cos_m, sin_m, s)


def head_logits_with_stats(cv_bf16, w, bias):
    """Forward logits for the FUSED head+loss path (no autograd tracking —
    gradients flow through FusedHeadLoss instead).  Uses the custom MFMA
    head_fwd (+ online-softmax stats epilogue) when gated on, else the
    hipBLASLt linear; either way the result carries what the fused loss
    needs stashed as tensor attributes."""
    B, EP = cv_bf16.shape
    L = w.shape[0]
    with torch.no_grad():
        if _HEAD_FWD and _HF_AIMG and EP == 128 and L % 8 == 0:
            # W pre-swizzled into the A-fragment image so the kernel's W
            # reads are contiguous 1-KB wave reads.  Originally the
            # large-L fix (strided per-lane row loads streamed W from
            # HBM inefficiently at L=261k), but measured faster than the
            # direct-load kernel at top11 scale too (63.7 vs 79.4 us at
            # L=72,416; step 1.337 vs 1.350 ms) — the swizzle cost
            # (~7 us, L2-resident) is well under the fragment-read win.
            wimg = _scratch_bf16("hf_aimg",
                                 ((L + 255) // 256 * 16, 4, 64, 8),
                                 w.device)
            ext().swizzle_a(w, wimg)
            logits = torch.empty(B, L, dtype=torch.bfloat16,
                                 device=cv_bf16.device)
            gx = (L + 255) // 256
            pm = torch.empty(gx, B, dtype=torch.float32, device=w.device)
            ps = torch.empty_like(pm)
            ext().head_fwd_img(cv_bf16, wimg, bias.float(), logits, pm, ps,
                               L)
            logits._c2v_lsm_partials = (pm, ps)
            logits._c2v_wimg_a = wimg  # reusable by the streaming backward
        elif _HEAD_FWD and EP % 32 == 0 and L <= _HEAD_FWD_MAXL:
            # direct-load kernel: the EP != 128 path (C2V_HF_AIMG=0 also
            # lands here below C2V_HEAD_FWD_MAXL)
            logits = torch.empty(B, L, dtype=torch.bfloat16,
                                 device=cv_bf16.device)
            gx = (L + 255) // 256
            pm = torch.empty(gx, B, dtype=torch.float32, device=w.device)
            ps = torch.empty_like(pm)
            ext().head_fwd(cv_bf16, w, bias.float(), logits, pm, ps)
            logits._c2v_lsm_partials = (pm, ps)
        else:
            logits = torch.nn.functional.linear(
                cv_bf16, w, bias.to(torch.bfloat16))
    return logits


class FusedHeadLoss(torch.autograd.Function):
    """K10+K12 collapsed into one autograd node (recompute-G backward).

    Forward: merges the head epilogue's online-softmax partials into
    (lse, acc) — the [B, L] logits are never re-read in full when the
    custom head forward ran.  Backward: dW/dbias (head_bwd_dw) and dcv
    (head_bwd_dcv) recompute G[b,l] = coef_b*(exp(logit-lse_b) - [l==y_b])
    from logits+lse in registers; the dlogits tensor of the unfused chain
    (a 61 MB write + 3x 61 MB reads at top11, 534 MB x4 at java-large) is
    never materialized.  Reference math: main.py:251-264 composed with
    model/model.py:83.

    ``logits`` is a NON-differentiable input (computed under no_grad by
    head_logits_with_stats); gradients flow to cv/w/bias directly.
    """

    @staticmethod
    def forward(ctx, logits, cv_bf16, w, bias, label, weight):
        B, L = logits.shape
        if weight is None:  # unweighted: the kernels take w_y = 1
            weight = _NONE_T
        lse = torch.empty(B, dtype=torch.float32, device=logits.device)
        partials = getattr(logits, "_c2v_lsm_partials", None)
        if partials is not None:
            pm, ps = partials
            del logits._c2v_lsm_partials
            acc, loss = _finalize_stats(logits, pm, ps, label, weight, lse)
        else:
            acc, loss = _lsm_stats(logits, label, weight, lse)
        ctx.save_for_backward(logits, cv_bf16, w, label, weight, lse, acc,
                              bias)
        # saved_tensors re-wraps the tensor object, so python attributes
        # do not survive — carry the forward's W fragment image on ctx
        ctx.wimg_a = getattr(logits, "_c2v_wimg_a", None)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, cv, w, label, weight, lse, acc, bias = ctx.saved_tensors
        B, L = logits.shape
        dev = w.device
        g = dloss.contiguous().float().view(1)
        # per-row (coef, lse, y) packed once: ONE 16-B load per staged
        # logits chunk in the kernels below
        coef_lse = _scratch_f32("head_coef_lse", (B, 4), dev)
        ext().head_bwd_prep(label, weight, acc, g, lse, coef_lse)
        # dW + dbias (label-major): cv pre-swizzled once (256 KB) into the
        # MFMA fragment-image layout so every B-fragment read in the dW
        # kernel is a contiguous 1-KB wave read from L2
        nchunk = (B + 63) // 64 * 2
        cvimg = _scratch_bf16("head_cvimg", (nchunk, 8, 64, 8), dev)
        ext().swizzle_cv(cv.contiguous(), cvimg)
        dw = torch.empty(L, 128, dtype=torch.bfloat16, device=dev)
        dbias = torch.empty(L, dtype=torch.float32, device=dev)
        if _HB_PIPE_DW:
            ext().head_bwd_dw_pipe(logits, cvimg, coef_lse, dw, dbias, 0)
        else:
            ext().head_bwd_dw(logits, cvimg, coef_lse, dw, dbias)
        # dcv (batch-major split-K): label chunk balances split-K slab
        # traffic against grid width (A/B-swept: 1024 beats 512 by ~30
        # us/step at top11; 4096 at java-large keeps slabs ~33 MB).  W is
        # pre-swizzled into the B-fragment image the kernel stages from
        # (one contiguous 32-KB LDS copy per sub-stage; replaces the
        # transpose_w kernel + line-amplified transposed-W staging).
        chunk = int(os.environ.get("C2V_HB_DCV_CHUNK", "0")) or (
            1024 if L <= 131072 else 4096)
        split = (L + chunk - 1) // chunk
        wimg = _scratch_bf16("head_wimg", ((L + 127) // 128 * 4, 8, 64, 8),
                             dev)
        ext().swizzle_cv(w, wimg)
        partials = _scratch_f32("head_fused_dcv", (split, B, 128), dev)
        if _HB_RC:
            # STREAMING dcv: the [B, L] logits are never read — each wave
            # recomputes its logits tile by MFMA from the swizzle_a
            # fragment images of cv and W (the W image is reused from the
            # forward when head_fwd_img ran) and adds the f32 bias
            cvimg_a = _scratch_bf16(
                "head_cvimg_a", ((B + 255) // 256 * 16, 4, 64, 8), dev)
            ext().swizzle_a(cv.contiguous(), cvimg_a)
            wimg_a = ctx.wimg_a
            if wimg_a is None:
                wimg_a = _scratch_bf16(
                    "hf_aimg", ((L + 255) // 256 * 16, 4, 64, 8), dev)
                ext().swizzle_a(w, wimg_a)
            ext().head_bwd_dcv_rc(cvimg_a, wimg_a, wimg,
                                  bias.detach().float().contiguous(),
                                  coef_lse, partials, B, L, chunk)
        elif _HB_PIPE_DCV:
            ext().head_bwd_dcv_pipe(logits, wimg, coef_lse, partials, chunk,
                                    -1)
        else:
            ext().head_bwd_dcv(logits, wimg, coef_lse, partials, chunk)
        dcv = torch.empty(B, 128, dtype=torch.bfloat16, device=dev)
        ext().slab_sum_bf16(partials, dcv)
        return None, dcv, dw, dbias, None, None


def fused_head_loss_supported(cv_bf16, w, training: bool) -> bool:
    """Shape/mode gates for the fused head+loss path."""
    B, EP = cv_bf16.shape
    L = w.shape[0]
    return (FUSED_HEAD and training and torch.is_grad_enabled()
            and cv_bf16.is_cuda and EP == 128 and L % 8 == 0 and B % 8 == 0
            and L < (1 << 24))  # y carried as f32 in the G recompute


def row_max_argmax(logits: torch.Tensor):
    """K17: per-row (max, argmax) for the eval/export prediction path —
    the last eval op that went through a torch kernel.  Falls back to
    torch.max off the HIP bf16 path."""
    if logits.is_cuda and logits.dtype == torch.bfloat16 \
            and logits.is_contiguous():
        B = logits.shape[0]
        vals = torch.empty(B, dtype=torch.float32, device=logits.device)
        idx = torch.empty(B, dtype=torch.int64, device=logits.device)
        ext().row_max_argmax(logits, vals, idx)
        return vals, idx
    return torch.max(logits.float(), dim=1)


# chunk width of the K19 stage-1 grid (columns per block); the extension
# checks it against the compiled value.  Exposed so tests can plant values
# on chunk boundaries.
ROW_TOPK_CHUNK = 32768
_ROW_TOPK_SLOTS = 16  # candidates each chunk hands to stage 2


def row_topk(x: torch.Tensor, k: int):
    """K19: per-row top-k (1 <= k <= 16) + log-sum-exp in one pass.

    Returns (vals f32 [B, k], idx i64 [B, k], lse f32 [B]) in the total
    order of ops/reference.py::row_topk (descending value, ties to the
    smallest column).  Device bf16/f32 input runs the HIP kernel (no host
    sync; capturable); CPU tensors and other dtypes take the reference.
    A non-contiguous device tensor is an error rather than a silent copy
    or an eager fallback."""
    from . import reference as R

    k = int(k)
    R.check_row_topk_args(x, k)
    if not (x.is_cuda and x.dtype in (torch.bfloat16, torch.float32)):
        return R.row_topk(x, k)
    if not x.is_contiguous():
        raise ValueError("row_topk: device input must be contiguous")
    B, L = x.shape
    dev = x.device
    vals = torch.empty(B, k, dtype=torch.float32, device=dev)
    idx = torch.empty(B, k, dtype=torch.int64, device=dev)
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    nchunk = (L + ROW_TOPK_CHUNK - 1) // ROW_TOPK_CHUNK
    if nchunk > 1:
        part = torch.empty(B, nchunk, _ROW_TOPK_SLOTS, dtype=torch.int64,
                           device=dev)
        pm = torch.empty(B, nchunk, dtype=torch.float32, device=dev)
        ps = torch.empty_like(pm)
    else:
        part = pm = ps = _NONE_T
    ext().row_topk(x, k, ROW_TOPK_CHUNK, part, pm, ps, vals, idx, lse)
    return vals, idx, lse


def topk_probs(vals: torch.Tensor, lse: torch.Tensor) -> torch.Tensor:
    """Softmax probabilities of row_topk's selected entries."""
    return torch.exp(vals - lse[:, None])


# K20 tiles: queries per block (the index is streamed once per query tile)
# and index rows per MFMA tile (slice boundaries fall on multiples of it).
# The extension checks both against the compiled values.
SIM_QUERY_TILE = 16
SIM_ROW_TILE = 16
# stage-1 blocks the default nsplit aims for (a few per CU of a 256-CU
# device; results do not depend on nsplit, so this is a constant)
_SIM_TARGET_BLOCKS = 1024
# tiles a slice should at least hold: every block fills its lists from
# empty, which threshold-first selection only repays on a long stream
# (PERF.md, "Similarity search": the nsplit sweep)
_SIM_MIN_SLICE_TILES = 128
# C2V_SIM_FUSED=0 routes sim_topk to sim_topk_composed (A/B baseline)
_SIM_FUSED = os.environ.get("C2V_SIM_FUSED", "1") == "1"
_SIM_COMPOSED_SCORE_BYTES = 1 << 30


def sim_topk_default_nsplit(nq: int, N: int) -> int:
    """Index slices K20 uses when the caller does not force a number."""
    nqt = max(1, -(-nq // SIM_QUERY_TILE))
    ntile = -(-N // SIM_ROW_TILE)
    return max(1, min(-(-_SIM_TARGET_BLOCKS // nqt),
                      ntile // _SIM_MIN_SLICE_TILES))


def sim_topk_slice_rows(N: int, nsplit: int) -> int:
    """Index rows per slice for a given nsplit (slice s owns rows
    [s * rows, (s + 1) * rows)); exposed so tests can plant values on
    slice boundaries."""
    ntile = -(-N // SIM_ROW_TILE)
    return -(-ntile // nsplit) * SIM_ROW_TILE


def _sim_topk_check_device(q, db):
    if q.dtype != torch.bfloat16 or db.dtype != torch.bfloat16:
        raise ValueError(
            f"sim_topk: device inputs must be bf16, got {q.dtype} and "
            f"{db.dtype}")
    if q.device != db.device:
        raise ValueError("sim_topk: q and db must be on the same device")
    if not (q.is_contiguous() and db.is_contiguous()):
        raise ValueError("sim_topk: device inputs must be contiguous")


def sim_topk(q: torch.Tensor, db: torch.Tensor, k: int, exclude=None,
             nsplit: Optional[int] = None):
    """K20: per query row of q [nq, EP], the k (1..16) rows of db [N, EP]
    with the largest dot product, without materializing the [nq, N] score
    matrix.  Returns (vals f32 [nq, k], idx i64 [nq, k]) in row_topk's
    total order (descending score, ties to the smallest index row).
    ``exclude`` [nq] i64: one index row per query that is never returned
    (-1: none).  Device bf16 input runs the HIP kernel (no host sync;
    capturable); CPU tensors take ops/reference.py::sim_topk.  ``nsplit``
    forces the number of index slices (results do not depend on it)."""
    from . import reference as R

    k = int(k)
    R.check_sim_topk_args(q, db, k, exclude)
    if not (q.is_cuda or db.is_cuda):
        return R.sim_topk(q, db, k, exclude)
    _sim_topk_check_device(q, db)
    if not _SIM_FUSED:
        return sim_topk_composed(q, db, k, exclude)
    nq, N = q.shape[0], db.shape[0]
    dev = q.device
    if exclude is not None:
        if exclude.device != dev or not exclude.is_contiguous():
            raise ValueError(
                "sim_topk: exclude must be contiguous on the inputs' device")
    if nsplit is None:
        nsplit = sim_topk_default_nsplit(nq, N)
    nsplit = int(nsplit)
    if nsplit < 1:
        raise ValueError(f"sim_topk: nsplit must be >= 1, got {nsplit}")
    vals = torch.empty(nq, k, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, k, dtype=torch.int64, device=dev)
    if nq == 0:
        return vals, idx
    part = (torch.empty(nq, nsplit, 16, dtype=torch.int64, device=dev)
            if nsplit > 1 else _NONE_T)
    ext().sim_topk(q, db, exclude if exclude is not None else _NONE_T, k,
                   nsplit, SIM_QUERY_TILE, SIM_ROW_TILE, part, vals, idx)
    return vals, idx


def sim_topk_composed(q: torch.Tensor, db: torch.Tensor, k: int,
                      exclude=None):
    """sim_topk's contract through existing parts: an fp32 matmul per
    query chunk (chunks sized so the scores stay under about 1 GiB), then
    row_topk (K19).  The A/B baseline of the fused kernel; scores differ
    from K20's only by fp32 summation order."""
    from . import reference as R

    k = int(k)
    R.check_sim_topk_args(q, db, k, exclude)
    if q.is_cuda or db.is_cuda:
        _sim_topk_check_device(q, db)
    nq, N = q.shape[0], db.shape[0]
    dev = q.device
    vals = torch.empty(nq, k, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, k, dtype=torch.int64, device=dev)
    dbt = db.float().t()
    step = max(1, _SIM_COMPOSED_SCORE_BYTES // (4 * N))
    for a in range(0, nq, step):
        b = min(nq, a + step)
        S = q[a:b].float() @ dbt
        if exclude is not None:
            ex = exclude[a:b].to(dev)
            # no host sync: excluded entries via a one-column scatter whose
            # "none" rows (-1) rewrite column 0 with its own value
            col = ex.clamp(0, N - 1).view(-1, 1)
            cur = S.gather(1, col)
            hit = ((ex >= 0) & (ex < N)).view(-1, 1)
            S.scatter_(1, col, torch.where(
                hit, torch.full_like(cur, float("-inf")), cur))
        v, i, _ = row_topk(S, k)
        vals[a:b] = v
        idx[a:b] = i
    return vals, idx


# K24 runs on K20's tiles; the waves of a block split their slice into
# contiguous runs (the extension checks the number against the compiled one).
SIM_RANGE_WAVES = 4
# blocks the default nsplit aims for per pass: one per CU of a 256-CU
# device.  K24 has no lists to merge, so longer runs per wave cost nothing
# (PERF.md, "K24 similarity range search": the nsplit sweep)
_SIM_RANGE_TARGET_BLOCKS = 256
# tiles a slice should at least hold (16 per wave): below that the query
# fragments and the pipeline prologue are loaded for a handful of MFMAs
_SIM_RANGE_MIN_SLICE_TILES = 64
SIM_RANGE_MAX_PAIRS = 1 << 24


def sim_range_default_nsplit(nq: int, N: int) -> int:
    """Index slices K24 uses when the caller does not force a number."""
    nqt = max(1, -(-nq // SIM_QUERY_TILE))
    ntile = -(-N // SIM_ROW_TILE)
    return max(1, min(-(-_SIM_RANGE_TARGET_BLOCKS // nqt),
                      ntile // _SIM_RANGE_MIN_SLICE_TILES))


def sim_range_slice_rows(N: int, nsplit: int) -> int:
    """Index rows per slice for a given nsplit (slice s owns rows
    [s * rows, (s + 1) * rows)); exposed so tests can plant rows on slice
    boundaries."""
    return sim_topk_slice_rows(N, nsplit)


def sim_range_wave_rows(N: int, nsplit: int) -> int:
    """Index rows per wave within a slice: wave w of slice s owns rows
    [s * slice_rows + w * wave_rows, ... + wave_rows), cut at the slice's
    end; exposed so tests can plant rows on wave boundaries."""
    tiles = sim_topk_slice_rows(N, nsplit) // SIM_ROW_TILE
    return -(-tiles // SIM_RANGE_WAVES) * SIM_ROW_TILE


def _sim_range_check_device(q, db, exclude, after):
    if q.dtype != torch.bfloat16 or db.dtype != torch.bfloat16:
        raise ValueError(
            f"sim_range: device inputs must be bf16, got {q.dtype} and "
            f"{db.dtype}")
    if q.device != db.device:
        raise ValueError("sim_range: q and db must be on the same device")
    if not (q.is_contiguous() and db.is_contiguous()):
        raise ValueError("sim_range: device inputs must be contiguous")
    for name, t in (("exclude", exclude), ("after", after)):
        if t is not None and (t.device != q.device
                              or not t.is_contiguous()):
            raise ValueError(
                f"sim_range: {name} must be contiguous on the inputs' "
                f"device")


def sim_range_count(q, db, threshold, exclude=None, after=None,
                    nsplit: Optional[int] = None):
    """K24's count pass on checked device inputs: (cur i64 [nq * nsplit *
    4 + 1], nsplit) — the exclusive write cursors of every (query, slice,
    wave), the total last.  No host sync."""
    nq, N = q.shape[0], db.shape[0]
    if nsplit is None:
        nsplit = sim_range_default_nsplit(nq, N)
    nsplit = int(nsplit)
    if nsplit < 1:
        raise ValueError(f"sim_range: nsplit must be >= 1, got {nsplit}")
    counts = torch.empty(nq, nsplit, SIM_RANGE_WAVES, dtype=torch.int32,
                         device=q.device)
    ext().sim_range_count(q, db, exclude if exclude is not None else _NONE_T,
                          after if after is not None else _NONE_T,
                          threshold, nsplit, SIM_QUERY_TILE, SIM_ROW_TILE,
                          SIM_RANGE_WAVES, counts)
    cur = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=q.device)
    cur[1:] = torch.cumsum(counts.view(-1), 0, dtype=torch.int64)
    return cur, nsplit


def sim_range_fill(q, db, threshold, cur, nsplit: int, total: int,
                   exclude=None, after=None):
    """K24's fill pass: (offsets, rows, scores) from sim_range_count's
    cursors and their total (cur[-1], read back by the caller)."""
    nq = q.shape[0]
    dev = q.device
    offsets = cur[::nsplit * SIM_RANGE_WAVES].contiguous()
    rows = torch.empty(total, dtype=torch.int64, device=dev)
    scores = torch.empty(total, dtype=torch.float32, device=dev)
    if total:
        ext().sim_range_fill(
            q, db, exclude if exclude is not None else _NONE_T,
            after if after is not None else _NONE_T, threshold, nsplit,
            SIM_QUERY_TILE, SIM_ROW_TILE, SIM_RANGE_WAVES, cur, rows, scores)
    assert offsets.shape[0] == nq + 1
    return offsets, rows, scores


def sim_range(q: torch.Tensor, db: torch.Tensor, threshold: float,
              exclude=None, after=None,
              max_pairs: int = SIM_RANGE_MAX_PAIRS,
              nsplit: Optional[int] = None):
    """K24: per query row of q [nq, EP], EVERY row of db [N, EP] whose dot
    product is at least fp32(threshold), without materializing the [nq, N]
    score matrix.  Returns a CSR (offsets i64 [nq + 1], rows i64 [nnz],
    scores f32 [nnz]): query i owns rows[offsets[i]:offsets[i + 1]],
    strictly ascending; a score has the bits sim_topk gives the same pair.
    ``exclude`` [nq] i64: one index row per query that is never reported
    (-1: none).  ``after`` [nq] i64: only rows > after[i] are reported
    (-1: all), which makes a self-join emit every unordered pair once.
    More than ``max_pairs`` pairs raise a ValueError
    (reference.TooManyPairs) before any output is allocated.

    Device bf16 input runs the HIP kernel in two passes (count, fill) with
    ONE host sync between them — the total is read back to size the
    outputs, as for torch.nonzero — so the op is NOT graph-capturable.  CPU
    tensors take ops/reference.py::sim_range.  ``nsplit`` forces the number
    of index slices (results do not depend on it)."""
    from . import reference as R

    R.check_sim_range_args(q, db, threshold, exclude, after, max_pairs)
    if not (q.is_cuda or db.is_cuda):
        return R.sim_range(q, db, threshold, exclude, after, max_pairs)
    _sim_range_check_device(q, db, exclude, after)
    t32 = R.sim_range_threshold(threshold)
    nq = q.shape[0]
    dev = q.device
    if nsplit is not None and int(nsplit) < 1:
        raise ValueError(f"sim_range: nsplit must be >= 1, got {nsplit}")
    if nq == 0:
        return (torch.zeros(1, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev))
    cur, nsplit = sim_range_count(q, db, t32, exclude, after, nsplit)
    total = int(cur[-1])  # the op's one host sync
    if total > max_pairs:
        raise R.TooManyPairs(total, t32, max_pairs)
    return sim_range_fill(q, db, t32, cur, nsplit, total, exclude, after)


def sim_range_composed(q: torch.Tensor, db: torch.Tensor, threshold: float,
                       exclude=None, after=None,
                       max_pairs: int = SIM_RANGE_MAX_PAIRS):
    """sim_range's contract through existing parts: an fp32 matmul per
    query chunk (chunks sized so the scores stay under about 1 GiB), then
    >= and nonzero.  The A/B baseline of the fused kernel and a test
    reference; scores differ from K24's only by fp32 summation order.  One
    host sync per chunk."""
    from . import reference as R

    R.check_sim_range_args(q, db, threshold, exclude, after, max_pairs)
    if q.is_cuda or db.is_cuda:
        _sim_range_check_device(q, db, exclude, after)
    t32 = R.sim_range_threshold(threshold)
    nq, N = q.shape[0], db.shape[0]
    dev = q.device
    dbt = db.float().t()
    step = max(1, _SIM_COMPOSED_SCORE_BYTES // (4 * N))
    counts = torch.zeros(nq, dtype=torch.int64, device=dev)
    rows, scores = [], []
    total = 0
    for a in range(0, nq, step):
        b = min(nq, a + step)
        S = q[a:b].float() @ dbt
        mask = R.sim_range_mask(
            S, t32, None if exclude is None else exclude[a:b],
            None if after is None else after[a:b])
        counts[a:b] = mask.sum(dim=1)
        total += int(counts[a:b].sum())
        if total > max_pairs:
            raise R.TooManyPairs(total, t32, max_pairs)
        hit = torch.nonzero(mask)
        rows.append(hit[:, 1])
        scores.append(S[hit[:, 0], hit[:, 1]])
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    if not rows:
        return (offsets, torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.float32, device=dev))
    return offsets, torch.cat(rows), torch.cat(scores)


# K23 runs on K20's tiles (SIM_QUERY_TILE x SIM_ROW_TILE).  Label tiles a
# slice holds by default: fixed, so the default nsplit depends on the head's
# shape alone and a query's lse bits do not depend on the batch it is in
# (PERF.md, "K23 fused head + top-k": the slice-width sweep; 128 sits
# between the 32-64 small batches want and the 256-512 of nq = 1024).
_HEAD_TOPK_SLICE_TILES = 128
# C2V_HEAD_TOPK_FUSED=0 routes head_topk to head_topk_composed (A/B baseline)
_HEAD_TOPK_FUSED = os.environ.get("C2V_HEAD_TOPK_FUSED", "1") == "1"


def head_topk_default_nsplit(L: int, EP: int) -> int:
    """Label slices K23 uses when the caller does not force a number: a
    function of the head's shape only, never of the number of queries.
    (The measured width is EP = 128's; other widths use it as it is.)"""
    return max(1, -(-L // SIM_ROW_TILE) // _HEAD_TOPK_SLICE_TILES)


def head_topk_slice_rows(L: int, nsplit: int) -> int:
    """Labels per slice for a given nsplit (slice s owns labels
    [s * rows, (s + 1) * rows)); exposed so tests can plant values on
    slice boundaries."""
    return sim_topk_slice_rows(L, nsplit)


def _head_topk_check_device(q, w, bias):
    if q.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise ValueError(
            f"head_topk: device inputs must be bf16, got {q.dtype} and "
            f"{w.dtype}")
    if q.device != w.device or (bias is not None
                                and bias.device != q.device):
        raise ValueError(
            "head_topk: q, w and bias must be on the same device")
    if not (q.is_contiguous() and w.is_contiguous()
            and (bias is None or bias.is_contiguous())):
        raise ValueError("head_topk: device inputs must be contiguous")


def head_topk(q: torch.Tensor, w: torch.Tensor, k: int, bias=None,
              scale: float = 1.0, nsplit: Optional[int] = None):
    """K23: per query row of q [nq, EP], the k (1..16) labels with the
    largest logit scale * q . w[l] + bias[l] over w [L, EP] and the
    log-sum-exp over all L logits, without materializing the [nq, L]
    matrix.  Returns (vals f32 [nq, k], idx i64 [nq, k], lse f32 [nq]) in
    row_topk's total order.  Device bf16 input runs the HIP kernel (no host
    sync; capturable); CPU tensors take ops/reference.py::head_topk.
    ``nsplit`` forces the number of label slices: vals and idx do not
    depend on it, lse does in its last bits, which is why the default is a
    function of (L, EP) alone."""
    from . import reference as R

    k = int(k)
    scale = float(scale)
    R.check_head_topk_args(q, w, k, bias, scale)
    if not (q.is_cuda or w.is_cuda):
        return R.head_topk(q, w, k, bias, scale)
    _head_topk_check_device(q, w, bias)
    if not _HEAD_TOPK_FUSED:
        return head_topk_composed(q, w, k, bias, scale)
    if not hasattr(ext(), "head_topk"):
        # a missing kernel is an error, never a quiet change of path
        raise RuntimeError(
            "head_topk: the built extension has no K23 kernel; rebuild it "
            "(python setup.py build_ext --inplace)")
    nq, EP = q.shape
    L = w.shape[0]
    dev = q.device
    if nsplit is None:
        nsplit = head_topk_default_nsplit(L, EP)
    nsplit = int(nsplit)
    if nsplit < 1:
        raise ValueError(f"head_topk: nsplit must be >= 1, got {nsplit}")
    vals = torch.empty(nq, k, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, k, dtype=torch.int64, device=dev)
    lse = torch.empty(nq, dtype=torch.float32, device=dev)
    if nq == 0:
        return vals, idx, lse
    if nsplit > 1:
        part = torch.empty(nq, nsplit, 16, dtype=torch.int64, device=dev)
        pm = torch.empty(nq, nsplit, dtype=torch.float32, device=dev)
        ps = torch.empty_like(pm)
    else:
        part = pm = ps = _NONE_T
    ext().head_topk(q, w, bias if bias is not None else _NONE_T, scale, k,
                    nsplit, SIM_QUERY_TILE, SIM_ROW_TILE, part, pm, ps, vals,
                    idx, lse)
    return vals, idx, lse


def head_topk_composed(q: torch.Tensor, w: torch.Tensor, k: int, bias=None,
                       scale: float = 1.0, bf16_logits: bool = False):
    """head_topk's contract through existing parts, in query chunks sized so
    the logits stay under about 1 GiB: an fp32 matmul, then row_topk (K19).
    The A/B baseline of the fused kernel; logits differ from K23's only by
    fp32 summation order.  ``bf16_logits=True`` is the prediction path as it
    was before K23, for timing it: OutputHead's bf16 [chunk, L] logits, then
    K19 (default head only: a bias and scale == 1)."""
    from . import reference as R

    k = int(k)
    scale = float(scale)
    R.check_head_topk_args(q, w, k, bias, scale)
    if q.is_cuda or w.is_cuda:
        _head_topk_check_device(q, w, bias)
    if bf16_logits and (bias is None or scale != 1.0):
        raise ValueError(
            "head_topk_composed: bf16_logits is the default head's path "
            "(a bias and scale == 1)")
    nq, L = q.shape[0], w.shape[0]
    dev = q.device
    vals = torch.empty(nq, k, dtype=torch.float32, device=dev)
    idx = torch.empty(nq, k, dtype=torch.int64, device=dev)
    lse = torch.empty(nq, dtype=torch.float32, device=dev)
    wt = None if bf16_logits else w.float().t()
    step = max(1, _SIM_COMPOSED_SCORE_BYTES // ((2 if bf16_logits else 4) * L))
    for a in range(0, nq, step):
        b = min(nq, a + step)
        if bf16_logits:
            with torch.no_grad():
                z = OutputHead.apply(q[a:b], w, bias)
        else:
            z = q[a:b].float() @ wt
            if scale != 1.0:
                z *= scale
            if bias is not None:
                z += bias
        v, i, s = row_topk(z, k)
        vals[a:b] = v
        idx[a:b] = i
        lse[a:b] = s
    return vals, idx, lse


def adam_step(
    param: torch.Tensor,
    grad: torch.Tensor,
    master: Optional[torch.Tensor],
    m: torch.Tensor,
    v: torch.Tensor,
    bc_pow: torch.Tensor,
    lr: float,
    beta1: float,
    beta2: float,
    eps: float,
    weight_decay: float,
) -> None:
    """K16: fused Adam.  bf16 params carry an f32 master (updated in f32,
    rounded to bf16 param); f32 params update in place (master is None).
    ``bc_pow`` is the optimizer's device-resident (beta1^t, beta2^t)
    float64 pair (advanced by adam_tick once per step)."""
    if param.dtype == torch.bfloat16:
        assert master is not None
        ext().adam_step_bf16(
            param.view(-1), grad.view(-1), master, m, v,
            bc_pow, lr, beta1, beta2, eps, weight_decay,
        )
    else:
        ext().adam_step_f32(
            param.view(-1), grad.view(-1).float(), m, v,
            bc_pow, lr, beta1, beta2, eps, weight_decay,
        )
