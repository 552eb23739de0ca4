"""The code2vec model — torch (oracle/CPU) and HIP (MI355X) backends.

Math parity target: reference model/model.py:15-106.  Both backends are
initialized from the same logical fp32 tensors (same seeds => identical
starting points), and both return ``(outputs, code_vector, attention)``.

The HIP backend stores parameters in MI355X-native padded layouts:
- embedding tables bf16 [T, TS] / [P, PS] (TS/PS = seg_round(dt/dp):
  16-B granules — dt=100 stores as 104, keeping rows 16-B aligned for
  bf16x8 gathers without the 32-element MFMA padding waste),
- combiner weight bf16 [EP, KP] stored TRANSPOSED (so the MFMA B
  fragment is memory-contiguous; KP = round_up(2*TS+PS, 32),
  EP = round_up(E, 32)),
- output weight bf16 [L, EP]; LN/attention/bias params fp32.
Pad regions are zero and stay zero through training (padding checks in
tests/test_model_gpu.py).
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops import reference as R
from ..ops import round_up, seg_round
from ..ops import functional as Fn


def init_logical_params(option, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """Reference-equivalent initial values, in logical fp32 shapes.

    Init schemes follow reference model/model.py:18-42: embeddings N(0,1)
    (nn.Embedding default), input_linear default Linear init (no bias), LN
    ones/zeros, attention xavier_normal on [E,1] then flattened, output
    Linear default with zero bias (or xavier_uniform, no bias, for the
    angular-margin head).
    """
    g = generator
    dt, dp, E, L = (
        option.terminal_embed_size,
        option.path_embed_size,
        option.encode_size,
        option.label_count,
    )
    K = 2 * dt + dp
    p: Dict[str, torch.Tensor] = {}
    p["terminal_embedding"] = torch.randn(option.terminal_count, dt, generator=g)
    p["path_embedding"] = torch.randn(option.path_count, dp, generator=g)
    w_in = torch.empty(E, K)
    nn.init.kaiming_uniform_(w_in, a=math.sqrt(5), generator=g)
    p["input_weight"] = w_in
    p["ln_gamma"] = torch.ones(E)
    p["ln_beta"] = torch.zeros(E)
    attn = torch.zeros(E, 1)
    nn.init.xavier_normal_(attn, generator=g)
    p["attention_a"] = attn.view(-1)
    w_out = torch.empty(L, E)
    if option.angular_margin_loss:
        nn.init.xavier_uniform_(w_out, generator=g)
        p["output_weight"] = w_out
    else:
        nn.init.kaiming_uniform_(w_out, a=math.sqrt(5), generator=g)
        p["output_weight"] = w_out
        p["output_bias"] = torch.zeros(L)
    return p


ANGULAR_PREDICT_ERROR = (
    "Predictor does not support the angular-margin head on this path: its "
    "forward needs the true label, which prediction does not "
    "have; use fused_head=True / --fused_head, which scores the "
    "margin-free logits")


def _unit_rows(x, out=None):
    """bf16 unit rows of x [R, EP] bf16 as the angular head's training
    forward forms them (inv_rownorm + rowscale; EP = 128 on the device),
    else through torch ops.  ``out``: a contiguous tensor like x to write
    into (its address is kept)."""
    if out is None:
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
    if x.is_cuda and x.shape[1] == 128:
        x = x.contiguous()
        inv = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        Fn.ext().inv_rownorm(x, inv)
        Fn.ext().rowscale(x, inv, out)
    else:
        out.copy_(F.normalize(x.float()))
    return out


def _pad32(x):
    """x [R, E] zero-padded to the next multiple of 32 columns (the oracle's
    head_topk shares the kernel's EP contract; zeros add nothing to a dot
    product)."""
    return F.pad(x.detach().float(), (0, round_up(x.shape[1]) - x.shape[1]))


def _reject_packed(model) -> None:
    """forward_packed is label-free inference: eval mode, default head."""
    assert not model.training, "forward_packed is inference only: eval() first"
    if model.option.angular_margin_loss:
        raise ValueError(ANGULAR_PREDICT_ERROR)


class Code2VecTorch(nn.Module):
    """Reference-math backend (fp32, stock torch ops) — CPU path + oracle."""

    backend = "torch"

    def __init__(self, option, logical: Optional[Dict[str, torch.Tensor]] = None):
        super().__init__()
        self.option = option
        if logical is None:
            logical = init_logical_params(option)
        self.terminal_embedding = nn.Parameter(logical["terminal_embedding"].clone())
        self.path_embedding = nn.Parameter(logical["path_embedding"].clone())
        self.input_weight = nn.Parameter(logical["input_weight"].clone())
        self.ln_gamma = nn.Parameter(logical["ln_gamma"].clone())
        self.ln_beta = nn.Parameter(logical["ln_beta"].clone())
        self.attention_a = nn.Parameter(logical["attention_a"].clone())
        self.output_weight = nn.Parameter(logical["output_weight"].clone())
        if not option.angular_margin_loss:
            self.output_bias = nn.Parameter(logical["output_bias"].clone())
        else:
            self.output_bias = None
        if option.angular_margin_loss:
            self.cos_m = math.cos(option.angular_margin)
            self.sin_m = math.sin(option.angular_margin)
        self.dropout_p = (
            option.dropout_prob if 0.0 < option.dropout_prob < 1.0 else 0.0
        )

    def forward(self, starts, paths, ends, label):
        opt = self.option
        ccv = R.gather_concat(
            starts, paths, ends, self.terminal_embedding, self.path_embedding
        )
        ccv = R.combiner(ccv, self.input_weight, self.ln_gamma, self.ln_beta)
        if self.dropout_p > 0.0:
            ccv = F.dropout(ccv, p=self.dropout_p, training=self.training)
        mask = (starts > 0).float()
        attn = R.attention(ccv, self.attention_a, mask)
        cv = R.code_vector(ccv, attn)
        if opt.angular_margin_loss:
            outputs = R.angular_margin_head(
                cv, self.output_weight, label, self.cos_m, self.sin_m,
                opt.inverse_temp,
            )
        else:
            outputs = R.output_head(cv, self.output_weight, self.output_bias)
        return outputs, cv, attn

    @torch.no_grad()
    def encode(self, starts, paths, ends):
        """Code2VecHIP.encode's contract on the oracle backend: (code_vector
        [B, E], the same again — fp32 stands in for the bf16 copy —,
        attention [B, C])."""
        assert not self.training, "encode is inference only: eval() first"
        ccv = R.gather_concat(
            starts, paths, ends, self.terminal_embedding, self.path_embedding
        )
        ccv = R.combiner(ccv, self.input_weight, self.ln_gamma, self.ln_beta)
        attn = R.attention(ccv, self.attention_a, (starts > 0).float())
        cv = R.code_vector(ccv, attn)
        return cv, cv, attn

    @torch.no_grad()
    def encode_packed(self, starts, paths, ends, lengths):
        """Code2VecHIP.encode_packed's contract on the oracle backend (pads
        to the longest method, as ``forward_packed`` does)."""
        assert not self.training, "encode_packed is inference only: eval() first"
        padded, real = self._pad_packed(starts, paths, ends, lengths)
        cv, cvb, attn = self.encode(*padded)
        return cv, cvb, attn[real]

    def _pad_packed(self, starts, paths, ends, lengths):
        """The [B, longest] rectangles of a packed batch and the mask of
        their real positions."""
        M = starts.numel()
        lens = R.check_packed_lengths(lengths, M)
        B, C = lens.numel(), int(lens.max())
        # row-major positions of the real contexts in the [B, C] rectangle
        real = (torch.arange(C)[None, :] < lens[:, None]).to(starts.device)
        padded = []
        for t in (starts, paths, ends):
            buf = torch.zeros(B, C, dtype=t.dtype, device=t.device)
            buf[real] = t.reshape(-1)
            padded.append(buf)
        return padded, real

    @torch.no_grad()
    def head_topk(self, cvb, k: int):
        """Code2VecHIP.head_topk's contract in fp32 through the oracle: the
        default head's logits, or inverse_temp * cosine (no margin) for the
        angular head."""
        opt = self.option
        if not opt.angular_margin_loss:
            return R.head_topk(_pad32(cvb), _pad32(self.output_weight), k,
                               bias=self.output_bias.detach(), scale=1.0)
        return R.head_topk(_pad32(F.normalize(cvb)),
                           _pad32(F.normalize(self.output_weight.detach())),
                           k, bias=None, scale=opt.inverse_temp)

    @torch.no_grad()
    def forward_packed(self, starts, paths, ends, lengths):
        """Code2VecHIP.forward_packed's contract on the oracle backend:
        pads to the longest method of the batch, calls ``forward`` and
        slices the attention back to ragged.  Returns (outputs [B, L],
        code_vector [B, E], attention [M]).  (A method whose rows are all
        PAD gets the padded row's uniform weights here, 1/n from K21; its
        code vector is the same.)"""
        _reject_packed(self)
        padded, real = self._pad_packed(starts, paths, ends, lengths)
        label = torch.zeros(real.shape[0], dtype=torch.int64,
                            device=starts.device)
        outputs, cv, attn = self.forward(*padded, label)
        return outputs, cv, attn[real]

    def forward_packed_train(self, starts, paths, ends, lengths, label):
        """Code2VecHIP.forward_packed_train's contract on the oracle
        backend, with autograd on: pads to the longest method of the batch
        and calls ``forward``.  Returns (outputs [B, L], code_vector
        [B, E], attention [M])."""
        padded, real = self._pad_packed(starts, paths, ends, lengths)
        outputs, cv, attn = self.forward(*padded, label)
        return outputs, cv, attn[real]

    def loss(self, outputs, label, class_weight):
        return R.logsoftmax_nll(outputs, label, class_weight)


class Code2VecHIP(nn.Module):
    """MI355X backend — padded bf16 parameters, hand-written HIP kernels."""

    backend = "hip"

    def __init__(self, option, logical: Optional[Dict[str, torch.Tensor]] = None,
                 device: Optional[torch.device] = None):
        super().__init__()
        self.option = option
        if logical is None:
            logical = init_logical_params(option)
        device = device or torch.device("cuda")
        dt, dp, E = (
            option.terminal_embed_size,
            option.path_embed_size,
            option.encode_size,
        )
        self.TS = seg_round(dt)
        self.PS = seg_round(dp)
        self.EP = round_up(E)
        # combiner K: segments at offsets [0, TS, TS+PS], summed width
        # padded to the MFMA K granularity (gather zero-fills the tail)
        self.KP = round_up(2 * self.TS + self.PS, 32)
        self.E = E

        def pad2(t, rows, cols):
            out = torch.zeros(rows, cols, dtype=torch.float32)
            out[: t.shape[0], : t.shape[1]] = t
            return out

        def pad1(t, n):
            out = torch.zeros(n, dtype=torch.float32)
            out[: t.shape[0]] = t
            return out

        term = pad2(logical["terminal_embedding"], option.terminal_count, self.TS)
        path = pad2(logical["path_embedding"], option.path_count, self.PS)
        # combiner weight: logical [E, K=2dt+dp] -> padded TRANSPOSED layout
        # [EP, KP] (so MFMA B fragments are contiguous; see combiner.hip).
        w_in = logical["input_weight"]  # [E, K]
        w_pad = torch.zeros(self.EP, self.KP, dtype=torch.float32)
        w_pad[:E, :dt] = w_in[:, :dt]
        w_pad[:E, self.TS : self.TS + dp] = w_in[:, dt : dt + dp]
        w_pad[:E, self.TS + self.PS : self.TS + self.PS + dt] = w_in[:, dt + dp :]

        w_out = torch.zeros(option.label_count, self.EP, dtype=torch.float32)
        w_out[:, :E] = logical["output_weight"]

        self.terminal_embedding = nn.Parameter(term.to(device=device, dtype=torch.bfloat16))
        self.path_embedding = nn.Parameter(path.to(device=device, dtype=torch.bfloat16))
        self.input_weight = nn.Parameter(w_pad.to(device=device, dtype=torch.bfloat16))
        self.ln_gamma = nn.Parameter(pad1(logical["ln_gamma"], self.EP).to(device))
        self.ln_beta = nn.Parameter(pad1(logical["ln_beta"], self.EP).to(device))
        self.attention_a = nn.Parameter(pad1(logical["attention_a"], self.EP).to(device))
        self.output_weight = nn.Parameter(w_out.to(device=device, dtype=torch.bfloat16))
        if not option.angular_margin_loss:
            self.output_bias = nn.Parameter(logical["output_bias"].to(device))
        else:
            self.output_bias = None
        if option.angular_margin_loss:
            self.cos_m = math.cos(option.angular_margin)
            self.sin_m = math.sin(option.angular_margin)
        self.dropout_p = (
            option.dropout_prob if 0.0 < option.dropout_prob < 1.0 else 0.0
        )

    def forward(self, starts, paths, ends, label):
        cv, cvb, attn = self._code_vector(starts, paths, ends)
        outputs = self._head(cvb, label)
        return outputs, cv[:, : self.E], attn

    def _code_vector(self, starts, paths, ends):
        """K1-K9: (cv [B, EP] f32, cvb [B, EP] bf16, attn [B, C]); what
        ``forward`` and ``encode`` share."""
        B, C = starts.shape
        starts = starts.to(torch.int32)
        paths = paths.to(torch.int32)
        ends = ends.to(torch.int32)
        x = y = cvb = None
        if Fn.FUSE_GATHER_COMBINER:
            # fused K1-K6: the concat tensor is never materialized
            y = Fn.FusedGatherCombiner.apply(
                starts, paths, ends, self.terminal_embedding,
                self.path_embedding, self.input_weight, self.ln_gamma,
                self.ln_beta, self.E, self.dropout_p, self.training,
            )
        else:
            x = Fn.GatherConcat.apply(
                starts, paths, ends, self.terminal_embedding,
                self.path_embedding, self.training
            )
        if y is None and Fn.combiner_attention_pool_supported(
                x, self.input_weight):
            # K3-K9 as one node: its backward never writes the attention
            # gradient, and the forward hands back cv in bf16 as well
            cv, attn, cvb = Fn.CombinerAttentionPool.apply(
                x, self.input_weight, self.ln_gamma, self.ln_beta,
                self.attention_a, starts, self.E, self.dropout_p,
                self.training,
            )
        else:
            if y is None:
                y = Fn.CombinerLNTanh.apply(
                    x, self.input_weight, self.ln_gamma, self.ln_beta,
                    self.E, self.dropout_p, self.training,
                )
            ccv = y.view(B, C, self.EP)
            cv, attn = Fn.AttentionPool.apply(ccv, self.attention_a, starts,
                                              self.E)
            cvb = cv.to(torch.bfloat16)
        return cv, cvb, attn

    @torch.no_grad()
    def encode(self, starts, paths, ends):
        """Label-free inference up to the code vector, with the kernels
        ``forward`` launches in eval mode.  Returns (code_vector [B, E] f32,
        cvb [B, EP] bf16 — what the head reads —, attention [B, C])."""
        assert not self.training, "encode is inference only: eval() first"
        cv, cvb, attn = self._code_vector(starts, paths, ends)
        return cv[:, : self.E], cvb, attn

    @torch.no_grad()
    def encode_packed(self, starts, paths, ends, lengths):
        """``encode`` on a packed batch (``forward_packed``'s inputs and
        kernels).  Returns (code_vector [B, E], cvb [B, EP] bf16, attention
        [M])."""
        assert not self.training, "encode_packed is inference only: eval() first"
        cv, cvb, attn = self._code_vector_packed(starts, paths, ends, lengths)
        return cv[:, : self.E], cvb, attn

    def train(self, mode: bool = True):
        # the optimizer's kernels write parameters without touching their
        # version counters: entering or leaving training marks the unit-row
        # image stale (eval() on a model in eval mode changes nothing)
        if mode != self.training:
            self._uw_key = None
        return super().train(mode)

    def _unit_output_weight(self):
        """Unit-row bf16 image of output_weight for the angular head.  ONE
        buffer for the model's lifetime, refreshed IN PLACE when the
        parameter has changed (an in-place torch op or load_state_dict bumps
        ``_version``; a rebind moves ``data_ptr``; ``train()`` marks it
        stale, see there): a captured graph that read it keeps a valid
        address, and sees the new rows once this has run again."""
        w = self.output_weight
        key = (w._version, w.data_ptr())
        buf = getattr(self, "_uw_buf", None)
        if buf is None or buf.shape != w.shape or buf.device != w.device:
            buf = torch.empty_like(w.detach(),
                                   memory_format=torch.contiguous_format)
            self._uw_buf, self._uw_key = buf, None
        if getattr(self, "_uw_key", None) != key:
            _unit_rows(w.detach(), out=buf)
            self._uw_key = key
        return buf

    @torch.no_grad()
    def prepare_head_topk(self) -> None:
        """Bring what ``head_topk`` reads besides the parameters up to date
        (the angular head's unit-row image).  ``head_topk`` does this
        itself; a replayed graph of it cannot, so its owner calls this
        before every replay."""
        if self.option.angular_margin_loss:
            self._unit_output_weight()

    @torch.no_grad()
    def head_topk(self, cvb, k: int):
        """The k most likely labels of code vectors cvb [B, EP] bf16 and the
        log-sum-exp over all labels, through K23: no [B, L] tensor.  Default
        head: logits cvb . W + b.  Angular head: inverse_temp * cosine, the
        margin-free logits its training forward gives every label but the
        true one.  Returns (vals [B, k] f32, idx [B, k] i64, lse [B] f32)."""
        opt = self.option
        if not opt.angular_margin_loss:
            return Fn.head_topk(cvb, self.output_weight, k,
                                bias=self.output_bias.detach(), scale=1.0)
        return Fn.head_topk(_unit_rows(cvb), self._unit_output_weight(), k,
                            bias=None, scale=opt.inverse_temp)

    def _head(self, cvb, label):
        """The output head over cvb [B, EP] bf16 (padded and packed
        training share it: the heads see the code vectors and the label
        only)."""
        opt = self.option
        if opt.angular_margin_loss:
            outputs = Fn.angular_margin_head_hip(
                cvb, self.output_weight, label,
                self.cos_m, self.sin_m, opt.inverse_temp,
            )
        else:
            if Fn.fused_head_loss_supported(cvb, self.output_weight,
                                            self.training):
                # fused head+loss path: logits are computed WITHOUT autograd
                # tracking; loss() builds the single FusedHeadLoss node whose
                # backward recomputes G (dlogits never materialized).  The
                # returned outputs tensor itself carries no grad — training
                # flows through model.loss(), which is the only consumer
                # (reference main.py:172-174).
                outputs = Fn.head_logits_with_stats(
                    cvb.detach(), self.output_weight.detach(),
                    self.output_bias.detach())
                outputs._c2v_fused_head = (cvb, self.output_weight,
                                           self.output_bias)
            else:
                outputs = Fn.OutputHead.apply(
                    cvb, self.output_weight, self.output_bias
                )
        return outputs

    def forward_packed_train(self, starts, paths, ends, lengths, label,
                             offsets=None, row_capacity=None):
        """Training forward on a packed batch (autograd on): flat [M] index
        tensors holding the methods' contexts back to back and the
        methods' row counts (list or CPU int tensor; every n >= 1, sum ==
        M, checked on the host before any launch).  No pad row is
        gathered, combined, scored or back-propagated.  Returns (outputs
        [B, L], code_vector [B, E], attention [M]); ``loss`` and
        ``backward`` follow as after ``forward``.

        ``offsets``: device int32 [B+1] offsets a loader built from these
        same lengths (saves the host-to-device copy here).
        ``row_capacity``: the most rows any batch of the run will have
        (batch_size * max_path_length); the row-sized persistent scratch of
        the table-gradient grouping is then allocated once for that many
        rows instead of once per distinct M."""
        M = starts.numel()
        starts = starts.reshape(-1).to(torch.int32).contiguous()
        paths = paths.reshape(-1).to(torch.int32).contiguous()
        ends = ends.reshape(-1).to(torch.int32).contiguous()
        lens, offsets = Fn.packed_offsets(lengths, M, starts.device, offsets)
        if not (paths.numel() == M and ends.numel() == M):
            raise ValueError("packed starts/paths/ends sizes differ")
        x = Fn.GatherConcat.apply(
            starts.view(M, 1), paths.view(M, 1), ends.view(M, 1),
            self.terminal_embedding, self.path_embedding, True,
            row_capacity)
        if Fn.combiner_attention_pool_supported(x, self.input_weight):
            cv, attn, cvb = Fn.combiner_attention_pool_packed(
                x, self.input_weight, self.ln_gamma, self.ln_beta,
                self.attention_a, starts, lens, self.E, self.dropout_p,
                self.training, offsets=offsets)
        else:
            y = Fn.CombinerLNTanh.apply(
                x, self.input_weight, self.ln_gamma, self.ln_beta,
                self.E, self.dropout_p, self.training)
            cv, attn = Fn.attention_pool_packed_train(
                y, self.attention_a, starts, lens, self.E, offsets=offsets)
            cvb = cv.to(torch.bfloat16)
        outputs = self._head(cvb, label)
        return outputs, cv[:, : self.E], attn

    @torch.no_grad()
    def forward_packed(self, starts, paths, ends, lengths):
        """Inference on a packed batch: flat [M] index tensors holding the
        contexts of all methods back to back, and the methods' row counts
        (list or CPU int tensor; every n >= 1, sum == M).  No pads, no cap
        on a method's length.  Returns (outputs [B, L], code_vector
        [B, E], attention [M]).  Gather and combiner are row-local and K21
        is segment-local, so a method's code vector and attention do not
        depend on the rest of the batch.  Forward only."""
        _reject_packed(self)
        cv, cvb, attn = self._code_vector_packed(starts, paths, ends, lengths)
        outputs = Fn.OutputHead.apply(cvb, self.output_weight,
                                      self.output_bias)
        return outputs, cv[:, : self.E], attn

    def _code_vector_packed(self, starts, paths, ends, lengths):
        """K1-K6 + K21 on a packed batch: (cv [B, EP] f32, cvb [B, EP]
        bf16, attn [M]); what ``forward_packed`` and ``encode_packed``
        share."""
        M = starts.numel()
        lens = R.check_packed_lengths(lengths, M)
        starts = starts.reshape(-1).to(torch.int32).contiguous()
        paths = paths.reshape(-1).to(torch.int32).contiguous()
        ends = ends.reshape(-1).to(torch.int32).contiguous()
        x = Fn.GatherConcat.apply(
            starts.view(M, 1), paths.view(M, 1), ends.view(M, 1),
            self.terminal_embedding, self.path_embedding, False)
        y = Fn.CombinerLNTanh.apply(
            x, self.input_weight, self.ln_gamma, self.ln_beta, self.E,
            0.0, False)
        return Fn.attention_pool_packed(
            y, self.attention_a, starts, lens, self.E)

    def loss(self, outputs, label, class_weight):
        fused = getattr(outputs, "_c2v_fused_head", None)
        if fused is not None:
            cvb, w, bias = fused
            del outputs._c2v_fused_head
            return Fn.FusedHeadLoss.apply(
                outputs.contiguous(), cvb, w, bias, label, class_weight)
        return Fn.FusedLogSoftmaxNLL.apply(
            outputs.contiguous(), label, class_weight)

    # ------------------------------------------------------------------
    def reference_state_dict(self) -> Dict[str, torch.Tensor]:
        """Checkpoint in the reference's state_dict format
        (keys/shapes of reference model/model.py, fp32, unpadded) so
        ``code2vec.model`` files are interchangeable."""
        opt = self.option
        dt, dp, E = opt.terminal_embed_size, opt.path_embed_size, opt.encode_size
        w_pad = self.input_weight.float()  # [EP, KP] transposed layout
        w_in = torch.cat(
            [
                w_pad[:E, :dt],
                w_pad[:E, self.TS : self.TS + dp],
                w_pad[:E, self.TS + self.PS : self.TS + self.PS + dt],
            ],
            dim=1,
        )
        sd = {
            "terminal_embedding.weight": self.terminal_embedding[:, :dt].float().cpu(),
            "path_embedding.weight": self.path_embedding[:, :dp].float().cpu(),
            "input_linear.weight": w_in.cpu(),
            "input_layer_norm.weight": self.ln_gamma[:E].detach().float().cpu(),
            "input_layer_norm.bias": self.ln_beta[:E].detach().float().cpu(),
            "attention_parameter": self.attention_a[:E].detach().float().cpu(),
        }
        if opt.angular_margin_loss:
            sd["output_linear"] = self.output_weight[:, :E].float().cpu()
        else:
            sd["output_linear.weight"] = self.output_weight[:, :E].float().cpu()
            sd["output_linear.bias"] = self.output_bias.detach().float().cpu()
        return sd


def reference_state_dict_torch(model: Code2VecTorch) -> Dict[str, torch.Tensor]:
    """Reference-format state_dict for the torch backend."""
    opt = model.option
    sd = {
        "terminal_embedding.weight": model.terminal_embedding.detach().cpu(),
        "path_embedding.weight": model.path_embedding.detach().cpu(),
        "input_linear.weight": model.input_weight.detach().cpu(),
        "input_layer_norm.weight": model.ln_gamma.detach().cpu(),
        "input_layer_norm.bias": model.ln_beta.detach().cpu(),
        "attention_parameter": model.attention_a.detach().cpu(),
    }
    if opt.angular_margin_loss:
        sd["output_linear"] = model.output_weight.detach().cpu()
    else:
        sd["output_linear.weight"] = model.output_weight.detach().cpu()
        sd["output_linear.bias"] = model.output_bias.detach().cpu()
    return sd


def logical_from_reference_state_dict(sd, option) -> Dict[str, torch.Tensor]:
    """Convert a reference-format state_dict (keys of reference
    model/model.py; our checkpoints use the same format) into logical
    init tensors, so checkpoints load into either backend."""
    p = {
        "terminal_embedding": sd["terminal_embedding.weight"].float(),
        "path_embedding": sd["path_embedding.weight"].float(),
        "input_weight": sd["input_linear.weight"].float(),
        "ln_gamma": sd["input_layer_norm.weight"].float(),
        "ln_beta": sd["input_layer_norm.bias"].float(),
        "attention_a": sd["attention_parameter"].float(),
    }
    if "output_linear" in sd:  # angular-margin head (Parameter, no bias)
        p["output_weight"] = sd["output_linear"].float()
    else:
        p["output_weight"] = sd["output_linear.weight"].float()
        p["output_bias"] = sd["output_linear.bias"].float()
    return p


def build_model(option, backend: str = "auto", logical=None, device=None):
    """Factory: 'hip' on CUDA devices, 'torch' on CPU (or forced)."""
    if backend == "auto":
        dev = device or option.device
        backend = "hip" if (dev is not None and torch.device(dev).type == "cuda") else "torch"
    if backend == "hip":
        return Code2VecHIP(option, logical=logical, device=device or option.device)
    model = Code2VecTorch(option, logical=logical)
    if device is not None:
        model = model.to(device)
    return model
