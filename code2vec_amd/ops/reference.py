"""Pure-PyTorch reference implementations of every framework op.

These define the exact math (reference model/model.py:44-105 and
main.py:251-264) and serve three roles:
1. the CPU training/eval path,
2. the numerical oracle that every HIP kernel is tested against
   (tests/test_kernels_gpu.py),
3. documentation of each kernel's contract.

Shapes: B batch, C contexts (max_path_length), dt/dp terminal/path embed
sizes, E encode size, L label count, T/P terminal/path vocab sizes.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

NINF = -3.4 * math.pow(10, 38)  # matches reference model/model.py:12


def gather_concat(starts, paths, ends, terminal_weight, path_weight):
    """K1/K2: triple embedding gather + concat (reference model/model.py:48-51).

    starts/paths/ends: int [B, C]; returns [B, C, 2*dt+dp].
    """
    e_s = F.embedding(starts.long(), terminal_weight)
    e_p = F.embedding(paths.long(), path_weight)
    e_e = F.embedding(ends.long(), terminal_weight)
    return torch.cat((e_s, e_p, e_e), dim=2)


def combiner(ccv, weight, gamma, beta, eps: float = 1e-5):
    """K3-K5: context combiner = Linear(no bias) -> LayerNorm -> tanh
    (reference model/model.py:54-57).

    ccv: [B, C, 2dt+dp]; weight: [E, 2dt+dp]; returns [B, C, E].
    """
    x = F.linear(ccv, weight)
    shape = x.shape
    x = F.layer_norm(x.view(-1, shape[-1]), (shape[-1],), gamma, beta, eps)
    return torch.tanh(x).view(shape)


def attention(ccv, a, mask):
    """K7/K8: masked single-query attention scores + softmax
    (reference model/model.py:90-105).

    ccv: [B, C, E]; a: [E]; mask: [B, C] float (1 valid, 0 pad).
    Returns attention [B, C].
    """
    scores = torch.sum(ccv * a.unsqueeze(0).unsqueeze(0), dim=2)
    scores = scores * mask + (1.0 - mask) * NINF
    return F.softmax(scores, dim=1)


def code_vector(ccv, attn):
    """K9: attention-weighted sum (reference model/model.py:68-69)."""
    return torch.sum(ccv * attn.unsqueeze(-1), dim=1)


def attention_code_vector(ccv, a, mask):
    """Fused K7+K8+K9 — contract of the HIP attention kernel."""
    attn = attention(ccv, a, mask)
    return code_vector(ccv, attn), attn


def output_head(cv, weight, bias):
    """K10: label projection (reference model/model.py:83)."""
    return F.linear(cv, weight, bias)


def angular_margin_head(cv, weight, label, cos_m, sin_m, inverse_temp):
    """K11: ArcFace-style head (reference model/model.py:71-80).

    Note the reference computes but never uses th/mm; the actual math is:
    phi = cos*cos_m - sin*sin_m, phi where cos>0 else cos,
    blend by one-hot, scale by inverse_temp.
    """
    cosine = F.linear(F.normalize(cv), F.normalize(weight))
    sine = torch.sqrt(torch.clamp(1.0 - cosine * cosine, min=0.0))
    phi = cosine * cos_m - sine * sin_m
    phi = torch.where(cosine > 0, phi, cosine)
    one_hot = torch.zeros_like(cosine)
    one_hot.scatter_(1, label.view(-1, 1).long(), 1)
    outputs = one_hot * phi + (1.0 - one_hot) * cosine
    return outputs * inverse_temp


ROW_TOPK_MAX_K = 16


def check_row_topk_args(x, k: int) -> None:
    """Argument contract shared by the oracle and the HIP op."""
    if x.dim() != 2:
        raise ValueError(f"row_topk: x must be [B, L], got {tuple(x.shape)}")
    if not 1 <= k <= ROW_TOPK_MAX_K:
        raise ValueError(
            f"row_topk: k must be in 1..{ROW_TOPK_MAX_K}, got {k}")
    if k > x.shape[1]:
        raise ValueError(
            f"row_topk: k = {k} exceeds row length {x.shape[1]}")


def row_topk(x, k: int):
    """K19: per-row top-k + log-sum-exp.

    Total order: descending value, ties to the smallest column (a stable
    descending sort) — ``torch.topk`` does not promise this.  Returns
    (vals f32 [B, k], idx i64 [B, k], lse f32 [B]); lse runs over the whole
    row, so ``exp(vals - lse[:, None])`` are softmax probabilities.
    """
    check_row_topk_args(x, k)
    xf = x.float()
    vals, idx = torch.sort(xf, dim=1, descending=True, stable=True)
    return (vals[:, :k].contiguous(), idx[:, :k].contiguous(),
            torch.logsumexp(xf, dim=1))


SIM_TOPK_MAX_EP = 512


def check_sim_topk_args(q, db, k: int, exclude=None) -> None:
    """Argument contract shared by the oracle and the HIP op (K20)."""
    if q.dim() != 2 or db.dim() != 2:
        raise ValueError(
            f"sim_topk: q must be [nq, EP] and db [N, EP], got "
            f"{tuple(q.shape)} and {tuple(db.shape)}")
    EP, N = q.shape[1], db.shape[0]
    if db.shape[1] != EP:
        raise ValueError(
            f"sim_topk: q has EP = {EP}, db has EP = {db.shape[1]}")
    if EP % 32 != 0 or not 32 <= EP <= SIM_TOPK_MAX_EP:
        raise ValueError(
            f"sim_topk: EP must be a multiple of 32 in "
            f"32..{SIM_TOPK_MAX_EP}, got {EP}")
    if not 1 <= k <= ROW_TOPK_MAX_K:
        raise ValueError(
            f"sim_topk: k must be in 1..{ROW_TOPK_MAX_K}, got {k}")
    if N >= 1 << 31:
        raise ValueError("sim_topk: N must be < 2^31")
    if k > N:
        raise ValueError(f"sim_topk: k = {k} exceeds the index's {N} rows")
    if exclude is not None:
        if exclude.dim() != 1 or exclude.shape[0] != q.shape[0] \
                or exclude.dtype != torch.int64:
            raise ValueError("sim_topk: exclude must be int64 [nq]")
        if k > N - 1:
            raise ValueError(
                f"sim_topk: with exclude, k = {k} must be below the "
                f"index's {N} rows")


def sim_topk(q, db, k: int, exclude=None):
    """K20: the k index rows of ``db`` with the largest dot product per
    query row of ``q``, in row_topk's total order (descending score, ties
    to the smallest index row).  ``exclude`` [nq] i64 names one index row
    per query that is never returned (-1: none).  Returns (vals f32
    [nq, k], idx i64 [nq, k])."""
    check_sim_topk_args(q, db, k, exclude)
    S = q.float() @ db.float().t()
    if exclude is not None:
        ex = exclude.to(S.device)
        rows = torch.nonzero((ex >= 0) & (ex < db.shape[0])).flatten()
        S[rows, ex[rows]] = float("-inf")
    return row_topk(S, k)[:2]


SIM_RANGE_MAX_PAIRS = 1 << 24


class TooManyPairs(ValueError):
    """sim_range counted more pairs than ``max_pairs`` allows."""

    def __init__(self, total: int, threshold: float, max_pairs: int):
        super().__init__(
            f"sim_range: {total} pairs score at least the threshold "
            f"{threshold}, more than max_pairs = {max_pairs}; raise the "
            f"threshold or max_pairs")
        self.total = total
        self.threshold = threshold
        self.max_pairs = max_pairs


def sim_range_threshold(threshold) -> float:
    """The threshold as the fp32 value every comparison uses."""
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(
            f"sim_range: threshold must be a number, got {threshold!r}")
    t32 = float(torch.tensor(t, dtype=torch.float32)) if math.isfinite(t) \
        else t
    if not math.isfinite(t32):
        raise ValueError(
            f"sim_range: threshold must be finite in fp32, got {threshold}")
    return t32


def check_sim_range_args(q, db, threshold, exclude=None, after=None,
                         max_pairs: int = SIM_RANGE_MAX_PAIRS) -> None:
    """Argument contract shared by the oracle and the HIP op (K24)."""
    if q.dim() != 2 or db.dim() != 2:
        raise ValueError(
            f"sim_range: q must be [nq, EP] and db [N, EP], got "
            f"{tuple(q.shape)} and {tuple(db.shape)}")
    EP, N = q.shape[1], db.shape[0]
    if db.shape[1] != EP:
        raise ValueError(
            f"sim_range: q has EP = {EP}, db has EP = {db.shape[1]}")
    if EP % 32 != 0 or not 32 <= EP <= SIM_TOPK_MAX_EP:
        raise ValueError(
            f"sim_range: EP must be a multiple of 32 in "
            f"32..{SIM_TOPK_MAX_EP}, got {EP}")
    if not 1 <= N < 1 << 31:
        raise ValueError(f"sim_range: N must be in 1..2^31-1, got {N}")
    sim_range_threshold(threshold)
    for name, t in (("exclude", exclude), ("after", after)):
        if t is not None and (not torch.is_tensor(t) or t.dim() != 1
                              or t.shape[0] != q.shape[0]
                              or t.dtype != torch.int64):
            raise ValueError(f"sim_range: {name} must be int64 [nq]")
    if isinstance(max_pairs, bool) or not isinstance(max_pairs, int) \
            or max_pairs < 0:
        raise ValueError(
            f"sim_range: max_pairs must be an integer >= 0, got {max_pairs!r}")


def sim_range_mask(S, t32: float, exclude=None, after=None):
    """Allowed pairs of a score block S [n, N] f32 (exclude/after [n])."""
    mask = S >= torch.tensor(t32, dtype=torch.float32, device=S.device)
    if exclude is not None or after is not None:
        cols = torch.arange(S.shape[1], device=S.device).view(1, -1)
        if exclude is not None:
            mask &= cols != exclude.to(S.device).view(-1, 1)
        if after is not None:
            mask &= cols > after.to(S.device).view(-1, 1)
    return mask


def sim_range(q, db, threshold, exclude=None, after=None,
              max_pairs: int = SIM_RANGE_MAX_PAIRS):
    """K24: every index row of ``db`` whose dot product with a query row of
    ``q`` is at least fp32(threshold), as a CSR: (offsets i64 [nq + 1],
    rows i64 [nnz], scores f32 [nnz]); query i owns
    rows[offsets[i]:offsets[i + 1]], strictly ascending.  ``exclude`` [nq]
    i64 names one row per query that is never reported (-1: none);
    ``after`` [nq] i64 admits only rows > after[i] (-1: all).  More than
    ``max_pairs`` pairs raise TooManyPairs (a ValueError)."""
    check_sim_range_args(q, db, threshold, exclude, after, max_pairs)
    t32 = sim_range_threshold(threshold)
    nq = q.shape[0]
    S = q.float() @ db.float().t()
    mask = sim_range_mask(S, t32, exclude, after)
    counts = mask.sum(dim=1)
    total = int(counts.sum())
    if total > max_pairs:
        raise TooManyPairs(total, t32, max_pairs)
    offsets = torch.zeros(nq + 1, dtype=torch.int64, device=S.device)
    offsets[1:] = torch.cumsum(counts, 0)
    # nonzero is row-major: ascending query, then ascending index row
    hit = torch.nonzero(mask)
    return offsets, hit[:, 1].contiguous(), S[hit[:, 0], hit[:, 1]]


def check_head_topk_args(q, w, k: int, bias=None, scale: float = 1.0) -> None:
    """Argument contract shared by the oracle and the HIP op (K23)."""
    if q.dim() != 2 or w.dim() != 2:
        raise ValueError(
            f"head_topk: q must be [nq, EP] and w [L, EP], got "
            f"{tuple(q.shape)} and {tuple(w.shape)}")
    EP, L = q.shape[1], w.shape[0]
    if w.shape[1] != EP:
        raise ValueError(
            f"head_topk: q has EP = {EP}, w has EP = {w.shape[1]}")
    if EP % 32 != 0 or not 32 <= EP <= SIM_TOPK_MAX_EP:
        raise ValueError(
            f"head_topk: EP must be a multiple of 32 in "
            f"32..{SIM_TOPK_MAX_EP}, got {EP}")
    if not 1 <= k <= ROW_TOPK_MAX_K:
        raise ValueError(
            f"head_topk: k must be in 1..{ROW_TOPK_MAX_K}, got {k}")
    if L >= 1 << 31:
        raise ValueError("head_topk: L must be < 2^31")
    if k > L:
        raise ValueError(f"head_topk: k = {k} exceeds the head's {L} labels")
    if bias is not None and (bias.dim() != 1 or bias.shape[0] != L
                             or bias.dtype != torch.float32):
        raise ValueError(f"head_topk: bias must be float32 [{L}]")
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        # a non-positive scale would reverse or flatten the order
        raise ValueError(
            f"head_topk: scale must be finite and > 0, got {scale}")


def head_topk(q, w, k: int, bias=None, scale: float = 1.0):
    """K23: the k most likely labels of a head without its logits matrix.
    Logits z[i, l] = scale * sum_e q[i, e] w[l, e] + bias[l] in fp32;
    selection in row_topk's total order (descending value, ties to the
    smallest label); lse over all L labels.  A ``bias`` entry of -inf masks
    a label: it adds nothing to lse and sorts below every finite logit.
    Returns (vals f32 [nq, k], idx i64 [nq, k], lse f32 [nq])."""
    check_head_topk_args(q, w, k, bias, scale)
    z = float(scale) * (q.float() @ w.float().t())
    if bias is not None:
        z = z + bias.to(z.device)
    return row_topk(z, k)


def logsoftmax_nll(logits, label, weight):
    """K12: log_softmax + weighted NLL (reference main.py:251-264 with the
    criterion built at main.py:129-130).

    weight: [L] per-class weights (1/freq — effectively all ones, see
    data/vocab.py docstring).  Reduction follows nn.NLLLoss default:
    sum(w_yi * -logp_yi) / sum(w_yi).
    """
    logp = F.log_softmax(logits.float(), dim=1)
    return F.nll_loss(logp, label.long(), weight=weight)


def check_packed_lengths(lengths, M: int):
    """Host-side contract of a packed batch's lengths (list or CPU
    int32/int64 tensor): at least one method, every n >= 1, sum == M.
    Returns them as a CPU int64 tensor."""
    if isinstance(lengths, torch.Tensor):
        if lengths.is_cuda or lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError(
                "packed lengths must be a CPU int32/int64 tensor or a list")
        lens = lengths.detach().to(torch.int64).reshape(-1)
    else:
        lens = torch.tensor([int(n) for n in lengths], dtype=torch.int64)
    if lens.numel() < 1:
        raise ValueError("packed lengths: no methods")
    if int(lens.min()) < 1:
        raise ValueError(
            f"packed lengths: every method needs n >= 1 rows, got "
            f"{int(lens.min())}")
    total = int(lens.sum())
    if total != int(M):
        raise ValueError(
            f"packed lengths sum to {total}, the batch has {int(M)} rows")
    if total >= 1 << 31:
        raise ValueError("packed batch: M must be < 2^31")
    return lens


def attention_pool_packed(ccv, a, starts, lengths, E: int):
    """K21: attention pool over a packed batch, a loop over segments in
    fp32.

    ccv: [M, EP] rows of all methods back to back; a: [EP]; starts: [M]
    (mask = starts > 0); lengths: host list / CPU int tensor, method b owns
    the next lengths[b] rows.  Softmax over each method's own rows, pool
    over the round8(E) valid columns, columns past them zero.  Returns
    (cv f32 [B, EP], cvb bf16 [B, EP], attn f32 [M])."""
    M, EP = ccv.shape
    lens = check_packed_lengths(lengths, M)
    ts = min((int(E) + 7) & ~7, EP)
    c32 = ccv.float()
    a32 = a.float()
    mask = (starts.reshape(-1) > 0).float()
    cv = torch.zeros(lens.numel(), EP, dtype=torch.float32, device=ccv.device)
    attn = torch.empty(M, dtype=torch.float32, device=ccv.device)
    lo = 0
    for b, n in enumerate(lens.tolist()):
        seg = c32[lo:lo + n, :ts].unsqueeze(0)
        at = attention(seg, a32[:ts], mask[lo:lo + n].unsqueeze(0))
        cv[b, :ts] = code_vector(seg, at)[0]
        attn[lo:lo + n] = at[0]
        lo += n
    return cv, cv.to(torch.bfloat16), attn
