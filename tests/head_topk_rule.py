"""The tolerance rule of the K23 tests (test_head_topk_gpu.py states and
derives the bounds; test_predict_fused_gpu.py applies them to a model's
head)."""

import torch

from code2vec_amd.ops import functional as Fn


def n_chain(L, nsplit):
    tps = -(-(-(-L // Fn.SIM_ROW_TILE)) // nsplit)
    n = 4 * -(-tps // 4) + 5
    if nsplit > 1:
        n += -(-nsplit // 256) + 9
    return n


K19_CHAIN = 160


def lse_logit_tol(Z, tol):
    """What the logits' own error can move lse by, per query: with
    p = softmax(Z) and |d_l| <= tol_l, lse(Z + d) - lse(Z) =
    log(sum_l p_l e^(d_l)) lies within +-log(sum_l p_l e^(tol_l)).  Each
    label's tolerance counts by the weight it carries; the value never
    exceeds max_l tol_l over the labels with any weight."""
    p = torch.softmax(Z, dim=1)
    # a masked label (Z = -inf, tol = inf) carries no weight
    terms = torch.where(p > 0, p * torch.exp(tol), torch.zeros_like(p))
    return torch.log(terms.sum(dim=1))


def lse_bound(ref, logit_tol, chain):
    return ((chain + 64) * 2.0 ** -24 + 2.0 ** -17
            + 2.0 ** -22 * ref.abs() + logit_tol)


def check_rule(vals, idx, lse, c, k, chain, tag=""):
    Z, tol = c["Z"], c["tol"]
    nq, L = Z.shape
    assert vals.dtype == torch.float32 and vals.shape == (nq, k)
    assert idx.dtype == torch.int64 and idx.shape == (nq, k)
    assert lse.dtype == torch.float32 and lse.shape == (nq,)
    vals, idx, lse = vals.cpu().double(), idx.cpu(), lse.cpu().double()
    assert bool(((idx >= 0) & (idx < L)).all())
    assert k == 1 or bool(
        (torch.sort(idx, dim=1).values.diff(dim=1) > 0).all())
    err = (vals - Z.gather(1, idx)).abs()
    best = torch.sort(Z, dim=1, descending=True).values[:, :k]
    miss = (vals - best).abs()
    tolmax = tol.max(dim=1).values
    lerr = (lse - c["lse"]).abs()
    lb = lse_bound(c["lse"], lse_logit_tol(Z, tol), chain)
    print(f"head_topk {tag} nq={nq} L={L} k={k}: max |val - fp64| / tol = "
          f"{(err / tol.gather(1, idx)).max():.3f}, max |val - best_j| / "
          f"tol = {(miss / tolmax[:, None]).max():.3f}, max |lse - fp64| = "
          f"{lerr.max():.3e} (bound {lb.min():.3e})")
    assert bool((err <= tol.gather(1, idx)).all())
    d = vals.diff(dim=1)
    assert bool((d <= 0).all())
    assert bool((idx.diff(dim=1)[d == 0] > 0).all())
    assert bool((miss <= tolmax[:, None]).all())
    assert bool((lerr <= lb).all())
    for qi, l in c["plants"]:
        if sum(1 for a, _ in c["plants"] if a == qi) <= k:
            assert l in idx[qi].tolist(), (qi, l)
