"""Held-out cross-modal retrieval of an ``iMDBN_BiModal``: given a mod1 item, which held-out mod2 item belongs to it?

The score of a pair is the negative free energy of the first joint layer on it, ``S[q, n] = -F([z1_q | z2_n])`` (Srivastava &
Salakhutdinov 2012); the measure is the place of the true partner among all candidates of the split, in both directions.
``evaluate_retrieval`` encodes the whole split once with ``mod{1,2}_dbn.represent`` (codes are ``N x Dz``, small), makes ONE
``HipEngine.pair_scores`` call with ``gt_q = gt_n = arange`` (imdbn_rbm_pair_scores: every pair scored in one sweep, both rank
vectors and the top-k lists from the same score bits, no ``[Q, N]`` matrix in memory) and synchronises with the host once.
No random draws, no parameter is written: evaluating between epochs does not change training.  Under data parallelism each
rank evaluates the loader it is given.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from imdbn import engine as _E
from imdbn.utils.batches import batches, rows_on_device

__all__ = ["retrieval_metrics", "evaluate_retrieval"]


def retrieval_metrics(ranks, ks: Sequence[int] = (1, 5, 10)) -> dict:
    """Metrics of 0-based ``ranks`` (any integer sequence or tensor; CPU): ``recall@k`` = share of rows with rank < k,
    ``median_rank`` and ``mean_rank`` (0-based), ``mrr`` = mean of 1 / (rank + 1), ``n`` and ``skipped``.  Rows with rank -1 (an
    invalid truth) are counted as ``skipped`` and enter nothing; without any other row the metrics are NaN."""
    r = torch.as_tensor(ranks).detach().reshape(-1).cpu().to(torch.int64)
    ok = r[r >= 0].double()
    n = int(ok.numel())
    nan = float("nan")
    out = {f"recall@{int(k)}": float((ok < int(k)).double().mean()) if n else nan for k in ks}
    out["median_rank"] = float(ok.median()) if n else nan          # the lower of the two middle values for an even count
    out["mean_rank"] = float(ok.mean()) if n else nan
    out["mrr"] = float((1.0 / (ok + 1.0)).mean()) if n else nan
    out["n"] = n
    out["skipped"] = int(r.numel()) - n
    return out


@torch.no_grad()
def evaluate_retrieval(model, loader=None, ks: Sequence[int] = (1, 5, 10), topk: int = 0, max_rows: Optional[int] = None) -> Optional[dict]:
    """Retrieval metrics of ``model`` over the pairs of ``loader`` (default ``model.val_loader``; None without one):
    ``{"mod1_to_mod2": retrieval_metrics(rank of pair i among all mod2 items for query mod1_i), "mod2_to_mod1": ...,
    "matched_score_mean": mean of S[i, i], "n": pairs}``; with ``topk > 0`` also ``top_idx`` / ``top_score`` ``[n, topk]`` (numpy, per mod1
    query the best mod2 items).  ``max_rows`` keeps the first rows of the split only."""
    loader = loader if loader is not None else getattr(model, "val_loader", None)
    if loader is None:
        return None
    dev = model.device
    z1s, z2s, n = [], [], 0
    for mod1, mod2 in batches(loader):
        if max_rows is not None and n >= int(max_rows):
            break
        z1s.append(model.mod1_dbn.represent(rows_on_device(mod1, dev)))
        z2s.append(model.mod2_dbn.represent(rows_on_device(mod2, dev)))
        n += z1s[-1].size(0)
    if not z1s:
        return None
    z1, z2 = torch.cat(z1s), torch.cat(z2s)
    if max_rows is not None:
        z1, z2 = z1[:int(max_rows)], z2[:int(max_rows)]
    n = z1.size(0)
    gt = torch.arange(n, dtype=torch.int32, device=z1.device)
    eng = _E.get_engine(model.joint_rbm.W.data)
    o = eng.pair_scores(model.joint_rbm, z1, z2, gt_q=gt, gt_n=gt, k=int(topk))
    flat = torch.cat([o["rank_q"].double(), o["rank_n"].double(), o["score_q"].double()]).cpu()      # the one host sync
    rq, rn, sq = flat[:n].to(torch.int64), flat[n:2 * n].to(torch.int64), flat[2 * n:]
    out = {"mod1_to_mod2": retrieval_metrics(rq, ks), "mod2_to_mod1": retrieval_metrics(rn, ks),
           "matched_score_mean": float(sq.mean()), "n": n}
    if int(topk) > 0:
        out["top_idx"], out["top_score"] = o["top_idx"].cpu().numpy(), o["top_score"].cpu().numpy()
    return out
