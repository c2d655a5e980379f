"""A test double with the one engine call of imdbn.utils.retrieval, ``HipEngine.pair_scores``, on the float64 twin of
tests/retrieval_oracle.py (CPU tensors in, CPU tensors out): the CPU suite runs the host logic of ``evaluate_retrieval`` through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import retrieval_oracle as RO


class RetrievalOracleEngine:
    name = "oracle-test-double-retrieval"

    def __init__(self):
        self.calls = []

    def pair_scores(self, rbm, z1, z2, gt_q=None, gt_n=None, k=0, return_scores=False):
        self.calls.append(("pair_scores", tuple(z1.shape), tuple(z2.shape), gt_q is not None, gt_n is not None, int(k), bool(return_scores)))
        npy = lambda t: t.detach().cpu().numpy()
        S = RO.scores(npy(rbm.W), npy(rbm.hid_bias), npy(rbm.vis_bias), z1.size(1), npy(z1), npy(z2)).astype(np.float32)
        o = {}
        if gt_q is not None:
            r, s = RO.ranks_rows(S, npy(gt_q))
            o["rank_q"], o["score_q"] = torch.from_numpy(r.astype(np.int32)), torch.from_numpy(s)
        if gt_n is not None:
            r, s = RO.ranks_cols(S, npy(gt_n))
            o["rank_n"], o["score_n"] = torch.from_numpy(r.astype(np.int32)), torch.from_numpy(s)
        if k > 0:
            i, s = RO.topk(S, int(k))
            o["top_idx"], o["top_score"] = torch.from_numpy(i), torch.from_numpy(s)
        if return_scores:
            o["scores"] = torch.from_numpy(S)
        return o
