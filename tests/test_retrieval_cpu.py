"""CPU-only: the float64 twin of the pair scores against a brute-force triple loop, ``retrieval_metrics`` on hand-written ranks, the
host logic of ``evaluate_retrieval`` on an engine double, presence of the symbol / method / module, the planted association on the
twin, and -- for every GPU case -- that the case's tolerance leaves the rank of at least 95 % of its queries a single point."""
import os
import re
import types

import numpy as np
import pytest
import torch

import retrieval_cases as RC
import retrieval_oracle as RO
from retrieval_engine_double import RetrievalOracleEngine
from imdbn import engine as E
from imdbn.engine import native
from imdbn.utils import retrieval as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_twin_matches_the_triple_loop():
    g = np.random.default_rng(0)
    D1, D2, H, Q, N = 3, 4, 5, 4, 6
    W, c, b = g.standard_normal((D1 + D2, H)) * 3, g.standard_normal(H), g.standard_normal(D1 + D2)
    z1, z2 = g.random((Q, D1)), (g.random((N, D2)) > 0.5).astype(np.float64)
    np.testing.assert_allclose(RO.scores(W, c, b, D1, z1, z2), RO.scores_loops(W, c, b, D1, z1, z2), rtol=0, atol=1e-11)


def test_twin_rank_rule_ties_and_invalid_entries():
    S = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [np.nan, 1.0, 2.0, 0.0]])
    r, s = RO.ranks_rows(S, [2, 1, 3])
    assert r.tolist() == [1, 1, 2] and s.tolist() == [3.0, 5.0, 0.0]          # the equal score at a lower index ranks first; NaN never
    r, s = RO.ranks_rows(S, [4, -1, 0])
    assert r.tolist() == [-1, -1, 0] and np.isnan(s).all()                    # out of range: -1 / NaN; a NaN reference: nothing beats it
    r, _ = RO.ranks_cols(S, [1, 0, 0, 2])
    assert r.tolist() == [0, 1, 1, 2]
    i, sc = RO.topk(S, 5)
    assert i.tolist() == [[1, 2, 3, 0, -1], [0, 1, 2, 3, -1], [2, 1, 3, -1, -1]]
    assert sc[2].tolist() == [2.0, 1.0, 0.0, -np.inf, -np.inf]
    lo, hi = RO.rank_interval(np.array([[0.0, 1.0, 0.05, -1.0]]), [0], 0.05)
    assert (lo.tolist(), hi.tolist()) == ([1], [2])


def test_retrieval_metrics_on_hand_written_ranks():
    m = RT.retrieval_metrics([0, 0, 4, 9, -1, 2, -1], ks=(1, 5, 10))
    assert m["n"] == 5 and m["skipped"] == 2
    assert m["recall@1"] == pytest.approx(2 / 5) and m["recall@5"] == pytest.approx(4 / 5) and m["recall@10"] == 1.0
    assert m["median_rank"] == 2.0 and m["mean_rank"] == pytest.approx(3.0)
    assert m["mrr"] == pytest.approx((1 + 1 + 1 / 5 + 1 / 10 + 1 / 3) / 5)
    assert RT.retrieval_metrics(torch.tensor([3, 1, 1, 0], dtype=torch.int32))["median_rank"] == 1.0      # even count: the lower middle
    e = RT.retrieval_metrics([-1, -1])
    assert e["n"] == 0 and e["skipped"] == 2 and all(np.isnan(e[k]) for k in ("recall@1", "median_rank", "mean_rank", "mrr"))
    for ranks in ([0, 0, 4, 9, -1, 2, -1], [5], [-1], [7, 7, 7, 0]):
        a, b = RT.retrieval_metrics(ranks), RO.metrics(ranks)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == pytest.approx(b[k], nan_ok=True), k


class _Stack:
    def __init__(self, P):
        self.P = torch.from_numpy(P)
        self.calls = 0

    def represent(self, x):
        self.calls += 1
        return torch.sigmoid(x.float() @ self.P)


def _stub_model(n=23, with_val=True):
    g = np.random.default_rng(5)
    X1, X2 = g.random((n, 6)).astype(np.float32), g.random((n, 5)).astype(np.float32)
    dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(X1), torch.from_numpy(X2)), batch_size=8, shuffle=False)
    mdl = types.SimpleNamespace(device=torch.device("cpu"), val_loader=dl if with_val else None,
                                mod1_dbn=_Stack(g.standard_normal((6, 4)).astype(np.float32)),
                                mod2_dbn=_Stack(g.standard_normal((5, 3)).astype(np.float32)),
                                joint_rbm=types.SimpleNamespace(W=torch.from_numpy((g.standard_normal((7, 9)) * 2).astype(np.float32)),
                                                                hid_bias=torch.from_numpy(g.standard_normal(9).astype(np.float32)),
                                                                vis_bias=torch.from_numpy(g.standard_normal(7).astype(np.float32))))
    return mdl, dl, X1, X2


@pytest.fixture
def double():
    eng = RetrievalOracleEngine()
    E.set_engine_for_testing(eng)
    yield eng
    E.set_engine_for_testing(None)


def test_evaluate_retrieval_host_logic(double):
    mdl, dl, X1, X2 = _stub_model()
    out = RT.evaluate_retrieval(mdl, topk=4)                                  # loader falls back to val_loader
    assert double.calls == [("pair_scores", (23, 4), (23, 3), True, True, 4, False)]          # ONE engine call for the whole split
    z1, z2 = mdl.mod1_dbn.represent(torch.from_numpy(X1)).numpy(), mdl.mod2_dbn.represent(torch.from_numpy(X2)).numpy()
    r = mdl.joint_rbm
    S = RO.scores(r.W.numpy(), r.hid_bias.numpy(), r.vis_bias.numpy(), 4, z1, z2).astype(np.float32)
    gt = np.arange(23)
    assert out["n"] == 23
    close = lambda d: pytest.approx(d, rel=1e-12)          # the two means add in different orders
    assert out["mod1_to_mod2"] == close(RO.metrics(RO.ranks_rows(S, gt)[0])) and out["mod2_to_mod1"] == close(RO.metrics(RO.ranks_cols(S, gt)[0]))
    assert out["matched_score_mean"] == pytest.approx(float(np.diag(S).astype(np.float64).mean()))
    np.testing.assert_array_equal(out["top_idx"], RO.topk(S, 4)[0])
    assert out["top_score"].shape == (23, 4)
    # max_rows: the first rows only, still one call; an explicit loader wins over val_loader
    double.calls.clear()
    out = RT.evaluate_retrieval(mdl, loader=dl, max_rows=10, ks=(1, 3))
    assert double.calls == [("pair_scores", (10, 4), (10, 3), True, True, 0, False)]
    assert out["n"] == 10 and "top_idx" not in out and set(out["mod1_to_mod2"]) >= {"recall@1", "recall@3"}
    assert out["mod1_to_mod2"] == close(RO.metrics(RO.ranks_rows(S[:10, :10], gt[:10])[0], ks=(1, 3)))
    mdl2, dl2, _, _ = _stub_model(with_val=False)
    assert RT.evaluate_retrieval(mdl2) is None
    assert RT.evaluate_retrieval(mdl2, loader=dl2)["n"] == 23


def test_symbol_method_and_module_are_present():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bimdbn_rbm_pair_scores\s*\(", src) and re.search(r"\bimdbn_pair_ws_bytes\s*\(", src)
    assert "imdbn_rbm_pair_scores" in native.SIGNATURES and "imdbn_pair_ws_bytes" in native.SIGNATURES
    lib = native.lib()
    assert hasattr(lib, "imdbn_rbm_pair_scores")
    import ctypes as C
    assert C.sizeof(native.PairOut) == 8 * 8
    from imdbn.engine.hip_engine import HipEngine
    from imdbn.models.imdbn_bimodal import iMDBN_BiModal
    assert callable(HipEngine.pair_scores) and callable(iMDBN_BiModal.evaluate_retrieval)
    assert set(RT.__all__) == {"retrieval_metrics", "evaluate_retrieval"}
    import imdbn.utils
    assert imdbn.utils.retrieval is RT
    # the size helper: 0 outside the limits, grows with k, and more than the scratch of either propagation
    ws = lib.imdbn_pair_ws_bytes
    assert ws(36, 24, 64, 64, 0) > 0 and ws(36, 24, 64, 64, 5) > ws(36, 24, 64, 64, 0)
    assert ws(1, 24, 64, 64, 0) == 0 and ws(36, 24, 0, 64, 0) == 0 and ws(36, 24, 64, 64, 65) == 0 and ws(36, 24, 64, 64, -1) == 0
    assert ws(36, 24, 64, 130, 0) >= max(lib.imdbn_ws_bytes(v, 24, 130) for v in (1, 20, 35))


@pytest.mark.parametrize("roll", [0, 1])
def test_planted_association_on_the_twin(roll):
    p = RC.planted(roll)
    S = RO.scores(p["W"], p["c"], p["b"], p["D1"], p["z1"], p["z2"])
    sp = RO.softplus
    hit, miss = sp(4.0) + 47 * sp(-12.0), 2 * sp(-4.0) + 46 * sp(-12.0)
    gt = p["gt"]
    np.testing.assert_allclose(S[np.arange(48), gt], hit, rtol=1e-14)
    mask = np.ones_like(S, dtype=bool)
    mask[np.arange(48), gt] = False
    np.testing.assert_allclose(S[mask], miss, rtol=1e-14)
    rq, _ = RO.ranks_rows(S, gt)
    inv = np.empty(48, dtype=np.int64)
    inv[gt] = np.arange(48)
    rn, _ = RO.ranks_cols(S, inv)
    assert not rq.any() and not rn.any()
    assert RO.metrics(rq)["recall@1"] == 1.0
    np.testing.assert_array_equal(RO.topk(S, 1)[0][:, 0], gt)


@pytest.mark.parametrize("name", RC.case_names())
def test_gpu_cases_are_decided_by_their_tolerance(name):
    """On the twin alone: under the case's tau at least 95 % of the queries (and of the columns) have lo == hi.  The logits of every
    case of some size reach beyond +-30, and the tolerance stays far below the spread of the scores."""
    c = RC.get_case(name)
    S, t = c.S64(), c.tau()
    assert np.isfinite(S).all() and 0 < t < 0.02
    x = c.x()
    assert 30 < np.abs(x).max() < 80 and c.xmax() >= np.abs(x).max() - 1e-4
    if x.size >= 1000:
        assert x.max() > 30 and x.min() < -30
    for gt, M in ((c.gt_q, S), (c.gt_n, S.T)):
        lo, hi = RO.rank_interval(M, gt, t)
        assert (lo == hi).mean() >= 0.95, f"{name}: {(lo == hi).mean():.3f} of the rows are decided"
