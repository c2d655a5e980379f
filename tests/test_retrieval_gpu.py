"""imdbn_rbm_pair_scores / HipEngine.pair_scores / iMDBN_BiModal.evaluate_retrieval on the device against the float64 twin
(tests/retrieval_oracle.py) under the derived tolerance of tests/retrieval_cases.py, and against themselves with no tolerance.

Measured on an MI355X, max |device - twin| as a fraction of tau: see DESIGN §28."""
import ctypes as C

import numpy as np
import pytest
import torch

import retrieval_cases as RC
import retrieval_oracle as RO
from likelihood_gpu import DEV, _native, dev, device_rbm, eng  # noqa: F401  (the fixtures, by name)
from imdbn.engine import native

pytestmark = pytest.mark.gpu
INVALID, WORKSPACE, UNSUPPORTED = -1, -2, -5
POISON_I, POISON_F = -77, 12345.5


def _rbm(W, c, b):
    return device_rbm({"W": W, "b": b, "c": c})


def _padded(a, pad):
    """`a` on the device as a view of rows `pad` floats longer, the padding NaN"""
    t = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device=DEV)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t[:, :a.shape[1]]


class Raw:
    """One raw call of the entry: poisoned outputs, a workspace of `ws_mult` times the minimum, the status returned, not raised."""

    def __init__(self, eng, r, z1, z2, gt_q=None, gt_n=None, k=0, scores=True, lds_pad=0, ws_mult=1.0, D1=None, Q=None, N=None,
                 ld1=None, ld2=None, lds=None, null=(), ws_bytes=None, want_q=True, want_n=True):
        d = eng._desc(r, False)
        Qa, Na = z1.size(0), z2.size(0)
        self.rank_q = torch.full((Qa,), POISON_I, dtype=torch.int32, device=DEV)
        self.rank_n = torch.full((Na,), POISON_I, dtype=torch.int32, device=DEV)
        self.score_q = torch.full((Qa,), POISON_F, device=DEV)
        self.score_n = torch.full((Na,), POISON_F, device=DEV)
        kk = max(k, 1)
        self.top_idx = torch.full((Qa, kk), POISON_I, dtype=torch.int32, device=DEV)
        self.top_score = torch.full((Qa, kk), POISON_F, device=DEV)
        self.full = torch.full((Qa, Na + lds_pad), POISON_F, device=DEV)
        self.scores = self.full[:, :Na]
        o = native.PairOut()
        if gt_q is not None and want_q:
            o.rank_q, o.score_q = self.rank_q.data_ptr(), self.score_q.data_ptr()
        if gt_n is not None and want_n:
            o.rank_n, o.score_n = self.rank_n.data_ptr(), self.score_n.data_ptr()
        if k > 0 and "top" not in null:
            o.top_idx, o.top_score = self.top_idx.data_ptr(), self.top_score.data_ptr()
        if scores:
            o.scores = self.full.data_ptr()
        o.lds = self.full.stride(0) if lds is None else lds
        if "rank_q" in null:
            o.rank_q = self.rank_q.data_ptr()
        if "score_n" in null:
            o.score_n = self.score_n.data_ptr()
        need = int(eng._lib.imdbn_pair_ws_bytes(d.V, d.H, Qa, Na, min(max(k, 0), 64)))
        nbytes = int(need * ws_mult) if ws_bytes is None else ws_bytes
        self.ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
        p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        gq = None if gt_q is None else dev(np.asarray(gt_q, np.int32))
        gn = None if gt_n is None else dev(np.asarray(gt_n, np.int32))
        self.rc = eng._lib.imdbn_rbm_pair_scores(
            C.byref(d), z1.size(1) if D1 is None else D1, p(None if "z1" in null else z1), z1.stride(0) if ld1 is None else ld1,
            Qa if Q is None else Q, p(None if "z2" in null else z2), z2.stride(0) if ld2 is None else ld2, Na if N is None else N,
            p(gq), p(gn), k, None if "out" in null else C.byref(o), p(None if "ws" in null else self.ws), nbytes,
            eng._stream(torch.device(DEV)))
        torch.cuda.synchronize()

    def np(self, name):
        return getattr(self, name).cpu().numpy()

    def untouched(self):
        return all((self.np(n) == v).all() for n, v in (("rank_q", POISON_I), ("rank_n", POISON_I), ("score_q", POISON_F), ("score_n", POISON_F),
                                                        ("top_idx", POISON_I), ("top_score", POISON_F), ("full", POISON_F)))


def _case_call(eng, c, k, **kw):
    r = _rbm(c.W, c.c, c.b)
    return Raw(eng, r, _padded(c.z1, c.pad[0]), _padded(c.z2, c.pad[1]), c.gt_q, c.gt_n, k=k, lds_pad=c.pad[2], **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", RC.case_names())
def test_scores_ranks_and_lists_of_every_case(eng, name):
    c = RC.get_case(name)
    S64, t = c.S64(), c.tau()
    for k in (5, 1, 64):                                       # 64 > N in the cases of 1 and 3 candidates: padding
        o = _case_call(eng, c, k)
        assert o.rc == 0
        S = o.np("scores")
        # 1. within tau of the twin
        err = np.abs(S.astype(np.float64) - S64).max()
        print(f"{name} k={k}: max |device - twin| {err:.3g} = {err / t:.3f} tau (tau {t:.3g})")
        assert err <= t
        assert (o.np("full")[:, c.N:] == POISON_F).all()                    # the padding of the score rows is never written
        # 2. exact self-consistency with the call's own scores
        rq, sq = RO.ranks_rows(S, c.gt_q)
        rn, sn = RO.ranks_cols(S, c.gt_n)
        np.testing.assert_array_equal(o.np("rank_q"), rq); np.testing.assert_array_equal(o.np("rank_n"), rn)
        np.testing.assert_array_equal(_bits(o.np("score_q")), _bits(sq)); np.testing.assert_array_equal(_bits(o.np("score_n")), _bits(sn))
        ti, ts = RO.topk(S, k)
        np.testing.assert_array_equal(o.np("top_idx"), ti); np.testing.assert_array_equal(_bits(o.np("top_score")), _bits(ts))
        # 3. ranks against float64: inside the interval the tolerance allows, for every query and every column
        for got, gt, M in ((o.np("rank_q"), c.gt_q, S64), (o.np("rank_n"), c.gt_n, S64.T)):
            lo, hi = RO.rank_interval(M, gt, t)
            assert ((lo <= got) & (got <= hi)).all()


def test_a_pair_scores_the_same_bits_whatever_surrounds_it(eng):
    c = RC.get_case("h65_65x129")
    r = _rbm(c.W, c.c, c.b)
    z1, z2 = dev(c.z1), dev(c.z2)
    base = Raw(eng, r, z1, z2, c.gt_q, c.gt_n, k=5)
    assert base.rc == 0
    S = _bits(base.np("scores"))
    # other Q, N, k and rows permuted
    g = np.random.default_rng(11)
    pq, pn = g.permutation(c.Q)[:23], g.permutation(c.N)[:70]
    sub = Raw(eng, r, dev(c.z1[pq]), dev(c.z2[pn]), k=64)
    assert sub.rc == 0
    np.testing.assert_array_equal(_bits(sub.np("scores")), S[np.ix_(pq, pn)])
    one = Raw(eng, r, dev(c.z1[7:8]), dev(c.z2[100:101]), gt_q=[0], k=0)
    assert one.rc == 0 and _bits(one.np("scores"))[0, 0] == S[7, 100] and _bits(one.np("score_q"))[0] == S[7, 100]
    # four times the minimum workspace: more chunks, the same everything; and without the score matrix
    for o in (Raw(eng, r, z1, z2, c.gt_q, c.gt_n, k=5, ws_mult=4.0), Raw(eng, r, z1, z2, c.gt_q, c.gt_n, k=5, scores=False)):
        assert o.rc == 0
        for n in ("rank_q", "rank_n", "top_idx"):
            np.testing.assert_array_equal(o.np(n), base.np(n))
        for n in ("score_q", "score_n", "top_score"):
            np.testing.assert_array_equal(_bits(o.np(n)), _bits(base.np(n)))
    np.testing.assert_array_equal(_bits(Raw(eng, r, z1, z2, c.gt_q, c.gt_n, k=5, ws_mult=4.0).np("scores")), S)
    assert (Raw(eng, r, z1, z2, c.gt_q, c.gt_n, k=5, scores=False).np("full") == POISON_F).all()
    # duplicated candidate rows tie exactly and the lower index ranks first (a copy of query 0's best candidate, so both are listed)
    first = int(base.np("top_idx")[0, 0])
    lo_i, hi_i = sorted((first, (first + 37) % c.N))
    z2d = c.z2.copy()
    z2d[lo_i if first == hi_i else hi_i] = z2d[first]
    lo_, hi_ = Raw(eng, r, z1, dev(z2d), np.full(c.Q, lo_i), k=64), Raw(eng, r, z1, dev(z2d), np.full(c.Q, hi_i), k=64)
    assert lo_.rc == 0 and hi_.rc == 0
    Sd = _bits(lo_.np("scores"))
    np.testing.assert_array_equal(Sd[:, lo_i], Sd[:, hi_i])
    np.testing.assert_array_equal(hi_.np("rank_q"), lo_.np("rank_q") + 1)
    ti = lo_.np("top_idx")
    assert ti[0, :2].tolist() == [lo_i, hi_i]
    for q in range(c.Q):
        row = ti[q].tolist()
        assert (lo_i in row) == (hi_i in row) or row[-1] == lo_i
        if hi_i in row:
            assert row.index(hi_i) == row.index(lo_i) + 1


def test_invalid_gt_entries_give_minus_one_and_nan_for_their_row_only(eng):
    c = RC.get_case("h64_64x64_bin")
    r = _rbm(c.W, c.c, c.b)
    z1, z2 = dev(c.z1), dev(c.z2)
    good = Raw(eng, r, z1, z2, c.gt_q, c.gt_n, k=3)
    gq, gn = c.gt_q.copy(), c.gt_n.copy()
    gq[2], gq[40], gn[1], gn[63] = c.N, -7, c.Q + 1000000, -(2 ** 31)
    bad = Raw(eng, r, z1, z2, gq, gn, k=3)
    assert good.rc == 0 and bad.rc == 0
    for rank, score, rows in (("rank_q", "score_q", [2, 40]), ("rank_n", "score_n", [1, 63])):
        assert (bad.np(rank)[rows] == -1).all() and np.isnan(bad.np(score)[rows]).all()
        keep = np.setdiff1d(np.arange(64), rows)
        np.testing.assert_array_equal(bad.np(rank)[keep], good.np(rank)[keep])
        np.testing.assert_array_equal(_bits(bad.np(score)[keep]), _bits(good.np(score)[keep]))
    np.testing.assert_array_equal(bad.np("top_idx"), good.np("top_idx"))
    np.testing.assert_array_equal(_bits(bad.np("scores")), _bits(good.np("scores")))


BAD = {
    "Q=0": (dict(Q=0), INVALID), "N=0": (dict(N=0), INVALID), "D1=0": (dict(D1=0), INVALID), "D1=V": (dict(D1=36), INVALID),
    "ld1": (dict(ld1=19), INVALID), "ld2": (dict(ld2=15), INVALID), "lds": (dict(lds=63), INVALID),
    "k=-1": (dict(k=-1), INVALID), "k=65": (dict(k=65), INVALID),
    "null z1": (dict(null=("z1",)), INVALID), "null z2": (dict(null=("z2",)), INVALID), "null out": (dict(null=("out",)), INVALID),
    "rank_q without gt_q": (dict(gt_q=None, null=("rank_q",)), INVALID), "score_n without gt_n": (dict(gt_n=None, null=("score_n",)), INVALID),
    "k without lists": (dict(k=3, null=("top",)), INVALID),
    "nothing requested": (dict(k=0, scores=False, want_q=False, want_n=False), INVALID),
    "null workspace": (dict(null=("ws",)), WORKSPACE), "short workspace": (dict(ws_mult=0.999), WORKSPACE),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_invalid_arguments_launch_nothing(eng, what):
    c = RC.get_case("h64_64x64_bin")
    kw = dict(gt_q=c.gt_q, gt_n=c.gt_n, k=3)
    kw.update(BAD[what][0])
    o = Raw(eng, _rbm(c.W, c.c, c.b), dev(c.z1), dev(c.z2), **kw)
    assert o.rc == BAD[what][1] and o.untouched()
    buf = C.create_string_buffer(512)
    eng._lib.imdbn_last_error(buf, 512)
    assert b"pair_scores" in buf.value


def test_softmax_groups_are_unsupported(eng):
    c = RC.get_case("h64_64x64_bin")
    r = device_rbm({"W": c.W, "b": c.b, "c": c.c}, groups=[(30, 36)])
    o = Raw(eng, r, dev(c.z1), dev(c.z2), c.gt_q, c.gt_n, k=3)
    assert o.rc == UNSUPPORTED and o.untouched()


@pytest.mark.parametrize("roll", [0, 1])
def test_planted_association(eng, roll):
    from imdbn.utils.retrieval import retrieval_metrics
    p = RC.planted(roll)
    r = _rbm(p["W"], p["c"], p["b"])
    gt = torch.from_numpy(p["gt"]).to(DEV)
    inv = np.empty(48, dtype=np.int32)
    inv[p["gt"]] = np.arange(48)
    o = eng.pair_scores(r, dev(p["z1"]), dev(p["z2"]), gt_q=gt, gt_n=dev(inv), k=1)
    assert not o["rank_q"].cpu().numpy().any() and not o["rank_n"].cpu().numpy().any()
    assert retrieval_metrics(o["rank_q"].cpu())["recall@1"] == 1.0
    np.testing.assert_array_equal(o["top_idx"].cpu().numpy()[:, 0], p["gt"])
    sp = RO.softplus
    np.testing.assert_allclose(o["score_q"].cpu().numpy(), sp(4.0) + 47 * sp(-12.0), rtol=1e-6)


def test_engine_method_rejects_what_it_cannot_run(eng):
    c = RC.get_case("h64_64x64_bin")
    r = _rbm(c.W, c.c, c.b)
    with pytest.raises(native.EngineError):
        eng.pair_scores(r, torch.from_numpy(c.z1), dev(c.z2))                     # not on the device
    with pytest.raises(native.EngineError):
        eng.pair_scores(r, dev(c.z1), dev(c.z2[:, :10]), return_scores=True)      # D1 + D2 != V
    with pytest.raises(native.EngineError):
        eng.pair_scores(r, dev(c.z1), dev(c.z2), gt_q=dev(c.gt_q[:5]))           # gt of the wrong length
    with pytest.raises(native.EngineError):
        eng.pair_scores(r, dev(c.z1), dev(c.z2))                                  # nothing requested
    o = eng.pair_scores(r, dev(c.z1), dev(c.z2), gt_q=dev(c.gt_q), k=2, return_scores=True)
    assert set(o) == {"rank_q", "score_q", "top_idx", "top_score", "scores"}
    np.testing.assert_array_equal(o["rank_q"].cpu().numpy(), RO.ranks_rows(o["scores"].cpu().numpy(), c.gt_q)[0])


def test_model_level_evaluation_leaves_the_model_as_it_was(eng):
    mdl, X1, X2 = RC.bimodal_model(DEV)
    mdl.joint_history = [{"epoch": 0, "mod1_mse": 0.25, "mod2_mse": 0.5, "cd_losses": None}]
    layers = list(mdl.mod1_dbn.layers) + list(mdl.mod2_dbn.layers) + list(mdl.joint_layers)
    state = lambda: {(i, k): getattr(r, k).detach().clone() for i, r in enumerate(layers) for k in ("W", "hid_bias", "vis_bias", "W_m", "hb_m", "vb_m")}
    before = state()
    hist = [dict(h) for h in mdl.joint_history]
    out = mdl.evaluate_retrieval(topk=3)
    n = X1.shape[0]
    assert out["n"] == n and out["top_idx"].shape == (n, 3)
    after = state()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    assert mdl.joint_history == hist
    # the twin on the same codes
    z1 = mdl.mod1_dbn.represent(dev(X1)).cpu().numpy()
    z2 = mdl.mod2_dbn.represent(dev(X2)).cpu().numpy()
    j = mdl.joint_rbm
    W, cb, vb = (t.detach().cpu().numpy() for t in (j.W, j.hid_bias, j.vis_bias))
    D1 = z1.shape[1]
    S64 = RO.scores(W, cb, vb, D1, z1, z2)
    Wa = np.abs(RO.f64(W))
    xmax = float((np.abs(RO.f64(cb)) + (np.abs(RO.f64(z1)) @ Wa[:D1]).max(0) + (np.abs(RO.f64(z2)) @ Wa[D1:]).max(0)).max())
    bdot = float((np.abs(RO.f64(z1)) @ np.abs(RO.f64(vb[:D1]))).max() + (np.abs(RO.f64(z2)) @ np.abs(RO.f64(vb[D1:]))).max())
    t = RC.tau(W.shape[1], D1, z2.shape[1], xmax, bdot)
    gt = np.arange(n)
    for key, M in (("mod1_to_mod2", S64), ("mod2_to_mod1", S64.T)):
        lo, hi = RO.rank_interval(M, gt, t)
        best, worst = RO.metrics(lo), RO.metrics(hi)
        print(f"{key}: {(lo == hi).mean():.3f} of the rows decided; device {out[key]}")
        for m, v in out[key].items():
            a, b = min(best[m], worst[m]), max(best[m], worst[m])
            assert a - 1e-12 <= v <= b + 1e-12, (key, m)                   # a single point wherever lo == hi for every row
    assert out["matched_score_mean"] == pytest.approx(float(np.diag(S64).mean()), abs=t)
