"""GPU: imdbn_sample_values / imdbn_lower_bound / imdbn_log_likelihood_is / evaluate_imdbn_bound of imdbn/utils/likelihood.py on the
engine against the numpy twin (tests/bound_oracle.py).

Stack 100-40-20 under the joint RBM (20 + 4) <-> 16 (anneal_cases.PATH), 5 rows x 3 samples.  The seed was chosen on the CPU so that
the twin's smallest Bernoulli margin |p - u| is >= 1e-5 in both modes (asserted first), so the sampled code z must be the twin's
exactly.  The values are held to the sum of the per-layer bounds of test_dbn_bound_gpu.py, (V_l + H_l) * 1e-5 per image layer, plus the
label_loglik bound H_joint * 1e-5 of test_joint_ais_gpu.py, plus 1e-9 |value|."""
import numpy as np
import pytest
import torch

import anneal_cases as Cs
import bound_oracle as B
from likelihood_gpu import DEV, _native, close, device_rbm  # noqa: F401  (the fixture, by name)
from oracle.draws import PhiloxStream

pytestmark = pytest.mark.gpu


class _Stack:
    def __init__(self, layers):
        self.layers = [device_rbm(l) for l in layers]


class _Model:
    """What the likelihood functions read of an iMDBN."""

    def __init__(self, layers, joint, K):
        Dz = joint[0].shape[0] - K
        self.image_idbn, self.joint_rbm, self.num_labels = _Stack(layers), device_rbm(joint, groups=[(Dz, Dz + K)]), K
        self.val_loader = self.dataloader = self.wandb_run = None


@pytest.fixture(scope="module")
def path(_native):
    P = Cs.PATH
    layers, joint = Cs.imdbn(P)
    img, gt = Cs.inputs(P["B"], P["sizes"][0], P["K"], P["in_seed"])
    tol = sum((W.shape[0] + W.shape[1]) * 1e-5 for W, _, _ in layers) + joint[0].shape[1] * 1e-5
    return dict(layers=layers, joint=joint, K=P["K"], S=P["S"], img=img, gt=gt, model=_Model(layers, joint, P["K"]), tol=tol)


@pytest.mark.parametrize("mode", ["entropy", "logq"])
def test_sample_values_and_the_sampled_code_match_the_twin(path, mode):
    from imdbn import engine as E
    from imdbn.utils import likelihood as LK
    p = path
    tj, tm, margin, z = B.imdbn_values(p["layers"], p["joint"], p["K"], p["img"], p["gt"], p["S"], mode, PhiloxStream(Cs.PATH_SEED), 3.25)
    print(f"{mode}: twin margin {margin:.3g}")
    assert margin >= Cs.MARGIN
    img, y = torch.from_numpy(p["img"]).to(DEV), torch.from_numpy(p["gt"]).to(DEV)
    E.manual_seed(9)
    wj, wm = LK.imdbn_sample_values(p["model"], img, y, 3.25, n_samples=p["S"], mode=mode, seed=Cs.PATH_SEED)
    assert E.get_rng().offset == 0                                      # a seed leaves the ambient counter alone
    assert wj.dtype == wm.dtype == torch.float64 and tuple(wj.shape) == tuple(wm.shape) == (Cs.PATH["B"], p["S"])
    # the code the label kernel saw: the last bound_step's h under the same draws
    rng, cur, acc = E.PhiloxRng(Cs.PATH_SEED), img.repeat_interleave(p["S"], 0), None
    for r in p["model"].image_idbn.layers:
        acc, cur = E.get_hip_engine().bound_step(r, cur, rng, acc=acc, mode=mode)
    assert np.array_equal(cur.cpu().numpy(), z)
    for what, got, want in (("joint", wj, tj), ("image", wm, tm)):
        close(got.cpu().numpy(), want, p["tol"] + 1e-9 * np.abs(want), f"{mode} {what}")
    # the two values of a sample differ by the exact log p(y | z) of its code
    jj, mm = E.get_hip_engine().label_loglik(p["model"].joint_rbm, cur, p["K"], y.repeat_interleave(p["S"], 0))
    assert torch.allclose((wj - wm).reshape(-1), jj - mm, rtol=0, atol=1e-9) and (jj <= mm).all()


def test_reductions_and_the_thin_method(path):
    from imdbn.models.imdbn import iMDBN
    from imdbn.utils import likelihood as LK
    p = path
    img, y = torch.from_numpy(p["img"]).to(DEV), torch.nn.functional.one_hot(torch.from_numpy(p["gt"]), p["K"]).float().to(DEV)
    wj, wm = LK.imdbn_sample_values(p["model"], img, y, 3.25, n_samples=4, mode="entropy", seed=2)
    bj, bm = LK.imdbn_lower_bound(p["model"], img, y, 3.25, n_samples=4, seed=2)
    assert torch.equal(bj, wj.mean(1)) and torch.equal(bm, wm.mean(1))
    mj, mm = iMDBN.log_likelihood_bound(p["model"], img, y, 3.25, n_samples=4, seed=2)
    assert torch.equal(mj, bj) and torch.equal(mm, bm)
    lj, lm = LK.imdbn_sample_values(p["model"], img, y, 3.25, n_samples=4, mode="logq", seed=2)
    ij, im = LK.imdbn_log_likelihood_is(p["model"], img, y, 3.25, n_samples=4, seed=2)
    assert torch.allclose(ij, torch.logsumexp(lj, 1) - np.log(4.0), rtol=0, atol=1e-12) and (im >= ij).all()
    assert torch.allclose(im, torch.logsumexp(lm, 1) - np.log(4.0), rtol=0, atol=1e-12)


def test_evaluate_with_a_seed_is_reproducible_and_matches_the_one_shot_mean(path):
    from imdbn import engine as E
    from imdbn.utils import likelihood as LK
    p = path
    img, gt = Cs.inputs(11, Cs.PATH["sizes"][0], p["K"], 31)
    X, Y = torch.from_numpy(img), torch.nn.functional.one_hot(torch.from_numpy(gt), p["K"]).float()
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, Y), batch_size=4)      # 4 + 4 + 3 rows
    E.manual_seed(5)
    kw = dict(loader=loader, n_samples=3, n_chains=16, n_betas=20, seed=4)
    a = LK.evaluate_imdbn_bound(p["model"], **kw)
    b = LK.evaluate_imdbn_bound(p["model"], **kw)
    assert E.get_rng().offset == 0 and a == b
    assert a["n"] == 11 and a["n_samples"] == 3 and a["se"] > 0 and 1 <= a["ess"] <= 16 and np.isfinite(a["log_z_joint"])
    assert a["mean_image_bound"] >= a["mean_joint_bound"] and a["mean_label_logprob"] < 0
    assert a["mean_label_logprob"] == pytest.approx(a["mean_joint_bound"] - a["mean_image_bound"], abs=1e-9)
    # a given log Z: the batches' draws follow each other under the one private source
    c = LK.evaluate_imdbn_bound(p["model"], loader=loader, log_z_joint=2.0, n_samples=3, seed=4)
    rng, tot = E.PhiloxRng(4), 0.0
    for s in (0, 4, 8):
        wj, _ = LK._imdbn_values(p["model"], X[s:s + 4], Y[s:s + 4], 2.0, 3, "entropy", rng)
        tot += float(wj.mean(1).sum())
    assert c["se"] is None and c["mean_joint_bound"] == pytest.approx(tot / 11, rel=1e-12)
