"""GPU: imdbn_rbm_pseudo_loglik and the pseudo-likelihood functions of imdbn/utils/likelihood.py against the float64 numpy twin
(tests/pll_oracle.py: the definition, from free energies of whole states) fed the same fp32 parameters.

Tolerance, from the project's convention for the label-side kernel (a sum of H softplus terms on the same logits): every site term
within H 1e-5 + 1e-9 |value| of the twin, every row total within n_sites H 1e-5 + 1e-9 |value|.  Largest errors seen per case
(site / total, scale 0.1 | scale 1.0) are printed by the first test; DESIGN §21 holds the maxima."""
import ctypes as C

import numpy as np
import pytest
import torch

import anneal_cases as Cs
import pll_cases as P
import pll_oracle as O
from likelihood_gpu import DEV, _native, close, dev, device_rbm, eng, twin  # noqa: F401  (the fixtures, by name)

pytestmark = pytest.mark.gpu

ALL = [(n, s) for n in P.CASES for s in P.SCALES]


def _twin(name, scale):
    """(case, site [N, V], total [N]) of the twin, computed once."""
    def run():
        c = P.case(name, scale)
        return (c,) + O.sites(c["W"], c["b"], c["c"], c["v"], c["groups"])
    return twin(("pll", name, scale), run)


def _run(eng, c, v=None, r=None):
    pll, site = eng.pseudo_loglik(device_rbm(c) if r is None else r, dev(c["v"]) if v is None else v, return_sites=True)
    torch.cuda.synchronize()
    return pll, site


# ---- 1. against the twin ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", ALL)
def test_sites_and_totals_match_the_twin(eng, name, scale):
    c, want, want_tot = _twin(name, scale)
    pll, site = _run(eng, c)
    assert pll.dtype == torch.float64 and tuple(pll.shape) == (c["N"],) and site.dtype == torch.float32 and tuple(site.shape) == (c["N"], c["V"])
    got, got_tot = site.cpu().numpy().astype(np.float64), pll.cpu().numpy()
    close(got, want, P.site_tol(c, want), f"{name} scale {scale}: sites")
    close(got_tot, want_tot, P.total_tol(c, want_tot), f"{name} scale {scale}: totals")
    assert np.allclose(got.sum(1), got_tot, rtol=1e-6, atol=0)          # a row of out_site sums to out_pll
    for s, e in c["groups"]:
        t = s + c["v"][:, s:e].argmax(1)
        rest = np.ones((c["N"], e - s), bool)
        rest[np.arange(c["N"]), t - s] = False
        assert (got[:, s:e][rest] == 0.0).all() and (got[np.arange(c["N"]), t] < 0.0).all()
    assert torch.equal(eng.pseudo_loglik(device_rbm(c), dev(c["v"])), pll)      # without the site output: the same totals


# ---- 2. the engine's own free energy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,scale", ALL)
def test_site_terms_are_free_energy_differences_of_the_engine(eng, name, scale):
    c = P.case(name, scale)
    r = device_rbm(c)
    _, site = _run(eng, c, r=r)
    cols = P.check_columns(c)
    assert len(cols) == 8 and cols[0] == min(cols) and {P.TILE_COLS - 1, P.TILE_COLS} <= set(cols)
    flipped = np.repeat(c["v"], len(cols), 0)                          # row n's flips: the rows 8 n .. 8 n + 7
    for k, i in enumerate(cols):
        flipped[k::len(cols), i] = 1.0 - flipped[k::len(cols), i]
    F0 = eng.free_energy(r, dev(c["v"])).double().cpu().numpy()
    F1 = eng.free_energy(r, dev(flipped)).double().cpu().numpy().reshape(c["N"], len(cols))
    want = -np.logaddexp(0.0, F0[:, None] - F1)
    tol = 2e-5 * np.maximum(1.0, np.abs(F0))[:, None]                  # the project's free-energy margin
    close(site.cpu().numpy()[:, cols].astype(np.float64), want, tol, f"{name} scale {scale}: sites vs free_energy")


# ---- 3. batch independence and determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rows67", "wide", "two_groups"])
def test_a_row_gives_the_same_bits_alone_and_in_the_batch(eng, name):
    c = P.case(name, 1.0)
    r = device_rbm(c)
    x = dev(c["v"])
    pll, site = _run(eng, c, r=r)
    again, site2 = _run(eng, c, r=r)
    assert torch.equal(pll, again) and torch.equal(site, site2)
    for n in sorted({0, c["N"] // 2, c["N"] - 1}):
        p1, s1 = eng.pseudo_loglik(r, x[n:n + 1], return_sites=True)
        assert torch.equal(p1[0], pll[n]) and torch.equal(s1[0], site[n]), n


# ---- 4. invalid rows --------------------------------------------------------------------------------------------------
def test_rows_that_are_not_states_are_nan_and_only_they(eng):
    c = P.case("two_groups", 1.0)
    r = device_rbm(c)
    pll, site = _run(eng, c, r=r)
    v = c["v"].copy()
    v[1, 3] = 0.5
    v[4, 50:60] = 0.0
    v[4, 51] = v[4, 57] = 1.0
    p2, s2 = _run(eng, c, v=dev(v), r=r)
    keep = torch.tensor([n not in (1, 4) for n in range(c["N"])], device=DEV)
    assert torch.isnan(p2[~keep]).all() and torch.isnan(s2[~keep]).all()
    assert torch.equal(p2[keep], pll[keep]) and torch.equal(s2[keep], site[keep])
    c = P.case("odd", 0.1)                                              # a Bernoulli-only RBM: the 0/1 check alone
    v = c["v"].copy()
    v[2, 69] = 2.0
    p3, s3 = _run(eng, c, v=dev(v))
    assert torch.isnan(p3[2]) and torch.isnan(s3[2]).all() and torch.isfinite(p3[[0, 1, 3, 4]]).all()


def test_a_wide_group_with_two_distant_ones_or_none_is_nan(eng):
    """K = 256: the ones of a group are counted by 64 lanes in four trips -- two ones more than 64 columns apart fall to different
    trips (and, 200 apart, to different lanes); a group with no one at all must not pass as a state either."""
    c = P.case("k256", 1.0)
    (s, e), = c["groups"]
    r = device_rbm(c)
    pll, site = _run(eng, c, r=r)
    v = c["v"].copy()
    v[1, s:e] = 0.0
    v[1, s + 3] = v[1, s + 203] = 1.0
    v[3, s:e] = 0.0
    p2, s2 = _run(eng, c, v=dev(v), r=r)
    keep = torch.tensor([n not in (1, 3) for n in range(c["N"])], device=DEV)
    assert torch.isnan(p2[~keep]).all() and torch.isnan(s2[~keep]).all()
    assert torch.equal(p2[keep], pll[keep]) and torch.equal(s2[keep], site[keep])


# ---- 5. errors --------------------------------------------------------------------------------------------------------
def _raw(eng, r, x, N=None, ldv=None, lds=None, with_site=True, null_pll=False):
    """The export called directly on sentinel-filled outputs -> (EngineError message or None, out_pll, out_site)."""
    from imdbn.engine import native as Nt
    d = eng._desc(r, False)
    N = x.size(0) if N is None else N
    pll = torch.full((max(N, 1),), -7.25, dtype=torch.float64, device=DEV)
    site = torch.full((max(N, 1), d.V), -7.25, device=DEV)
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(N, 1))
    msg = None
    try:
        eng._call("imdbn_rbm_pseudo_loglik", C.byref(d), C.c_void_p(x.data_ptr()), x.stride(0) if ldv is None else ldv, N,
                  None if null_pll else C.c_void_p(pll.data_ptr()), C.c_void_p(site.data_ptr()) if with_site else None,
                  d.V if lds is None else lds, ws, nbytes, stream)
    except Nt.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, pll, site


@pytest.mark.parametrize("what", ["N0", "ldv", "lds", "null_pll"])
def test_invalid_arguments_launch_nothing(eng, what):
    c = P.case("odd", 0.1)
    r = device_rbm(c)
    x = dev(c["v"])
    msg, pll, site = _raw(eng, r, x, N=0 if what == "N0" else None, ldv=c["V"] - 1 if what == "ldv" else None,
                          lds=c["V"] - 2 if what == "lds" else None, null_pll=what == "null_pll")
    print(what, "->", msg)
    assert msg is not None and "rc=-1)" in msg
    assert {"N0": "N = 0", "ldv": f"ldv {c['V'] - 1}", "lds": f"lds {c['V'] - 2}", "null_pll": "out_pll"}[what] in msg
    assert (pll == -7.25).all() and (site == -7.25).all()
    # lds is only looked at when sites are asked for, and the same workspace still serves a good call
    msg, pll, site = _raw(eng, r, x, lds=0 if what == "lds" else None, with_site=what != "lds")
    assert msg is None and torch.isfinite(pll).all() and not (pll == -7.25).any()
    from imdbn import engine as E
    with pytest.raises(E.EngineError):
        eng.pseudo_loglik(r, x[:, :7])


# ---- 6. strided input -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "wide", "group_end"])
def test_strided_rows_equal_contiguous_rows_and_padding_is_never_read(eng, name):
    c = P.case(name, 1.0)
    r = device_rbm(c)
    pll, site = _run(eng, c, r=r)
    big = torch.full((c["N"] + 3, c["V"] + 5), float("nan"), device=DEV)          # NaN beyond V and beyond N
    big[:c["N"], :c["V"]] = dev(c["v"])
    x = big[:c["N"], :c["V"]]
    assert x.stride(0) == c["V"] + 5 and not x.is_contiguous()
    p2, s2 = _run(eng, c, v=x, r=r)
    assert torch.equal(p2, pll) and torch.equal(s2, site)
    assert torch.isnan(big[c["N"]:]).all() and torch.isnan(big[:, c["V"]:]).all()          # and only read


# ---- 7. the Python functions ------------------------------------------------------------------------------------------
class _Stack:
    def __init__(self, layers):
        self.layers = [device_rbm(l) for l in layers]


class _Model:
    """What the likelihood functions read of an iMDBN."""

    def __init__(self, layers, joint, K):
        Dz = joint[0].shape[0] - K
        self.image_idbn, self.joint_rbm, self.num_labels = _Stack(layers), device_rbm(joint, groups=[(Dz, Dz + K)]), K
        self.val_loader = self.dataloader = self.wandb_run = None


def test_imdbn_label_term_is_label_logliks_joint_minus_marginal(eng):
    from imdbn import engine as E
    from imdbn.utils import likelihood as LK
    Pth = Cs.PATH
    layers, joint = Cs.imdbn(Pth)
    K, HJ = Pth["K"], joint[0].shape[1]
    m = _Model(layers, joint, K)
    img, gt = Cs.inputs(Pth["B"], Pth["sizes"][0], K, Pth["in_seed"])
    X, Y = torch.from_numpy(img).to(DEV), torch.from_numpy(gt).to(DEV)
    E.manual_seed(9)
    pll, lpy = LK.imdbn_pseudo_log_likelihood(m, X, Y, seed=Cs.PATH_SEED)
    assert E.get_rng().offset == 0                                      # a seed leaves the ambient counter alone
    assert pll.dtype == lpy.dtype == torch.float64 and tuple(pll.shape) == tuple(lpy.shape) == (Pth["B"],)
    # the same sampled z: the directed layers under the same seed
    rng, z = E.PhiloxRng(Cs.PATH_SEED), X
    for r in m.image_idbn.layers:
        _, z = eng.bound_step(r, z, rng, mode="entropy")
    j, mg = eng.label_loglik(m.joint_rbm, z, K, Y.to(torch.int32))
    want = (j - mg).cpu().numpy()
    close(lpy.cpu().numpy(), want, 2 * HJ * 1e-5, "log p(y | z): group site vs label_loglik")
    rows = np.concatenate([z.cpu().numpy(), np.eye(K, dtype=np.float32)[gt]], 1)
    _, tot = O.sites(*joint, rows, [(rows.shape[1] - K, rows.shape[1])])
    close(pll.cpu().numpy(), tot, (rows.shape[1] - K + 1) * HJ * 1e-5 + 1e-9 * np.abs(tot), "joint PLL vs twin")


def test_evaluate_over_a_ragged_loader_on_the_device(eng):
    from imdbn.utils import likelihood as LK
    c, _, _ = _twin("group_end", 0.1)
    r = device_rbm(c)
    v = Cs.start_rows(11, c["V"], 12, c["groups"])
    v[5, 2] = 0.5
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.from_numpy(v), torch.zeros(11)), batch_size=4)
    _, tot = O.sites(c["W"], c["b"], c["c"], v, c["groups"])
    res = LK.evaluate_pseudo_likelihood(r, loader=loader)
    assert res["n"] == 10 and res["n_invalid"] == 1
    good = np.delete(tot, 5)
    assert abs(res["sum_pll"] - good.sum()) <= 10 * P.total_tol(c, good).max()
    assert res["mean_site"] == pytest.approx(res["sum_pll"] / 10 / P.n_sites(c), rel=1e-12)
