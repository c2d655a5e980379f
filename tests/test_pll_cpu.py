"""CPU-only: the numpy twin of imdbn_rbm_pseudo_loglik (tests/pll_oracle.py) against the enumerated joint, the kernel's
log1p(sigma expm1(.)) form against the twin, the host logic of the pseudo-likelihood functions of imdbn/utils/likelihood.py on a test
double of the engine, and the export's declaration and binding.

The kernel's form, restated here (``kernel_form``): g_i = s_i b_i + sum_j log1p(sigma_j expm1(s_i W_ij)).  With ``fp32=True`` it is
computed the way kernels_pll.hpp computes it: fp32 logits and sigma, fp32 expm1 planes, fp32 factors 1 + sigma E multiplied four at a
time, one fp32 log2 per product, the log2 values of a 128-wide chunk of j added in fp32 and the chunks in double.  Against the twin
(float64 throughout, by the definition) that form stays inside the GPU tolerance H 1e-5 + 1e-9 |value| per site; the largest errors
seen over pll_cases.CASES were 1.6e-6 (scale 0.1, case "rows67", bound 2e-3) and 1.3e-5 (scale 1.0, case "wide": V = 1100, H = 96,
bound 9.6e-4)."""
import os
import re

import numpy as np
import pytest
import torch

import anneal_cases as Cs
import pll_cases as P
import pll_oracle as O
from bound_oracle import host_rbm
from imdbn import engine as E
from imdbn.engine import native
from imdbn.utils import likelihood as LK
from pll_oracle import pll_double  # noqa: F401  (the fixture, by name)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


def kernel_form(W, b, c, v, groups, fp32):
    """-> (site [N, V], total [N]) float64 by the log1p . expm1 form; ``fp32``: with the kernel's fp32 terms (module docstring)."""
    T = F32 if fp32 else F64
    W, b, c, v = np.asarray(W, F32), np.asarray(b, F32), np.asarray(c, F32), np.asarray(v, F32)
    N, V = v.shape
    H = W.shape[1]
    x = (v.astype(T) @ W.astype(T) + c.astype(T)).astype(T)
    sig = (T(1) / (T(1) + np.exp(-x))).astype(T)
    in_group = np.zeros(V, bool)
    for s, e in groups:
        in_group[s:e] = True
    out = np.zeros((N, V), F64)
    if fp32:
        Hp = -(-H // P.CHUNK) * P.CHUNK
        sg = np.zeros((N, Hp), F32)
        sg[:, :H] = sig
        planes = np.zeros((2, V, Hp), F32)
        planes[0, :, :H], planes[1, :, :H] = np.expm1(W), np.expm1(-W)
        for r in range(N):
            E_ = planes[v[r].astype(np.int64), np.arange(V)]                         # [V, Hp]: the plane v_ri selects
            f = (sg[r][None, :] * E_ + F32(1)).astype(F32).reshape(V, Hp // 4, 4)     # (fma: one rounding; here two, no tighter)
            l2 = np.log2(((f[..., 0] * f[..., 1]) * (f[..., 2] * f[..., 3])).astype(F32)).astype(F32).reshape(V, Hp // P.CHUNK, P.CHUNK // 4)
            part = np.zeros(l2.shape[:2], F32)
            for q in range(l2.shape[2]):
                part = (part + l2[..., q]).astype(F32)
            g = np.where(v[r] == 1, -1.0, 1.0) * b.astype(F64) + np.log(2.0) * part.astype(F64).sum(1)
            out[r] = -np.logaddexp(0.0, g)
    else:
        s = 1.0 - 2.0 * v.astype(F64)
        g = s * b.astype(F64) + np.log1p(sig[:, None, :] * np.expm1(s[:, :, None] * W.astype(F64)[None])).sum(2)
        out = -np.logaddexp(0.0, g)
    out[:, in_group] = 0.0
    sd = sig.astype(F64)
    for s, e in groups:
        t = v[:, s:e].argmax(1)
        d = W.astype(F64)[s:e][None, :, :] - W.astype(F64)[s + t][:, None, :]          # [N, K, H]
        g = (b.astype(F64)[s:e][None, :] - b.astype(F64)[s + t][:, None]) + np.log1p(sd[:, None, :] * np.expm1(d)).sum(2)
        mx = g.max(1)
        out[np.arange(N), s + t] = -(mx + np.log(np.exp(g - mx[:, None]).sum(1)))
    return out, out.sum(1)


# ---- 1. the twin against brute force ----------------------------------------------------------------------------------
@pytest.mark.parametrize("V,H,groups", [(10, 6, ()), (12, 5, ((4, 8),))])
def test_twin_equals_the_conditionals_of_the_enumerated_joint(V, H, groups):
    W, b, c, _ = Cs.params(V, H, 900 + V, 1.0)
    W, b, c = W.astype(F64), b.astype(F64), c.astype(F64)
    st = ((np.arange(1 << V)[:, None] >> np.arange(V)[None, :]) & 1).astype(F64)
    for s, e in groups:
        st = st[st[:, s:e].sum(1) == 1]
    log_p = -O.free_energy(W, b, c, st)                                 # unnormalised: a conditional needs no Z
    key = {tuple(r): i for i, r in enumerate(st.astype(np.int64).tolist())}
    rows = Cs.start_rows(7, V, 3, groups).astype(F64)
    site, tot = O.sites(W, b, c, rows, groups)
    in_group = [any(s <= i < e for s, e in groups) for i in range(V)]
    for r, row in enumerate(rows.astype(np.int64).tolist()):
        for i in range(V):
            if in_group[i]:
                continue
            flip = list(row)
            flip[i] = 1 - flip[i]
            a, o = log_p[key[tuple(row)]], log_p[key[tuple(flip)]]
            assert abs((a - np.logaddexp(a, o)) - site[r, i]) <= 1e-10
        for s, e in groups:
            alts = []
            for k in range(s, e):
                alt = list(row)
                alt[s:e] = [0] * (e - s)
                alt[k] = 1
                alts.append(log_p[key[tuple(alt)]])
            t = s + int(np.argmax(row[s:e]))
            want = log_p[key[tuple(row)]] - np.logaddexp.reduce(alts)
            assert abs(want - site[r, t]) <= 1e-10
            assert all(site[r, k] == 0.0 for k in range(s, e) if k != t)
    assert np.allclose(tot, site.sum(1), rtol=0, atol=1e-12)


def test_twin_marks_rows_that_are_not_states():
    c = P.case("two_groups", 1.0)
    v = c["v"].copy()
    v[1, 3] = 0.5
    v[4, 50:60] = 0.0
    v[4, 51] = v[4, 57] = 1.0
    site, tot = O.sites(c["W"], c["b"], c["c"], v, c["groups"])
    clean, clean_tot = O.sites(c["W"], c["b"], c["c"], c["v"], c["groups"])
    assert np.isnan(tot[[1, 4]]).all() and np.isnan(site[[1, 4]]).all()
    keep = np.delete(np.arange(c["N"]), [1, 4])
    assert np.array_equal(site[keep], clean[keep]) and np.array_equal(tot[keep], clean_tot[keep])


def test_twin_marks_a_wide_group_with_two_distant_ones_or_none():
    c = P.case("k256", 1.0)
    (s, e), = c["groups"]
    v = c["v"].copy()
    v[1, s:e] = 0.0
    v[1, s + 3] = v[1, s + 203] = 1.0                                   # more than 64 columns apart
    v[3, s:e] = 0.0                                                     # no one at all
    site, tot = O.sites(c["W"], c["b"], c["c"], v, c["groups"])
    clean, clean_tot = O.sites(c["W"], c["b"], c["c"], c["v"], c["groups"])
    assert np.isnan(tot[[1, 3]]).all() and np.isnan(site[[1, 3]]).all()
    keep = np.delete(np.arange(c["N"]), [1, 3])
    assert np.array_equal(site[keep], clean[keep]) and np.array_equal(tot[keep], clean_tot[keep])
    # the new rows are what they are named for
    assert [e - s for s, e in P.CASES["k65"][3]] == [65] and [e - s for s, e in P.CASES["k256"][3]] == [256] and len(P.CASES["four"][3]) == 4


# ---- 2. the kernel's formula against the twin -------------------------------------------------------------------------
@pytest.mark.parametrize("scale", P.SCALES)
@pytest.mark.parametrize("name", list(P.CASES))
def test_kernel_form_stays_inside_the_gpu_tolerance(name, scale):
    c = P.case(name, scale)
    want, want_tot = O.sites(c["W"], c["b"], c["c"], c["v"], c["groups"])
    exact, exact_tot = kernel_form(c["W"], c["b"], c["c"], c["v"], c["groups"], fp32=False)
    got, got_tot = kernel_form(c["W"], c["b"], c["c"], c["v"], c["groups"], fp32=True)
    e64, e32 = np.abs(exact - want).max(), np.abs(got - want).max()
    print(f"{name} scale {scale}: float64 form {e64:.3g}, fp32-term form {e32:.3g} (site bound {P.site_tol(c, want).min():.3g}), "
          f"total {np.abs(got_tot - want_tot).max():.3g} (bound {P.total_tol(c, want_tot).min():.3g})")
    # in float64 the form is the definition up to rounding
    assert e64 <= 1e-10
    assert (np.abs(got - want) <= P.site_tol(c, want)).all()
    assert (np.abs(got_tot - want_tot) <= P.total_tol(c, want_tot)).all()


def test_identity_behind_the_form_is_exact_in_float64():
    """softplus(x + d) - softplus(x) = log1p(sigmoid(x) expm1(d)), over signs and magnitudes."""
    x, d = np.meshgrid(np.linspace(-30, 30, 61), np.linspace(-8, 8, 65))
    lhs = np.logaddexp(0.0, x + d) - np.logaddexp(0.0, x)
    rhs = np.log1p(np.expm1(d) / (1.0 + np.exp(-x)))
    assert np.abs(lhs - rhs).max() <= 1e-12


# ---- 3. host logic on the test double ---------------------------------------------------------------------------------
class _Run:
    def __init__(self): self.logged = []
    def log(self, d): self.logged.append(dict(d))


def test_function_and_method_return_the_twin(pll_double):
    c = P.case("two_groups", 1.0)
    r = host_rbm(c)
    site, tot = O.sites(c["W"], c["b"], c["c"], c["v"], c["groups"])
    x = torch.from_numpy(c["v"])
    E.manual_seed(5)
    pll = LK.pseudo_log_likelihood(r, x)
    pll2, st = r.pseudo_log_likelihood(x, return_sites=True)
    assert E.get_rng().offset == 0                                      # no draws
    assert pll.dtype == torch.float64 and tuple(pll.shape) == (c["N"],) and st.dtype == torch.float32 and tuple(st.shape) == (c["N"], c["V"])
    assert np.array_equal(pll.numpy(), tot) and torch.equal(pll, pll2) and np.array_equal(st.numpy(), site.astype(F32))

    class _Stack:
        layers = [r, None]
    assert torch.equal(LK.pseudo_log_likelihood(_Stack(), x), pll)       # the bottom layer of a stack


def test_evaluate_over_a_ragged_loader_with_an_invalid_row(pll_double):
    c = P.case("group_end", 0.1)
    r = host_rbm(c)
    r.wandb_run = _Run()
    v = Cs.start_rows(11, c["V"], 12, c["groups"])
    v[5, 2] = 0.5                                                       # one row that is no state
    X = torch.from_numpy(v)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(X, torch.zeros(11)), batch_size=4)      # 4 + 4 + 3 rows
    _, tot = O.sites(c["W"], c["b"], c["c"], v, c["groups"])
    assert np.isnan(tot[5]) and np.isfinite(np.delete(tot, 5)).all()
    res = LK.evaluate_pseudo_likelihood(r, loader=loader)
    assert [n for _, n in pll_double.calls] == [4, 4, 3]
    assert set(res) == {"mean_pll", "sum_pll", "n", "mean_site", "n_invalid"}
    assert res["n"] == 10 and res["n_invalid"] == 1
    assert res["sum_pll"] == pytest.approx(np.delete(tot, 5).sum(), rel=1e-12)
    assert res["mean_pll"] == pytest.approx(np.delete(tot, 5).mean(), rel=1e-12)
    assert res["mean_site"] == pytest.approx(res["mean_pll"] / P.n_sites(c), rel=1e-12) and P.n_sites(c) == 41
    assert r.wandb_run.logged == [{"ll/pll_" + k: res[k] for k in ("mean_pll", "mean_site", "n", "n_invalid")}]
    two = LK.evaluate_pseudo_likelihood(r, loader=loader, max_batches=2)
    assert two["n"] == 7 and two["n_invalid"] == 1 and two["sum_pll"] == pytest.approx(np.delete(tot[:8], 5).sum(), rel=1e-12)
    assert LK.evaluate_pseudo_likelihood(r) is None                       # no loader anywhere
    r.val_loader = loader
    assert LK.evaluate_pseudo_likelihood(r)["n"] == 10                    # the model's own


class _Stack:
    def __init__(self, layers):
        self.layers = [host_rbm(l) for l in layers]


class _Model:
    """What imdbn_pseudo_log_likelihood reads of an iMDBN."""

    def __init__(self, layers, joint, K):
        Dz = joint[0].shape[0] - K
        self.image_idbn, self.joint_rbm, self.num_labels = _Stack(layers), host_rbm(joint, groups=[(Dz, Dz + K)]), K


def test_imdbn_rows_are_code_then_one_hot_label_and_a_seed_leaves_the_ambient_counter_alone(pll_double):
    layers, joint = Cs.imdbn(Cs.TINY)
    K = Cs.TINY["K"]
    m = _Model(layers, joint, K)
    Dz = joint[0].shape[0] - K
    img, gt = Cs.inputs(6, Cs.TINY["sizes"][0], K, 21)
    E.manual_seed(77)
    E.get_rng().advance(3)
    pll, lpy = LK.imdbn_pseudo_log_likelihood(m, torch.from_numpy(img), torch.from_numpy(gt), seed=4)
    assert E.get_rng().offset == 3 and E.get_rng().seed == 77
    # by hand: the code the directed layers draw under the same seed, then the twin on [z | e_y]
    rng, z = E.PhiloxRng(4), torch.from_numpy(img)
    for r in m.image_idbn.layers:
        _, z = pll_double.bound_step(r, z, rng, mode="entropy")
    rows = np.concatenate([z.numpy(), np.eye(K, dtype=F32)[gt]], 1)
    site, tot = O.sites(*joint, rows, [(Dz, Dz + K)])
    assert pll.dtype == lpy.dtype == torch.float64 and tuple(pll.shape) == tuple(lpy.shape) == (6,)
    assert np.array_equal(pll.numpy(), tot)
    assert np.allclose(lpy.numpy(), site[np.arange(6), Dz + gt], rtol=0, atol=1e-6)          # through the fp32 site output
    # the group term is log p(y | z): the log-softmax of -F over the labels
    a = np.stack([-O.free_energy(*joint, np.concatenate([z.numpy(), np.tile(np.eye(K, dtype=F32)[k], (6, 1))], 1)) for k in range(K)], 1)
    assert np.allclose(site[np.arange(6), Dz + gt], a[np.arange(6), gt] - np.logaddexp.reduce(a, 1), rtol=0, atol=1e-12)
    # one-hot labels give the same; seed=None draws from the ambient source: one draw tensor per image layer
    y = torch.nn.functional.one_hot(torch.from_numpy(gt), K).float()
    assert torch.equal(LK.imdbn_pseudo_log_likelihood(m, torch.from_numpy(img), y, seed=4)[0], pll)
    LK.imdbn_pseudo_log_likelihood(m, torch.from_numpy(img), y)
    assert E.get_rng().offset == 3 + len(layers)
    # a label outside [0, K): that row is NaN, no other
    bad = gt.copy()
    bad[2] = K
    p2, l2 = LK.imdbn_pseudo_log_likelihood(m, torch.from_numpy(img), torch.from_numpy(bad), seed=4)
    keep = torch.arange(6) != 2
    assert torch.isnan(p2[2]) and torch.isnan(l2[2]) and torch.equal(p2[keep], pll[keep])


# ---- 4. ABI -----------------------------------------------------------------------------------------------------------
def test_export_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    assert re.search(r"\bint\s+imdbn_rbm_pseudo_loglik\s*\(", src)
    assert "#define IMDBN_ABI_VERSION 4" in src and native.ABI_VERSION == 4
    assert len(native.SIGNATURES["imdbn_rbm_pseudo_loglik"][1]) == 10       # (test_abi_cpu.py holds the library to every declared symbol)
    assert {"pseudo_log_likelihood", "evaluate_pseudo_likelihood", "imdbn_pseudo_log_likelihood"} <= set(LK.__all__)
