"""GPU: imdbn_rbm_ais_groups / HipEngine.ais_groups and imdbn_rbm_label_loglik / HipEngine.label_loglik against the numpy twins
(tests/anneal_oracle.py, tests/bound_oracle.py) and the enumerated partition function.

AIS parity: every case's seed was chosen on the CPU so that the twin's smallest Bernoulli margin |p - u| outside the softmax groups AND
its smallest categorical-CDF margin are >= 1e-5 (asserted first; test_joint_ais_cpu.py holds the same), so every decision of the device
must be the twin's: the final states are compared exactly.  logw is held to H * 1e-5 + 1e-9 |logw|, the bound of test_ais_gpu.py: the
increment's formula is unchanged, and the visible term is exact on a 0/1 state.
label_loglik: joint and marg are held to H * 1e-5 + 1e-9 |value|: an error delta in a logit base_j + W[Dz+k][j] moves
softplus by sigmoid(.) delta <= delta per hidden unit, 1e-5 is the logit agreement of the propagations, and logsumexp is
1-Lipschitz in the largest error of its arguments."""
import ctypes as C

import numpy as np
import pytest
import torch

import anneal_cases as Cs
import anneal_oracle as A
import bound_oracle as B
from likelihood_gpu import DEV, _native, base_bias, close, device_rbm, eng  # noqa: F401  (the fixtures, by name)
from oracle.draws import DrawStream, PhiloxStream

pytestmark = pytest.mark.gpu


def _close(got, want, H, what):
    close(got, want, H * 1e-5 + 1e-9 * np.abs(want), what)


# ---- 1. AIS parity with the twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(Cs.GROUPS))
def test_parity_with_the_twin(eng, name):
    from imdbn import engine as E
    from imdbn.engine import rng as R
    c = Cs.case(Cs.GROUPS, name)
    logw, vK, margin, cat_margin = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(c["seed"]), c["groups"])
    print(f"{name}: twin margins {margin:.3g} (Bernoulli), {cat_margin:.3g} (categorical)")
    assert margin >= Cs.MARGIN and cat_margin >= Cs.MARGIN
    r = device_rbm(c)
    rng = E.PhiloxRng(c["seed"])
    lw, v = eng.ais_groups(r, c["betas"], c["M"], rng, base_vis_bias=base_bias(c), return_state=True)
    torch.cuda.synchronize()
    G = len(c["groups"])
    assert lw.dtype == torch.float64 and tuple(lw.shape) == (c["M"],) and tuple(v.shape) == (c["M"], c["V"])
    assert rng.offset == (c["K"] - 1) * (2 + G) + 1 + G == len(R.sched_ais_groups(c["V"], c["H"], c["groups"], c["K"]))
    bad = np.nonzero(v.cpu().numpy() != vK)
    assert bad[0].size == 0, f"{name}: v_K differs at {list(zip(*bad))[:6]}"
    _close(lw.cpu().numpy(), logw, c["H"], name)
    route = eng.last_route()
    if name == "wide":
        assert route["up"] not in (None, "fused"), route              # a split-K route, not the fused short-K kernel
    if G > 0 and c["K"] > 1:
        assert route["finish_groups"], route
    if G == 0:                                                          # n_groups = 0: imdbn_rbm_ais bit for bit
        lw0, v0 = eng.ais(r, c["betas"], c["M"], E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c), return_state=True)
        assert torch.equal(lw, lw0) and torch.equal(v, v0)
    else:                                                               # deterministic, and the Philox key is the row
        lw2 = eng.ais_groups(r, c["betas"], c["M"], E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c))
        assert torch.equal(lw, lw2)
        if c["M"] <= 64:
            few = eng.ais_groups(r, c["betas"], min(3, c["M"]), E.PhiloxRng(c["seed"]), base_vis_bias=base_bias(c))
            assert torch.equal(few, lw[:few.numel()])


def test_estimate_against_the_enumerated_log_z(eng):
    from imdbn.utils import likelihood as LK
    c = Cs.groups_truth(True)
    exact = A.exact_log_z(c["W"], c["b"], c["c"], c["groups"])
    t_logw = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], c["M"], PhiloxStream(c["seed"]), c["groups"])[0]
    _, t_se, _ = A.weight_stats(t_logw)
    est = LK.estimate_joint_log_partition(device_rbm(c), n_chains=c["M"], betas=c["betas"], base_vis_bias=base_bias(c), seed=c["seed"])
    print(f"device log Z {est['log_z']:.4f}, exact {exact:.4f}, error {(est['log_z'] - exact) / t_se:+.2f} twin se; se {est['se']:.4f} (twin {t_se:.4f})")
    assert abs(est["log_z"] - exact) <= 5 * t_se and est["se"] <= 2 * t_se          # the rule of test_ais_gpu.py
    assert est["log_z_base"] == pytest.approx(A.log_z_base(c["V"], c["H"], c["bA"], c["groups"]), rel=1e-6)


# ---- 2. replay ----------------------------------------------------------------------------------------------------------
def test_replay_tape_with_cat_tape_matches_philox_fed_the_same_decisions(eng):
    """A replay tape (uniforms AND categorical indices) against the twin fed the same tape."""
    from imdbn import engine as E
    c = Cs.case(Cs.GROUPS, "two")
    M, G = 9, len(c["groups"])
    g = np.random.Generator(np.random.PCG64(5))
    cats = [g.integers(0, e - s, M) for _ in range(c["K"]) for s, e in c["groups"]]
    want, vK, margin, _ = A.ais_logw(c["W"], c["b"], c["c"], c["bA"], c["betas"], M, DrawStream(11, cat=cats), c["groups"])
    assert margin >= Cs.MARGIN
    src = DrawStream(11, cat=cats)
    lw, v = eng.ais_groups(device_rbm(c), c["betas"], M, E.ReplayRng(src), base_vis_bias=base_bias(c), return_state=True)
    assert src.exhausted_cat() and len(cats) == c["K"] * G
    vd = v.cpu().numpy()
    assert np.array_equal(vd, vK)
    for q, (s, e) in enumerate(c["groups"]):                           # the last transition's categories are the tape's
        assert np.array_equal(vd[:, s:e].argmax(1), cats[(c["K"] - 1) * G + q])
    _close(lw.cpu().numpy(), want, c["H"], "replay")


# ---- 3. errors ----------------------------------------------------------------------------------------------------------
def _raw(eng, r, betas, M, short=0, n_groups=None):
    """The export called directly on a sentinel-filled logw -> (EngineError message or None, logw)."""
    from imdbn.engine import native as N, rng as R
    from imdbn import engine as E
    d = N.RbmDesc.from_buffer_copy(eng._desc(r, False))          # a private copy: the cached descriptor stays as it is
    if n_groups is not None:
        d.n_groups = n_groups
    K = len(betas) - 1
    arr = (C.c_float * len(betas))(*[float(x) for x in betas])
    logw = torch.full((max(M, 1),), -7.25, dtype=torch.float64, device=DEV)
    nr, _ = eng._rng(E.PhiloxRng(1), R.sched_ais_groups(d.V, d.H, eng._groups(r), max(K, 1)), max(M, 1), torch.device(DEV))
    ws, nbytes, stream = eng._ws_tail(torch.device(DEV), d.V, d.H, max(M, 1))
    msg = None
    try:
        eng._call("imdbn_rbm_ais_groups", C.byref(d), M, K, arr, None, C.byref(nr), C.c_void_p(logw.data_ptr()), None, d.V, ws, nbytes - short, stream)
    except N.EngineError as e:
        msg = str(e)
    torch.cuda.synchronize()
    return msg, logw


@pytest.mark.parametrize("what,code", [("K0", -1), ("flat", -1), ("first", -1), ("last", -1), ("M0", -1), ("short", -2), ("groups5", -5)])
def test_invalid_arguments_launch_nothing(eng, what, code):
    c = Cs.case(Cs.GROUPS, "odd")
    r = device_rbm(c)
    betas = {"flat": [0, 0.5, 0.5, 1], "first": [0.1, 0.5, 1], "last": [0, 0.5, 0.9], "K0": [0.0]}.get(what, [0, 0.25, 0.5, 1])
    msg, logw = _raw(eng, r, betas, 0 if what == "M0" else 5, short=1 if what == "short" else 0, n_groups=5 if what == "groups5" else None)
    print(what, "->", msg)
    assert msg is not None and f"rc={code})" in msg
    assert (logw == -7.25).all()
    if what in ("flat", "first", "last"):
        assert "0.5" in msg or "0.1" in msg or "0.9" in msg          # the offending value is named
    if what == "groups5":
        assert "5" in msg
    # the same workspace still serves a good call
    msg, logw = _raw(eng, r, [0, 0.25, 0.5, 1], 5)
    assert msg is None and torch.isfinite(logw).all() and not (logw == -7.25).any()


def test_the_binary_call_still_refuses_groups_and_parameters_are_untouched(eng):
    from imdbn import engine as E
    c = Cs.case(Cs.GROUPS, "odd")
    r = device_rbm(c)
    W0, b0, c0 = r.W.data.clone(), r.vis_bias.data.clone(), r.hid_bias.data.clone()
    with pytest.raises(E.EngineError):
        eng.ais(r, c["betas"], 5, E.PhiloxRng(1))
    eng.ais_groups(r, c["betas"], 5, E.PhiloxRng(1), base_vis_bias=base_bias(c))
    assert torch.equal(r.W.data, W0) and torch.equal(r.vis_bias.data, b0) and torch.equal(r.hid_bias.data, c0)


# ---- 4. label_loglik ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,real,pad", [("small", 5, False, 0), ("small", 70, True, 3), ("paper", 5, True, 0), ("paper", 70, False, 12),
                                             ("slots", 5, False, 0), ("slots", 70, True, 3)])
def test_label_loglik_against_the_twin(eng, name, N, real, pad):
    c = Cs.label_case(name, N, real)
    Dz, K, H = c["Dz"], c["K"], c["H"]
    gt = c["gt"].copy()
    gt[1] = -1                                                            # one label out of range: NaN joint, finite marg, no fault
    if N > 64:
        gt[65] = K
    wj, wm = B.label_loglik(c["W"], c["b"], c["c"], c["z"], Dz, K, gt)
    r = device_rbm(c, groups=[(Dz, Dz + K)])
    zbuf = torch.full((N, Dz + pad), 7.0, device=DEV)                     # ldz > Dz: the columns behind the code are not read
    zbuf[:, :Dz] = torch.from_numpy(c["z"]).to(DEV)
    z = zbuf[:, :Dz]
    gtd = torch.from_numpy(gt).to(DEV)
    j, m = eng.label_loglik(r, z, K, gtd)
    torch.cuda.synchronize()
    assert j.dtype == m.dtype == torch.float64 and tuple(j.shape) == tuple(m.shape) == (N,)
    jn, mn = j.cpu().numpy(), m.cpu().numpy()
    bad = (gt < 0) | (gt >= K)
    assert np.isnan(jn[bad]).all() and np.isfinite(jn[~bad]).all() and np.isfinite(mn).all()
    _close(jn[~bad], wj[~bad], H, f"{name} N={N} joint")
    _close(mn, wm, H, f"{name} N={N} marg")
    assert (mn[~bad] >= jn[~bad]).all()
    # against the engine's own free energy of the stacked one-hot states (fp32 sums: looser, a plausibility check of the twin's reading)
    ok = torch.from_numpy(~bad).to(DEV)
    y = torch.zeros(N, K, device=DEV)
    y[torch.arange(N, device=DEV)[ok], gtd[ok].long()] = 1
    F = eng.free_energy(r, torch.cat([z, y], 1)).double().cpu().numpy()
    assert np.allclose(-F[~bad], jn[~bad], rtol=0, atol=H * 1e-5 + (Dz + K + H) * 2.0 ** -23 * np.abs(F).max() + 1e-4)
    # a row gives the same bits alone and inside the batch; a repeated call gives the same bits
    for i in (0, 1, N - 1):
        j1, m1 = eng.label_loglik(r, z[i:i + 1], K, gtd[i:i + 1])
        assert torch.equal(m1[0], m[i]) and (torch.equal(j1[0], j[i]) or (torch.isnan(j1[0]) and torch.isnan(j[i])))
    j2, m2 = eng.label_loglik(r, z, K, gtd)
    assert torch.equal(m2, m) and torch.equal(j2[~torch.isnan(j2)], j[~torch.isnan(j)])


@pytest.mark.parametrize("what", ["K1", "K257", "Dz0", "fit", "ldz", "N0"])
def test_label_loglik_invalid_arguments_name_the_value(eng, what):
    from imdbn.engine import native as N
    c = Cs.label_case("small", 5, False)
    Dz, K = c["Dz"], c["K"]
    r = device_rbm(c, groups=[(Dz, Dz + K)])
    d = eng._desc(r, False)
    z = torch.from_numpy(c["z"]).to(DEV)
    gt = torch.from_numpy(c["gt"]).to(DEV)
    j = torch.full((5,), -7.25, dtype=torch.float64, device=DEV)
    m = torch.full((5,), -7.25, dtype=torch.float64, device=DEV)
    n, dz, k, ldz, word = {"K1": (5, Dz, 1, Dz, "K = 1"), "K257": (5, Dz, 257, Dz, "K = 257"), "Dz0": (5, 0, K, Dz, "Dz = 0"),
                           "fit": (5, Dz, K + 1, Dz, f"K = {K + 1}"), "ldz": (5, Dz, K, Dz - 1, f"ldz {Dz - 1}"), "N0": (0, Dz, K, Dz, "N = 0")}[what]
    with pytest.raises(N.EngineError) as ei:
        eng._call("imdbn_rbm_label_loglik", C.byref(d), C.c_void_p(z.data_ptr()), ldz, n, dz, k, C.c_void_p(gt.data_ptr()),
                  C.c_void_p(j.data_ptr()), C.c_void_p(m.data_ptr()), *eng._ws_tail(torch.device(DEV), Dz, d.H, 5))
    torch.cuda.synchronize()
    print(what, "->", ei.value)
    assert "rc=-1)" in str(ei.value) and word in str(ei.value)
    assert (j == -7.25).all() and (m == -7.25).all()
