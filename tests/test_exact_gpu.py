"""GPU: imdbn_rbm_exact_logz against the float64 reference of exact_oracle.py (log Z and both marginals, every case of
exact_cases.py), coverage spikes at the edges of the walk, the tile and the launch, determinism, read-only parameters, the AIS
estimators against the exact value above H = 16, and every error code of the header comment."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_cases as Xc
import exact_oracle as X
from likelihood_gpu import DEV, dev, device_rbm

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
_REF = {}


def _reference(name):
    """The float64 reference of a case: computed once, shared, never changed."""
    if name not in _REF:
        c = Xc.case(name)
        _REF[name] = (c, X.reference(c["W"], c["b"], c["c"], c["side"], c["groups"], c["z"], marginals=True))
    return _REF[name]


def _model(c):
    if c["z"] is None:
        r = device_rbm(c)
        if c.get("pitch"):
            V, H, p = c["V"], c["H"], c["pitch"]
            torch.as_strided(r.W.data, (V, p), (p, 1))[:, H:] = float("nan")
        return r, None
    from imdbn.models import GaussianRBM
    r = GaussianRBM(c["V"], c["H"], 0.01, 0.0, 0.5).to(DEV)
    r.W.data.copy_(dev(c["W"])); r.vis_bias.data.copy_(dev(c["b"])); r.hid_bias.data.copy_(dev(c["c"])); r.logvar.data.copy_(dev(c["z"]))
    return r, r.logvar.data


def _engine():
    from imdbn import engine as E
    return E.get_hip_engine()


@pytest.mark.parametrize("name", list(Xc.CASES))
def test_log_z_and_marginals_match_the_float64_reference(name):
    c, want = _reference(name)
    r, z = _model(c)
    got = _engine().exact_log_z(r, logvar=z, side=c["side"], marginals=True)
    lz, wm = float(got["log_z"]), float(got["log_w_max"])
    tol = Xc.tol_log_z(c, want["log_z"])
    tm_v = Xc.tol_marginal(c, want["log_z"], want["x_max"] if c["z"] is not None else None)
    tm_h = Xc.tol_marginal(c, want["log_z"])
    ev = np.abs(got["vis_mean"].cpu().numpy().astype(F64) - want["vis_mean"]).max()
    eh = np.abs(got["hid_mean"].cpu().numpy().astype(F64) - want["hid_mean"]).max()
    print(f"{name}: log Z {lz:.6f} off by {lz - want['log_z']:+.3e} (tol {tol:.3e}); vis_mean {ev:.3e} (tol {tm_v:.3e}), hid_mean {eh:.3e} "
          f"(tol {tm_h:.3e})")
    assert got["side"] == want["side"] and got["bits"] == c["n"]
    assert abs(lz - want["log_z"]) <= tol and abs(wm - want["log_w_max"]) <= tol
    assert ev <= tm_v and eh <= tm_h
    if c.get("pitch"):
        V, H, p = c["V"], c["H"], c["pitch"]
        assert torch.isnan(torch.as_strided(r.W.data, (V, p), (p, 1))[:, H:]).all()


def _spike_weight(s):
    """The float64 log-weight of the spike's own state."""
    e, f, Wd = (s["c"], s["b"], s["W"].T) if s["side"] == "hidden" else (s["b"], s["c"], s["W"])
    x = f.astype(F64) + s["bits"].astype(F64) @ Wd.astype(F64)
    return float(s["bits"].astype(F64) @ e.astype(F64) + X.softplus(x).sum())


SPIKES = [(12, s) for s in (0, 1, 31, 32, 33, 2 ** 12 - 1)] + [(23, s) for s in (0, 1, 31, 32, 33, 2 ** 23 - 1, 2 ** 22 - 1, 2 ** 22, 2 ** 22 + 1)]


@pytest.mark.parametrize("n,s_star", SPIKES)
def test_a_spike_at_every_edge_of_the_walk_is_counted_once(n, s_star):
    side = "visible" if (n == 12 and s_star in (1, 33)) else "hidden"
    s = Xc.spike(n, 9, s_star, 100 + n + s_star % 97, side)
    got = _engine().exact_log_z(device_rbm(s), side=side, marginals=True)
    want = _spike_weight(s)
    lz = float(got["log_z"])
    print(f"n {n} s* {s_star} ({side}): log Z {lz:.6f}, the state's weight {want:.6f}, off by {lz - want:+.3e}")
    # every other state is at least e^-39 below (one bias of 40 lost, the weights move a softplus by < 1): log Z - weight < 2^n e^-39
    assert abs(lz - want) <= Xc.tol_log_z(s, want) + (2.0 ** n) * np.exp(-39.0)
    e_mean = got["hid_mean"] if side == "hidden" else got["vis_mean"]
    assert np.abs(e_mean.cpu().numpy() - s["bits"]).max() <= 1e-6


def test_the_same_call_gives_the_same_bits_whatever_the_scratch_held():
    eng = _engine()
    for name in ("group2", "gauss_n12_d129", "vis_n12_d65"):
        c, _ = _reference(name)
        r, z = _model(c)
        a = eng.exact_log_z(r, logvar=z, side=c["side"], marginals=True)
        a = [a["log_z"].clone(), a["log_w_max"].clone(), a["vis_mean"].clone(), a["hid_mean"].clone()]
        b = eng.exact_log_z(r, logvar=z, side=c["side"], marginals=True)
        for k, buf in eng._ws.items():
            if isinstance(k[0], str) and k[0] == "exact":
                buf.view(torch.float32).fill_(float("nan"))
        d = eng.exact_log_z(r, logvar=z, side=c["side"], marginals=True)
        for x, y, w in zip(a, (b["log_z"], b["log_w_max"], b["vis_mean"], b["hid_mean"]), (d["log_z"], d["log_w_max"], d["vis_mean"], d["hid_mean"])):
            assert torch.equal(x, y) and torch.equal(x, w)


def test_parameters_are_only_read():
    c, _ = _reference("gauss_n6_d65")
    r, z = _model(c)
    before = [t.clone() for t in (r.W.data, r.vis_bias.data, r.hid_bias.data, z)]
    _engine().exact_log_z(r, logvar=z, marginals=True)
    for t, u in zip(before, (r.W.data, r.vis_bias.data, r.hid_bias.data, z)):
        assert torch.equal(t, u)


def test_ais_lies_within_three_of_its_standard_errors_of_the_exact_value_above_16_hidden_units():
    from imdbn.utils import likelihood as LK
    W, b, c, _ = Xc.params(784, 20, 31, 0.05)
    r = device_rbm((W, b, c))
    cal = LK.ais_calibration(r, n_chains=256, n_betas=1000, seed=11)
    print(f"784x20: AIS {cal['log_z']:.4f} exact {cal['log_z_exact']:.4f} gap {cal['log_z_gap']:+.4f} se {cal['se']:.4f} ess {cal['ess']:.1f}")
    assert abs(cal["log_z_gap"]) <= 3 * cal["se"]
    assert r.log_partition_exact()["bits"] == 20
    g = Xc.case("gauss_n12_d129")
    Wg, bg, cg, _ = Xc.params(64, 12, 32, 0.1)
    gc = dict(g, V=64, H=12, W=Wg, b=bg, c=cg, z=np.linspace(-2.0, 1.0, 64).astype(F32))
    gr, _ = _model(gc)
    calg = LK.gaussian_ais_calibration(gr, n_chains=256, n_betas=1000, seed=12)
    print(f"gauss 64x12: AIS {calg['log_z']:.4f} exact {calg['log_z_exact']:.4f} gap {calg['log_z_gap']:+.4f} se {calg['se']:.4f}")
    assert abs(calg["log_z_gap"]) <= 3 * calg["se"]
    # the particle yardstick on the device: a block whose column means ARE the exact marginals has no gap
    vm, _ = r.exact_marginals()
    res = LK.chain_marginal_gap(r, vm.repeat(4, 1))
    assert float(res["max_gap"]) <= 1e-6 and res["max_gap"].is_cuda and res["rms_gap"].dtype == torch.float64


def test_every_argument_error_comes_before_the_first_launch():
    from imdbn.engine import native as N
    eng = _engine()
    lib = N.lib()
    c, _ = _reference("n6_d65")
    r, _ = _model(c)
    d = eng._desc(r, False)
    need = lib.imdbn_exact_scratch_bytes(c["V"], c["H"], 0)
    assert need > 0 and lib.imdbn_exact_scratch_bytes(c["V"], c["H"], 3) == 0 and lib.imdbn_exact_scratch_bytes(40, 31, 1) == 0
    scratch = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    out = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    vm, hm = torch.full((c["V"],), 7.0, device=DEV), torch.full((c["H"],), 7.0, device=DEV)
    z = torch.zeros(c["V"], device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    st = eng._stream(torch.device(DEV))

    def call(desc=d, logvar=None, side=0, o=out, v=None, h=None, s=scratch, nbytes=None, off=0):
        rc = lib.imdbn_rbm_exact_logz(None if desc is None else C.byref(desc), p(logvar), side, p(o),
                                      p(v), p(h), C.c_void_p(0 if s is None else s.data_ptr() + off), need if nbytes is None else nbytes, st)
        buf = C.create_string_buffer(512)
        lib.imdbn_last_error(buf, 512)
        return rc, buf.value.decode()

    bad = [(dict(desc=None), "null"), (dict(o=None), "out"), (dict(s=None), "scratch"), (dict(side=3), "side = 3"), (dict(side=-1), "side = -1"),
           (dict(nbytes=need - 1), str(need - 1)), (dict(off=8), "aligned"), (dict(v=vm), "hid_mean"), (dict(h=hm), "vis_mean"),
           (dict(side=2, logvar=z), "logvar")]
    for kw, word in bad:
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw.keys(), rc, msg)
    wide = device_rbm(Xc.params(40, 31, 1, 0.1)[:3])
    rc, msg = call(desc=eng._desc(wide, False), side=1)
    assert rc == -5 and "31" in msg
    grp = device_rbm(Xc.params(12, 14, 1, 0.1)[:3], groups=[(2, 6)])
    rc, msg = call(desc=eng._desc(grp, False), side=2)
    assert rc == -5 and "softmax" in msg
    tall = device_rbm(Xc.params(12, 14, 1, 0.1)[:3])                        # V < H: side = 0 is the visible side, which is Gaussian here
    rc, msg = call(desc=eng._desc(tall, False), side=0, logvar=torch.zeros(12, device=DEV))
    assert rc == -5 and "Gaussian" in msg and "side = 1" in msg
    rc, msg = call(desc=eng._desc(grp, False), side=1, logvar=torch.zeros(12, device=DEV))
    assert rc == -5 and "Gaussian visibles with softmax groups" in msg
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (vm == 7.0).all() and (hm == 7.0).all() and (scratch == 0).all()
    with pytest.raises(N.EngineError, match="max_bits"):
        eng.exact_log_z(r, max_bits=5)
    # side = 0 is resolved by the library itself: H <= V (and a tie) is the hidden side, V < H the visible one
    rc, msg = call(v=vm, h=hm)
    torch.cuda.synchronize()
    want = _reference("n6_d65")[1]
    assert rc == 0 and abs(float(out[0]) - want["log_z"]) <= Xc.tol_log_z(c, want["log_z"])
    assert np.abs(hm.cpu().numpy() - want["hid_mean"]).max() <= Xc.tol_marginal(c, want["log_z"])
    for name, side_name in (("vis_n12_d65", "visible"), ("vis_n6_d6", "hidden")):
        cv, _ = _reference(name)
        wv = X.reference(cv["W"], cv["b"], cv["c"], side_name, marginals=True)
        rv, _ = _model(cv)
        nv = lib.imdbn_exact_scratch_bytes(cv["V"], cv["H"], 0)
        assert nv == lib.imdbn_exact_scratch_bytes(cv["V"], cv["H"], 2 if side_name == "visible" else 1)
        sv = torch.empty(nv, dtype=torch.uint8, device=DEV)
        ov = torch.empty(2, dtype=torch.float64, device=DEV)
        v2, h2 = torch.empty(cv["V"], device=DEV), torch.empty(cv["H"], device=DEV)
        rc, msg = call(desc=eng._desc(rv, False), side=0, o=ov, v=v2, h=h2, s=sv, nbytes=nv)
        torch.cuda.synchronize()
        cs = dict(cv, D=cv["H"] if side_name == "visible" else cv["V"])
        print(f"{name} side 0 -> {side_name}: log Z {float(ov[0]):.6f} off by {float(ov[0]) - wv['log_z']:+.3e}")
        assert rc == 0 and abs(float(ov[0]) - wv["log_z"]) <= Xc.tol_log_z(cs, wv["log_z"])
        assert np.abs(v2.cpu().numpy() - wv["vis_mean"]).max() <= Xc.tol_marginal(cs, wv["log_z"])
        assert np.abs(h2.cpu().numpy() - wv["hid_mean"]).max() <= Xc.tol_marginal(cs, wv["log_z"])
