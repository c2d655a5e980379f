"""GPU: the row-parallel chain kernel (k4_chain / k4_split_planes) and its host routing on every path against float64, each case
asserting through imdbn_debug_last_chain the route, rows per block, blocks and records it names (chain_cases.py has the table, the
reference, the derivation of the bounds and the reasoning).  Every chain runs through HipEngine.chain_traced_vh with full visible
and hidden windows on a NaN-filled workspace; every recorded probability of every half step of every row must lie within the derived
bound of its float64 value, and the final state must be what the recorded last step and the same draws leave, bit for bit.  The
options and the engine mode of a case are reset in a `finally`.  The largest error / bound ratio of each group is printed."""
import contextlib

import numpy as np
import pytest
import torch

import chain_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
IDS = lambda c: c["id"]      # noqa: E731
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()             # raises if the library is missing: no silent fallback
    cu, arch = eng.device_info()
    assert "gfx950" in arch, arch
    yield eng
    for k, v in CC.OPTION_DEFAULTS.items():
        eng.set_option(k, v)
    for g in CC.GROUPS:
        if g in WORST:
            print(f"[chain kernel] group {g}: largest error / bound {WORST[g][0]:.3f} ({WORST[g][1]})")


@contextlib.contextmanager
def _routed(eng, c):
    """The case's options and engine mode for the duration of the call."""
    from imdbn.engine import native
    mode = eng.mode
    try:
        for k, v in c["opts"].items():
            eng.set_option(k, v)
        eng.mode = native.FAST_BF16 if c["mode"] == "fast" else native.PARITY_F32
        yield
    finally:
        eng.mode = mode
        for k in c["opts"]:
            eng.set_option(k, CC.OPTION_DEFAULTS[k])


def _poison_ws(eng, V, H, B):
    eng._workspace(torch.device(DEV), V, H, B).view(torch.float32).fill_(float("nan"))


def _rbm(c, prob):
    """RBM from the constructor (row pitch forced and its padding poisoned with NaN where the case says so) with the problem's parameters."""
    from imdbn.models import RBM
    V, H = c["V"], c["H"]
    with pytest.MonkeyPatch.context() as mp:
        if c["pitch"]:
            mp.setenv("IMDBN_ROW_PITCH_ABS", str(c["pitch"]))
        r = RBM(V, H, 0.1, 1e-4, 0.5, softmax_groups=[tuple(g) for g in c["groups"]] or None).to(DEV)
    pitch = r.W.stride(0)
    if c["pitch"]:
        assert pitch == c["pitch"] > H
        torch.as_strided(r.W.data, (V, pitch), (pitch, 1))[:, H:] = float("nan")
    r.W.data.copy_(torch.from_numpy(prob["W"]).to(DEV))
    r.hid_bias.data.copy_(torch.from_numpy(prob["hb"]).to(DEV)); r.vis_bias.data.copy_(torch.from_numpy(prob["vb"]).to(DEV))
    assert r.W.stride(0) == pitch
    return r


def _dev(x, strided, pad):
    """The array on the device; `strided`: as a column slice of a wider NaN-filled tensor."""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    if not strided:
        return t
    wide = torch.full((t.size(0), t.size(1) + pad), float("nan"), device=DEV)
    wide[:, 3:3 + t.size(1)] = t
    return wide[:, 3:3 + t.size(1)]


def _rng(c):
    from imdbn import engine as E
    return E.PhiloxRng(seed=c["seed"], row0=c["row0"]) if c["rng"] == "philox" else E.ReplayRng(CC.source(c))


@pytest.mark.parametrize("c", CC.cases(), ids=IDS)
def test_chain_matches_float64_step_by_step_on_its_route(c, _native):
    eng = _native
    cu, _ = eng.device_info()
    V, H, B = c["V"], c["H"], CC.batch(c, cu)
    prob = CC.problem(c, cu)
    want = CC.expected(c, cu)
    vk, mu = _dev(prob["vk"], c["strided"], 13), (_dev(prob["mu"], c["strided"], 7) if prob["mu"] is not None else None)
    chains = []
    for i, ch in enumerate(c["chains"]):
        chains.append({"v_known": vk, "mask": _dev(prob["mask"][i], c["strided"], 13), "steps": ch["steps"], "init_uniform": ch["init_uniform"],
                       "mu": mu, "trace": (0, V, ch["base"]), "trace_h": (0, H)})
    if c["strided"]:
        assert vk.stride(0) == V + 13 and chains[0]["mask"].stride(0) == V + 13 and mu.stride(0) == mu.size(1) + 7
    with _routed(eng, c):
        r = _rbm(c, prob)
        _poison_ws(eng, V, H, B)
        res = eng.chain_traced_vh(r, chains[0], chains[1] if len(chains) == 2 else None, _rng(c))
        rec = eng.last_chain()
        torch.cuda.synchronize()
    got = (_code(rec["route"]), rec["rows"], rec["blocks"], rec["recs"])
    assert got == want, f"{c['id']}: the call left the chain record {got}, the case names {want} (route, rows, blocks, records) at {cu} CUs"
    if c["pitch"]:
        pitch = r.W.stride(0)
        assert torch.isnan(torch.as_strided(r.W.data, (V, pitch), (pitch, 1))[:, H:]).all(), "the row padding of W changed"
    src = CC.source(c)
    worst = 0.0
    for i, (fin, vis, hid) in enumerate(res):
        ch = c["chains"][i]
        vis, hid, fin = vis.cpu().numpy(), hid.cpu().numpy(), fin.cpu().numpy()
        assert vis.shape == (CC.n_recs(ch), B, V) and hid.shape == (ch["n"], B, H) and fin.shape == (B, V)
        assert np.isfinite(vis).all() and np.isfinite(hid).all() and np.isfinite(fin).all(), f"{c['id']} chain {i}: not finite"
        w = CC.walk(c, prob, i, src, CC.encoding(c, i), (vis, hid, fin))
        print(f"{c['id']} chain {i}: max err {w['err']:.3e}, max bound {w['bound']:.3e}, err / bound hidden {w['ratio_h']:.3f} visible {w['ratio_v']:.3f}")
        worst = max(worst, w["ratio_h"], w["ratio_v"])
        assert w["ratio_h"] <= 1.0, f"{c['id']} chain {i}: a hidden probability is {w['ratio_h']:.2f} bounds from float64"
        assert w["ratio_v"] <= 1.0, f"{c['id']} chain {i}: a visible probability is {w['ratio_v']:.2f} bounds from float64"
        if not w["final_equal"]:
            bad = np.argwhere(w["rebuilt"] != fin)
            raise AssertionError(f"{c['id']} chain {i}: the final state is not what the recorded last step leaves at {len(bad)} elements, "
                                 f"first (row, column) {tuple(bad[0])}, rows {sorted(set(bad[:, 0]))[:8]}")
    if worst > WORST.get(c["group"], (0.0, ""))[0]:
        WORST[c["group"]] = (worst, c["id"])


def _code(name):
    from imdbn.engine import native
    return native.CHAIN_ROUTE.index(name) if name is not None else -1
