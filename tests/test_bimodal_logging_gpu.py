"""GPU: the hidden-state trace of imdbn_rbm_chain_traced_vh against the fp64 oracle on the chain kernel and on one launch per half
step, tracing as a pure observer, its argument checks, and imdbn.utils.bimodal_logging on the small trained bimodal model against
the reference's recording (bimodal_logging_small.npz, draws replayed from the fixture's seeds).

The chain checks go step by step (bimodal_logging_oracle.check_recorded_chain): each step's fp64 probabilities are computed from the
state the engine recorded entering it, so one Bernoulli decision at rounding distance from its uniform (40 rows x 12 steps x 788
decisions: there always is one) cannot make fp32 and fp64 chains part ways; the tolerance is on every recorded probability."""
import ctypes as C

import numpy as np
import pytest
import torch

import bimodal_logging_cases as BC
import bimodal_logging_oracle as BO
from oracle.draws import DrawStream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    yield E.get_hip_engine()


@pytest.fixture(scope="module")
def fx():
    return BC.fixture()


def _eng():
    from imdbn import engine as E
    return E.get_hip_engine()


def _rbm(W, hb, vb, groups=None):
    from imdbn.models import RBM
    r = RBM(W.shape[0], W.shape[1], 0.1, 1e-4, 0.5, softmax_groups=groups).to(DEV)
    r.W.data.copy_(torch.from_numpy(np.ascontiguousarray(W)))
    r.hid_bias.data.copy_(torch.from_numpy(hb)); r.vis_bias.data.copy_(torch.from_numpy(vb))
    return r


class _Tape:
    """Uniforms and normals of a DrawStream, categorical indices of a seeded generator (a replayed index is simply a given)."""

    def __init__(self, seed):
        self.s, self.g = DrawStream(seed), np.random.Generator(np.random.PCG64(seed + 1))

    def uniform(self, shape): return self.s.uniform(shape)
    def normal(self, shape): return self.s.normal(shape)
    def categorical(self, p): return self.g.integers(0, p.shape[1], p.shape[0])


def _step(**kw):
    return dict(dict(T=1.0, sigma=0.0, eta=0.0, sample_h=False, vmode=0, clamp=True), **kw)


SCHEDULES = {"sampled": lambda n: [_step(sample_h=True, vmode=1)] * n,
             "noisy": lambda n: [_step(T=0.7, sigma=0.3, sample_h=(i % 2 == 0), vmode=(1 if i % 3 == 0 else 0)) for i in range(n)]}


def _problem(V, H, B, groups, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    W = (g.standard_normal((V, H)) * (0.05 if V > 100 else 0.4)).astype(np.float32)
    hb, vb = (g.standard_normal(H) * 0.1).astype(np.float32), (g.standard_normal(V) * 0.1).astype(np.float32)
    vk = g.random((B, V), dtype=np.float32)
    ma, mb = np.zeros((B, V), np.float32), np.zeros((B, V), np.float32)
    cut = groups[0][0] if groups else V // 2
    ma[:, :cut] = 1; mb[:, cut:] = 1
    return W, hb, vb, vk, ma, mb


def _run_pair(r, vk, ma, mb, steps, seed, hwin_b, V, H):
    """The pair: a = visible full + baseline, hidden full; b = visible full, hidden `hwin_b`."""
    from imdbn import engine as E
    t = lambda x: torch.from_numpy(x).to(DEV)
    a = {"v_known": t(vk), "mask": t(ma), "steps": steps, "trace": (0, V, True), "trace_h": (0, H)}
    b = {"v_known": t(vk), "mask": t(mb), "steps": steps, "trace": (0, V, False), "trace_h": hwin_b}
    return _eng().chain_traced_vh(r, a, b, E.ReplayRng(_Tape(seed)))


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("sched", ["sampled", "noisy"])
@pytest.mark.parametrize("shape", ["36x24", "532x256"])
def test_hidden_trace_against_the_oracle(shape, sched, route):
    """36 <-> 24, B = 5: one partial block, partial MFMA tiles both ways; 532 <-> 256 with one softmax group, B = 40: three blocks
    per chain at 16 rows (the last partial), 12 steps, as a pair with a hidden trace on both members and a visible baseline on one;
    hidden window [5, 203) and the full one."""
    V, H, B, groups, n = (36, 24, 5, [], 6) if shape == "36x24" else (532, 256, 40, [(500, 532)], 12)
    W, hb, vb, vk, ma, mb = _problem(V, H, B, groups, 17)
    r = _rbm(W, hb, vb, groups)
    steps = SCHEDULES[sched](n)
    win = (5, 203) if H > 203 else (3, 17)
    eng = _eng()
    eng.set_option("no_chain_kernel", route)
    if shape == "532x256":
        eng.set_option("chain_rows", 16)
    try:
        (va, ta, ha), (vb_, tb, hb_) = _run_pair(r, vk, ma, mb, steps, 23, win, V, H)
        (va2, ta2, ha2), (vb2, tb2, hb2) = _run_pair(r, vk, ma, mb, steps, 23, (0, H), V, H)
    finally:
        eng.set_option("no_chain_kernel", 0)
        eng.set_option("chain_rows", 0)
    assert ta.shape == (n + 1, B, V) and ha.shape == (n, B, H) and tb.shape == (n, B, V) and hb_.shape == (n, B, win[1] - win[0])
    # the window is a slice of the full trace, bit for bit, and the window changes nothing else
    assert torch.equal(hb_, hb2[:, :, win[0]:win[1]]) and torch.equal(ha, ha2)
    assert torch.equal(va, va2) and torch.equal(vb_, vb2) and torch.equal(ta, ta2) and torch.equal(tb, tb2)
    src = _Tape(23)
    N = lambda x: x.cpu().numpy()
    for name, mask, vis, hid, fin, base in (("a", ma, ta, ha, va, True), ("b", mb, tb2, hb2, vb2, False)):
        eh, ev, same = BO.check_recorded_chain(W, hb, vb, groups, vk, mask, steps, src, N(vis), N(hid), N(fin), baseline=base)
        print(f"{shape} {sched} no_chain_kernel={route} chain {name}: hidden trace err {eh:.3g}, visible trace err {ev:.3g}")
        assert eh <= TOL and ev <= TOL, (name, eh, ev)
        assert same, f"chain {name}: the final state is not what the recorded last step leaves"
        h = N(hid)
        assert ((h > 0) & (h < 1)).any() and not np.isin(h, (0.0, 1.0)).all(), "probabilities, not samples"


def test_small_chain_free_running_against_the_oracle():
    """36 <-> 24, B = 5 on both routes against the free-running fp64 chain, on a seed whose every decision is 1e-4 clear."""
    from imdbn import engine as E
    V, H, B = 36, 24, 5
    W, hb, vb, vk, ma, _ = _problem(V, H, B, [], 17)
    steps = SCHEDULES["sampled"](6)
    for seed in range(100, 400):
        v, vis, hid, margin = BO.chain_vh(W, hb, vb, [], vk, ma, steps, _Tape(seed))
        if margin >= 1e-4:
            break
    else:
        raise AssertionError("no seed with robust draws")
    r = _rbm(W, hb, vb)
    t = lambda x: torch.from_numpy(x).to(DEV)
    for route in (0, 1):
        _eng().set_option("no_chain_kernel", route)
        try:
            ((fv, tv, th),) = _eng().chain_traced_vh(r, {"v_known": t(vk), "mask": t(ma), "steps": steps, "trace": (0, V, False),
                                                        "trace_h": (0, H)}, None, E.ReplayRng(_Tape(seed)))
        finally:
            _eng().set_option("no_chain_kernel", 0)
        BC.close(th.cpu(), hid, TOL, f"hidden trace, no_chain_kernel={route}")
        BC.close(tv.cpu(), vis, TOL, f"visible trace, no_chain_kernel={route}")
        BC.close(fv.cpu(), v, TOL, f"final state, no_chain_kernel={route}")


def test_tracing_only_observes_and_routes_agree():
    """Philox, sampled steps: final states and the rng offset equal between chain_pair, chain_traced and chain_traced_vh with and
    without hidden traces, on both routes; the routes' hidden traces agree to 1e-6."""
    from imdbn import engine as E
    V, H, B, groups = 532, 256, 40, [(500, 532)]
    W, hb, vb, vk, ma, mb = _problem(V, H, B, groups, 3)
    r = _rbm(W, hb, vb, groups)
    t = lambda x: torch.from_numpy(x).to(DEV)
    steps = SCHEDULES["sampled"](12)
    a = {"v_known": t(vk), "mask": t(ma), "steps": steps}
    b = {"v_known": t(vk), "mask": t(mb), "steps": steps}
    eng = _eng()
    hid = []
    for route in (0, 1):
        eng.set_option("no_chain_kernel", route)
        try:
            rngs = [E.PhiloxRng(seed=9) for _ in range(4)]
            p = eng.chain_pair(r, a, b, rngs[0])
            tr = eng.chain_traced(r, dict(a, trace=(500, V, True)), dict(b, trace=(0, 500, False)), rngs[1])
            v0 = eng.chain_traced_vh(r, dict(a, trace=(500, V, True)), dict(b, trace=(0, 500, False)), rngs[2])
            v1 = eng.chain_traced_vh(r, dict(a, trace=(500, V, True), trace_h=(0, H)), dict(b, trace_h=(5, 203)), rngs[3])
        finally:
            eng.set_option("no_chain_kernel", 0)
        assert len({x.offset for x in rngs}) == 1 and rngs[0].offset > 0
        for i in (0, 1):
            assert torch.equal(p[i], tr[i][0]) and torch.equal(p[i], v0[i][0]) and torch.equal(p[i], v1[i][0]), (route, i)
            assert v0[i][2] is None
            assert torch.equal(tr[i][1], v0[i][1])                       # NULL hidden traces: chain_traced, traces included
        assert torch.equal(tr[0][1], v1[0][1]) and v1[1][1] is None
        assert v1[0][2].shape == (12, B, H) and v1[1][2].shape == (12, B, 198)
        hid.append((v1[0][2].cpu(), v1[1][2].cpu()))
    BC.close(hid[0][0], hid[1][0], 1e-6, "hidden trace a: chain kernel vs per-launch")
    BC.close(hid[0][1], hid[1][1], 1e-6, "hidden trace b: chain kernel vs per-launch")


def test_argument_checks():
    from imdbn import engine as E
    from imdbn.engine import native as N
    V, H, B = 36, 24, 5
    W, hb, vb, vk, ma, _ = _problem(V, H, B, [], 17)
    r = _rbm(W, hb, vb)
    t = lambda x: torch.from_numpy(x).to(DEV)
    ch = {"v_known": t(vk), "mask": t(ma), "steps": SCHEDULES["sampled"](3)}
    for win in ((0, H + 1), (7, 7), (9, 4), (-1, 5)):
        with pytest.raises(N.EngineError, match="rc=-1"):
            _eng().chain_traced_vh(r, dict(ch, trace_h=win), None, E.PhiloxRng(seed=1))
    # with_baseline = 1 in a hidden trace, through the C entry
    eng = _eng()
    d = eng._desc(r, False)
    _, dev, specs, traces, results, sched, keep, hidden = eng._chain_specs("t", r, d, (dict(ch, trace=(0, V, True), trace_h=(0, H)), None), True)
    rr, _k = eng._rng(E.PhiloxRng(seed=1), sched, B, dev)
    lib = N.lib()
    tail = eng._ws_tail(dev, d.V, d.H, B)
    hidden[0][0].with_baseline = 1
    rc = lib.imdbn_rbm_chain_traced_vh(C.byref(d), B, C.byref(specs[0]), C.byref(traces[0]), C.byref(hidden[0][0]), None, None, None,
                                       C.byref(rr), *tail)
    assert rc == -1                                                       # IMDBN_E_INVALID
    hidden[0][0].with_baseline = 0
    rc = lib.imdbn_rbm_chain_traced_vh(C.byref(d), B, C.byref(specs[0]), C.byref(traces[0]), C.byref(hidden[0][0]), None, None, None,
                                       C.byref(rr), *tail)
    assert rc == 0                                                        # ... while a baseline in the VISIBLE trace is fine
    torch.cuda.synchronize()
    assert lib.imdbn_version() == 4


def test_trajectory_batch_rows_equal_the_b1_calls(fx):
    from imdbn import engine as E
    from imdbn.utils import bimodal_logging as L
    m = BC.model(fx, DEV)
    idx, T = [3, 40, 159, 77, 3, 12, 100], 12
    u = DrawStream(91).uniform((T, len(idx), 24))

    class Rows:
        def __init__(self, rows):
            self.rows, self.t = rows, 0

        def uniform(self, shape):
            self.t += 1
            return u[self.t - 1][self.rows]

    with E.use_rng(E.ReplayRng(Rows(slice(None)))):
        o = L.bimodal_trajectory_batch(m, idx, T)
    assert o["traj_h"].shape == (T + 1, len(idx), 24) and o["traj_z1"].shape == (T + 1, len(idx), 20)
    for i in range(len(idx)):
        with E.use_rng(E.ReplayRng(Rows(slice(i, i + 1)))):
            one = L.bimodal_trajectory_batch(m, idx[i:i + 1], T)
        for k in ("traj_h", "traj_z1"):
            BC.close(one[k][:, 0].cpu(), o[k][:, i].cpu(), 1e-6, f"row {i} {k}")
        for k in ("h_true", "z1_true", "z2_true"):
            BC.close(one[k][0].cpu(), o[k][i].cpu(), 1e-6, f"row {i} {k}")


def test_module_matches_the_reference_recording(fx):
    BC.check_module_against_recording(fx, DEV, tol=1e-5, pca_tol=5e-5, rho_tol=1e-6, probe_same=0.97)
