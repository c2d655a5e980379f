"""GPU: the weight / bias update (K3) on every kernel route against float64, each case asserting through imdbn_debug_last_update
that it launched the kernel and the tiles per block it names (update_cases.py has the table, the shapes and the reasoning).

  A  exact inputs through HipEngine.assoc_update: all six state tensors BIT-EQUAL to the float64 reference (signed zeros aside)
  B  real-valued and mixed inputs, non-trivial state and hyper-parameters: float64 within rel 2e-5 / atol 2e-6
  C  the routes only a CD pass reaches -- statistics into `delta` (cd_stats), the rank kernels (cd_factors + apply_factors) and a
     CD-1 train_epoch on the bin and planes routes -- against float64 computed from the operand planes the kernel read

Every call runs on a NaN-filled workspace; the options of a case are reset in a `finally`."""
import numpy as np
import pytest

import parity_cases as P
import update_cases as UC
import update_gpu as G
from golden_utils import assert_close

pytestmark = pytest.mark.gpu
DEV = G.DEV
F32, F64 = np.float32, np.float64
IDS = lambda c: c["id"]      # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    eng = E.get_hip_engine()             # raises if the library is missing: no silent fallback
    cu, arch = eng.device_info()
    assert "gfx950" in arch, arch
    assert cu >= 16, "the automatic tiles per block of the table's shapes is 1 only with more CUs than tiles"
    yield eng
    for k, v in UC.OPTION_DEFAULTS.items():
        eng.set_option(k, v)


_assert_update, _routed, _poison_ws, _rbm, _state, _close = G.assert_update, G.routed, G.poison_ws, G.rbm, G.state, G.close
_phases, _stats, _ws_reader, _block_reader = G.phases, G.stats, G.ws_reader, G.block_reader


# ---- A: exact inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", UC.cases("A"), ids=IDS)
def test_exact_inputs_give_the_float64_update_bit_for_bit(c, _native):
    ops = [P.T(x, DEV) for x in UC.operands(c)]
    ref = UC.ref_a(c)
    with _routed(_native, c):
        r = _rbm(c, UC.zero_params(c["V"], c["H"]), 0.0)
        _poison_ws(_native, c["V"], c["H"], c["B"])
        _native.assoc_update(r, *ops, 1.0, 0.0)
        _assert_update(c)
        got = _state(r)
    for k in UC.KEYS:
        want = ref[k].astype(F32)
        if not np.array_equal(got[k], want):
            bad = np.argwhere(got[k] != want)
            i = tuple(bad[0])
            raise AssertionError(f"{c['id']}: {k} differs from float64 at {len(bad)} of {want.size} elements, first {i}: got {got[k][i]!r}, "
                                 f"want {want[i]!r} (difference {float(got[k][i]) - float(want[i]):.3e}); rows {sorted(set(bad[:, 0]))[:8]}")


# ---- B: general arithmetic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", UC.cases("B"), ids=IDS)
def test_update_matches_float64_on_its_route(c, _native):
    ops = [P.T(x, DEV) for x in UC.operands(c)]
    with _routed(_native, c):
        r = _rbm(c, UC.params(c["V"], c["H"]), UC.B_WD, c["sparsity"])
        _poison_ws(_native, c["V"], c["H"], c["B"])
        _native.assoc_update(r, *ops, UC.B_LR, UC.B_MOM)
        _assert_update(c)
        got = _state(r)
    _close(c, got, UC.ref_b(c))


# ---- C: from the operand planes the kernel read ---------------------------------------------------------------------------------------
def _tagless(x):
    return P.T(x, DEV)


@pytest.mark.parametrize("c", UC.cases("C", "cd_stats"), ids=IDS)
def test_statistics_match_float64_of_the_planes(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    st = UC.params(V, H)
    with _routed(_native, c):
        r = _rbm(c, st, UC.C_WD)
        _poison_ws(_native, V, H, B)
        packed = _native.cd_stats(r, _tagless(UC.cd_data(c)), 1, E.PhiloxRng(seed=7))
        _assert_update(c)
        got = P.N(packed)[: V * H].reshape(V, H)
        vp, hp, vn, hn = _phases(c, B, _ws_reader(_native, c, B))
        after = _state(r)
    assert np.array_equal(vp.astype(F32), UC.cd_data(c)) or c["mode"] == "fast", "vis_tr0 does not hold the batch"
    want = vp.T @ hp - vn.T @ hn
    print(f"{c['id']}: max|d| {float(np.abs(got - want).max()):.3e} of max {float(np.abs(want).max()):.3e}")
    assert_close(got, want, UC.STATS_TOL["rel"], f"{c['id']}: statistics", atol=UC.STATS_TOL["atol"])
    for k in UC.KEYS:
        assert np.array_equal(after[k], st[k]), f"{c['id']}: the statistics pass changed {k}"


@pytest.mark.parametrize("c", UC.cases("C", "apply_factors"), ids=IDS)
def test_rank_update_matches_float64_of_the_gathered_planes(c, _native):
    from imdbn import engine as E
    V, H, R, Bl = c["V"], c["H"], c["R"], c["Bl"]
    st = UC.params(V, H)
    lr, mom = 0.07, 0.6
    with _routed(_native, c):
        r = _rbm(c, st, UC.C_WD)
        assert _native.factor_mode_ok(r, Bl)
        gathered = _native.gather_buffer(r, Bl, R)
        _poison_ws(_native, V, H, Bl)
        for rk in range(R):
            gathered[rk].copy_(_native.cd_factors(r, _tagless(UC.cd_data(c, rk)), 1, E.PhiloxRng(seed=11, row0=rk * Bl)))
        _native.apply_factors(r, gathered, Bl, R * Bl, lr, mom)
        _assert_update(c)
        got = _state(r)
        host = gathered.cpu().numpy()
        blocks = []
        for rk in range(R):
            read = _block_reader(_native, c, Bl, host[rk])
            blocks.append((_phases(c, Bl, read), read))
    if c["mode"] == "exact":
        for rk in range(R):
            assert np.array_equal(blocks[rk][0][0].astype(F32), UC.cd_data(c, rk)), f"rank {rk}: vis_tr0 does not hold the batch"
    _close(c, got, UC.ref_update(st, _stats(c, blocks), lr, mom, UC.C_WD, R * Bl))


@pytest.mark.parametrize("c", UC.cases("C", "train_epoch"), ids=IDS)
def test_cd1_step_matches_float64_of_the_planes(c, _native):
    from imdbn import engine as E
    V, H, B = c["V"], c["H"], c["B"]
    st = UC.params(V, H)
    with _routed(_native, c):
        r = _rbm(c, st, UC.C_WD)
        lr, mom = r._lr_mom(0)
        _poison_ws(_native, V, H, B)
        with E.use_rng(E.PhiloxRng(seed=13)):
            loss = r.train_epoch(_tagless(UC.cd_data(c)), 0, 10, CD=1)
        _assert_update(c)
        got = _state(r)
        read = _ws_reader(_native, c, B)
        ph = _phases(c, B, read)
    assert np.isfinite(float(loss)) and np.array_equal(ph[0].astype(F32), UC.cd_data(c))
    _close(c, got, UC.ref_update(st, _stats(c, [(ph, read)]), lr, mom, UC.C_WD, B))
