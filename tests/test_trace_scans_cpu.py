"""CPU: the case tables of trace_cases.py reach every edge they name, the planted situations are there (asserted on the oracle
alone), the fp32 twins stay where the bounds need them, and the panel's seed meets its condition."""
import numpy as np

import trace_cases as TC
import trace_oracle as TO

F32, F64 = np.float32, np.float64


# ---- A ------------------------------------------------------------------------------------------------------------------------------------
def test_window_table_reaches_every_kind_of_window():
    V, H, (gs, ge) = TC.WIN_V, TC.WIN_H, TC.WIN_GROUP
    assert V % 16 and H % 16 and 0 < gs < ge < V
    calls = TC.window_calls()
    vis = {c[0][:2] for c in calls if c[0]}
    for base in (0, 1):
        assert {c[0][:2] for c in calls if c[0] and c[0][2] == base} == vis == set(TC.VIS_WINDOWS)
    one = [w for w in vis if w[1] - w[0] == 1]
    assert (0, 1) in one and (V - 1, V) in one and any(w[0] % 2 == 1 for w in one)
    assert any(w[0] % 16 and w[1] % 16 and w[0] < 16 < w[1] and w[0] < 64 < w[1] for w in vis), "no unaligned window across 16 and 64"
    assert (gs, ge) in vis and any(gs < w[0] and w[1] < ge for w in vis) and (0, V) in vis
    hid = {c[1] for c in calls if c[1]}
    assert hid == set(TC.HID_WINDOWS) and (0, 1) in hid and (H - 1, H) in hid and (0, H) in hid
    assert any(w[0] % 16 and w[1] % 16 and w[0] < 16 < w[1] and w[0] < 32 < w[1] for w in hid)
    assert any(c[0] and c[0][2] == 1 and c[1] and c[1] != (0, H) for c in calls), "no hidden window under a baseline slot (htr_t0 = 1)"
    assert any(c[0] and c[0][2] == 0 and c[1] for c in calls) and any(c[0] is None and c[1] for c in calls)
    pairs = TC.window_pairs()
    assert any(a[0] and not a[1] and b[1] and not b[0] for a, b in pairs), "no pair of a visible-only and a hidden-only chain"
    assert all(a != b for a, b in pairs)
    assert TC.RAW_VIS in vis and TC.RAW_HID in hid and TC.RAW_VIS[0] % 16 and TC.RAW_HID[0] % 16
    assert min(TC.WIN_BATCHES) == 1 and any(b % 16 for b in TC.WIN_BATCHES) and max(TC.WIN_BATCHES) > 64
    # at least 3 steps: two records or more, so the chain kernel applies; the option sends the same call down the other route
    assert TC.WIN_STEPS >= 3 and TC.window_route(0, False) == "kernel" and TC.window_route(0, True) == "kernel_pair"
    assert TC.window_route(1, False) == TC.window_route(1, True) == "per_launch"
    steps = TC.window_steps(0)
    assert any(s["sample_h"] for s in steps) and any(s["vmode"] for s in steps)


# ---- B ------------------------------------------------------------------------------------------------------------------------------------
def test_code_scan_table_and_the_twin_against_float64():
    cs = TC.code_cases()
    assert len({c["id"] for c in cs}) == len(cs)
    assert {c["Dz"] % 64 for c in cs} >= {0, 1, 63} and any(c["Dz"] > 128 for c in cs) and any(c["Dz"] == 1 for c in cs)
    assert any(c["B"] % 4 for c in cs) and any(c["B"] % 4 == 0 for c in cs) and any(c["B"] == 1 for c in cs) and any(c["B"] > 8 for c in cs)
    assert {c["T"] for c in cs} == {1, 6} and {round(c["beta"], 6) for c in cs} == {0.0, 0.3, 1.0}
    assert any(c["strided"] and c["Dz"] % 64 == 1 for c in cs) and any(c["data"] == "grid" for c in cs)
    for c in cs:
        assert c["beta"] == float(F32(c["beta"]))
        zs, z0 = TC.code_inputs(c)
        zn, dz = TO.code_scan_f32(zs, z0, c["beta"])
        zr, dr = TC.code_ref(c["id"])
        assert c["data"] == "grid" or (dr > 0).all(), c["id"]
        if c["beta"] == 0.0:
            assert np.array_equal(zn, zs)
        if c["data"] == "grid":
            # the grid's sums are exact in fp32 in any order: the twin's sum of squares IS the exact one, only the root rounds
            assert np.array_equal(zs * 64, np.round(zs * 64)) and np.array_equal(z0 * 64, np.round(z0 * 64))
            want = np.sqrt(dr ** 2).astype(F32)
            assert (np.abs(dz.astype(F64) - want.astype(F64)) <= np.spacing(want).astype(F64)).all(), c["id"]
            assert np.array_equal((dz.astype(F64) ** 2 * 4096).round(), (dr ** 2 * 4096).round())
    for Dz in TC.CODE_DZ:
        wz, wd = TC.code_scan_twin_worst(Dz)
        bz, bd = TC.code_scan_bounds(Dz)
        print(f"code scan twin against float64, Dz {Dz}: z_new {wz:.3g} absolute, dz {wd:.3g} relative; bounds {bz:.3g}, {bd:.3g}")
        # the twin is fp32 arithmetic on numbers in [0, 1]: a few ulp on z_new; dz likewise once a row sums many columns (one
        # difference alone can cancel, which the parity cap then bounds)
        assert 0 < wz <= 4 * 2.0 ** -24 and 0 < wd and bz == 4 * wz and bd == min(4 * wd, TC.PARITY)
        assert Dz == 1 or wd <= 1e-6


# ---- C ------------------------------------------------------------------------------------------------------------------------------------
def test_patience_plants_are_present_on_the_oracle_alone():
    cs = TC.patience_cases()
    assert {c["B"] % 64 for c in cs} >= {0, 1, 63} and any(c["B"] > 128 for c in cs) and {c["T"] for c in cs} == {1, 2, 7}
    seen = set()
    for c in cs:
        dz, mse, rows = TC.patience_inputs(c)
        T, P = c["T"], c["P"]
        # dyadic, NaN or +inf: every comparison of the rule is exact in double
        fin = np.isfinite(mse)
        assert np.array_equal(mse[fin] * 1024, np.round(mse[fin] * 1024)) and np.array_equal(dz * 4096, np.round(dz * 4096))
        steps, best = TC.patience_ref(c)
        for name, b in rows.items():
            _, _, ws, wb = TC.plant(name, T, P)
            assert steps[b] == ws and best[b] == wb, (c["id"], name, steps[b], ws, best[b], wb)
            seen.add(name)
        if c["B"] >= 63:
            fits = {n for n in TC.PLANTS if TC.plant(n, T, P) is not None}
            assert set(rows) == fits
            if T == 7:
                assert fits == set(TC.PLANTS) - ({"late_reset"} if P == 1 else set()), (c["id"], fits)
            assert (steps <= T).any() or T < P
    assert seen == set(TC.PLANTS)
    # what each plant is there for, on the oracle
    T, P = 7, 3
    get = lambda n: TC.plant(n, T, P)      # noqa: E731
    assert get("stop_at_patience")[2] == P and get("all_nan")[2] == P and np.isnan(get("all_nan")[1]).all() and get("all_nan")[3] == np.inf
    assert get("stop_at_T")[2] == T and get("never")[2] == T + 1
    dz, mse, s, _ = get("dz_equals_eps")
    assert (dz == TC.EPS_Z).all() and s == T + 1
    assert TO.patience_scan(dz[None] - TC.SMALL, mse[None], TC.EPS_Z, TC.MSE_TOL, P)[0][0] == P + 1      # just below, it would stop
    dz, mse, s, b = get("exact_tol")
    assert mse[0] - mse[1] == TC.MSE_TOL and b == mse[0] and s == P + 1
    m2 = mse.copy(); m2[1:] -= TC.MSE_TOL                                  # twice the tolerance is taken
    assert TO.patience_scan(dz[None], m2[None], TC.EPS_Z, TC.MSE_TOL, P)[1][0] == m2[1]
    dz, mse, s, b = get("late_reset")
    assert s == 2 * P and mse[P - 1] < mse[P - 2]
    dz, mse, s, b = get("improve_at_stop")
    assert s == 2 * P + 1 and mse[P] < mse[P - 1] and (mse[:P] == mse[0]).all()      # the counter stood at P - 1 when step P + 1 improved
    assert np.isinf(get("inf_inside")[1]).any() and np.isfinite(get("inf_inside")[1]).any()


# ---- D ------------------------------------------------------------------------------------------------------------------------------------
def test_decode_table_and_the_bound_on_the_twin():
    cs = TC.decode_cases()
    assert len({c["id"] for c in cs}) == len(cs)
    one = [c for c in cs if len(c["sizes"]) == 2]
    assert {c["sizes"] for c in one} == {(V, H) for V in TC.DEC_V for H in TC.DEC_H}
    assert {V % 256 for V in TC.DEC_V} >= {0, 1, 255} and any(V > 512 for V in TC.DEC_V) and any(V < 64 for V in TC.DEC_V)
    assert any(H % 4 for H in TC.DEC_H) and any(H % 4 == 0 and H > 128 for H in TC.DEC_H)
    for key, vals in (("B", TC.DEC_B), ("kind", ("binary", "real")), ("ref_row", TC.REF_ROWS), ("strided", (False, True))):
        for v in vals:
            assert len({c["sizes"] for c in one if c[key] == v}) >= 3, (key, v)
    for V in TC.DEC_V:
        assert {c["kind"] for c in one if c["sizes"][0] == V} == {"binary", "real"}
    assert any(len(c["sizes"]) == 3 for c in cs) and any(c["B"] > 128 for c in cs) and any(c["B"] % 64 for c in cs)
    worst = 0.0
    for c in cs:
        z, ref, rows = TC.decode_inputs(c)
        R = ref.shape[0]
        if rows is not None:
            assert rows.dtype == np.int32 and rows.min() >= 0 and rows.max() < R and rows.shape == (c["B"],)
            if c["ref_row"] == "repeat" and c["B"] > 4:
                assert R < c["B"] and np.bincount(rows).max() > 1
            if c["ref_row"] == "perm":
                assert sorted(rows) == list(range(c["B"]))
        mse, bound = TC.decode_ref(c)
        frac = np.abs(TC.decode_twin(c).astype(F64) - mse) / bound
        worst = max(worst, float(frac.max()))
        assert (frac <= 1).all(), (c["id"], frac.max())
    print(f"decode error: the twin's largest fraction of the derived bound {worst:.3g}")


def test_row_sqerr_twin_is_a_mean_of_squares():
    g = np.random.Generator(np.random.PCG64(1))
    for N in (5, 255, 256, 257, 700):
        x, r = g.integers(0, 65, (3, N)).astype(F32) / 64, g.integers(0, 65, (3, N)).astype(F32) / 64
        s = ((x.astype(F64) - r) ** 2).sum(1)                                # exact on the grid: only the division rounds
        assert np.array_equal(TO.row_sqerr_f32(x, r), (s.astype(F32) / F32(N)).astype(F32))


# ---- E ------------------------------------------------------------------------------------------------------------------------------------
def test_panel_seed_meets_its_condition_on_the_oracle_alone():
    assert TC.PANEL_SEED == TC.panel_seed(), "the pinned seed is not the first that meets the condition"
    (r, s1, pred, m1), t = TC.panel_oracle(TC.PANEL_SEED)
    s2, m2 = t["steps"], t["margin"]
    excused = int((m1 <= TC.PANEL_MARGIN).sum() + (m2 <= TC.PANEL_MARGIN).sum())
    print(f"panel seed {TC.PANEL_SEED}: {excused} rows within {TC.PANEL_MARGIN} of a threshold; img2txt steps {s1.tolist()}, txt2img {s2.tolist()}")
    assert excused <= TC.PANEL_B // 4
    for s in (s1, s2):
        assert (s <= TC.PANEL_T).any() and len(set(s.tolist())) >= 2
    assert r["p1"].shape == (TC.PANEL_B, TC.PANEL_T) and t["image_mse"].shape == (TC.PANEL_B, TC.PANEL_T)
    w, X, Y, yi = TC.panel(TC.PANEL_SEED)
    assert w["joint_W"].shape == (26, 19) and X.shape == (9, 67) and [w[f"img{i}_W"].shape for i in range(2)] == [(67, 33), (33, 21)]
