"""CPU: the fp64 logging oracle against the reference's recorded latent logging (logging_small.npz), and the module surface of
imdbn.utils.imdbn_logging / imdbn.utils.logging (names, parameter lists, alias identity, no plotting imports, native symbols)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import logging_oracle as LO
import trace_oracle as TO
from golden_utils import Fixture
from oracle.draws import DrawStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return Fixture("logging_small.npz")


@pytest.fixture(scope="module")
def small():
    w, X, Y = TO.small_model_arrays()
    return TO.SmallOracle(w), X, Y


def _traj(o, y, seed, T):
    u = DrawStream(seed).uniform((T, 1, 16)).astype(np.float64)
    return LO.trajectory(o.W, o.hb, o.vb, o.groups, o.zcm[y.argmax(1)], y, u)


def test_oracle_reproduces_the_neighbour_lists(fx, small):
    o, X, Y = small
    Zb, H = o.represent(X.astype(np.float64)), LO.row_keys(X)
    T, k = fx.meta["steps"], fx.meta["k"]
    n_keyed_skips = 0
    for ci, c in enumerate(fx.meta["cases"]):
        si = c["sample_idx"]
        traj, margin = _traj(o, Y[si:si + 1], c["seed"], T)
        assert margin > 1e-5
        met = "cosine_l1" if c["metric"] == "cosine" else c["metric"]
        key = H if c["dedup"] == "image" else None
        ex = [si] if c["exclude_self"] else None
        for name, q, m in (("true", o.represent(X[si:si + 1].astype(np.float64)), met), ("z0", traj[0], met), ("zT", traj[-1], met),
                           ("zT_l2", traj[-1], "l2")):
            ids, vals, _ = LO.topk(Zb, q, m, k, exclude=ex, key=key)
            np.testing.assert_array_equal(ids[0], fx[f"c{ci}_{name}_idx"], err_msg=f"case {ci} {name}")
            np.testing.assert_allclose(vals[0], fx[f"c{ci}_{name}_sc"], rtol=1e-5, atol=1e-6)
            if key is not None:
                plain, _, _ = LO.topk(Zb, q, m, k, exclude=ex)
                n_keyed_skips += int(not np.array_equal(plain[0], ids[0]))
        dec = TO.decode_sqerr(o.decode_layers(), Zb[fx[f"c{ci}_zT_idx"]], X[fx[f"c{ci}_zT_idx"]].astype(np.float64))
        np.testing.assert_allclose(dec, fx[f"c{ci}_decode_mse"], rtol=1e-5)
    assert n_keyed_skips > 0            # the image-key collisions change some lists: the quirk is exercised
    assert fx.meta["n_distinct_keys"] == len({tuple(r) for r in H}) < len(H)


def test_oracle_reproduces_topk_similar(fx, small):
    o, X, _ = small
    Zb = o.represent(X.astype(np.float64))
    for met in ("cosine", "ip", "l2"):
        ids, vals, _ = LO.topk(Zb, fx["topk_q"], met, fx.meta["k"])
        np.testing.assert_array_equal(ids, fx[f"topk_{met}_idx"], err_msg=met)
        np.testing.assert_allclose(vals, fx[f"topk_{met}_sc"], rtol=1e-5, atol=1e-6)


def test_oracle_reproduces_the_pca3_trajectory(fx, small):
    o, X, Y = small
    si = fx.meta["pca3"]["sample_idx"]
    traj, _ = _traj(o, Y[si:si + 1], fx.meta["pca3"]["seed"], fx.meta["steps"])
    np.testing.assert_allclose(traj[:, 0], fx["pca3_Ztraj"], atol=2e-6)
    Zb = o.represent(X.astype(np.float64))
    mean, comp = LO.pca(Zb, 3)
    np.testing.assert_allclose((Zb - mean) @ comp.T, fx["pca3_Z3"], atol=5e-5)
    np.testing.assert_allclose((traj[:, 0] - mean) @ comp.T, fx["pca3_T3"], atol=5e-5)


def test_oracle_reproduces_the_auto_recon_metrics(fx, small):
    o, X, Y = small
    t1, bce, mse = LO.auto_recon(o, X[:8], Y[:8])
    r = fx.meta["auto_recon"]
    assert t1 == r["auto_recon/text_top1"]
    assert bce == pytest.approx(r["auto_recon/text_bce"], rel=1e-5)
    assert mse == pytest.approx(r["auto_recon/image_mse"], rel=1e-5)


def test_both_module_paths_expose_the_reference_functions(fx):
    from imdbn.utils import imdbn_logging as M
    from imdbn.utils import logging as A
    for name, params in fx.meta["funcs"].items():
        for mod in (M, A):
            assert list(inspect.signature(getattr(mod, name)).parameters) == params, (mod.__name__, name)
        assert getattr(A, name) is getattr(M, name)
    for name in M.__all__:
        assert getattr(A, name) is getattr(M, name)


def test_import_pulls_in_no_plotting_dependency():
    code = ("import sys; import imdbn.utils.imdbn_logging, imdbn.utils.logging; "
            "bad = [m for m in ('wandb', 'torchvision', 'sklearn', 'matplotlib') if m in sys.modules]; "
            "assert not bad, bad")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "multimodal-idbn_amd")]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_library_exports_the_search_entries():
    from imdbn.engine import native
    lib = native.lib()
    for s in ("imdbn_row_stats", "imdbn_latent_topk"):
        assert hasattr(lib, s) and s in native.SIGNATURES


def test_oracle_tie_and_dedup_rules():
    # equal scores go to the lower index; a key keeps its best-ranked row; exclusion drops one row
    s = np.array([0.5, 0.9, 0.9, 0.1, 0.7, 0.9])
    key = np.array([[1, 1], [2, 2], [3, 3], [4, 4], [2, 2], [3, 3]], np.float64)
    ids, vals, _ = LO.topk_row(s, 4)
    assert ids.tolist() == [1, 2, 5, 4]
    ids, _, _ = LO.topk_row(s, 4, key=key)
    assert ids.tolist() == [1, 2, 0, 3]
    ids, _, _ = LO.topk_row(s, 4, exclude=1, key=key)
    assert ids.tolist() == [2, 4, 0, 3]
    ids, _, _ = LO.topk(np.eye(3), np.ones((1, 3)), "ip", 5)
    assert ids.tolist() == [[0, 1, 2, -1, -1]]
