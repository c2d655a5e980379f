"""CPU: the fp64 trace oracle against the reference's recorded convergence traces (cross_trace_small.npz), and the host logic of
imdbn.utils.conditional_steps (panel selection, step statistics, the reference's function and parameter names)."""
import inspect

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import trace_oracle as TO
from golden_utils import Fixture
from oracle.draws import DrawStream


@pytest.fixture(scope="module")
def fx():
    return Fixture("cross_trace_small.npz")


@pytest.fixture(scope="module")
def small():
    w, X, Y = TO.small_model_arrays()
    return TO.SmallOracle(w), X, Y


def test_oracle_img2txt_matches_the_reference(fx, small):
    o, _, _ = small
    T = fx.meta["max_steps"]
    x = fx["fixed_img"].reshape(1, -1)
    for pre, seed, gt, kw in (("fx_i2t_", fx.meta["seeds"]["fixed"], fx["fixed_lbl"].argmax(1), {}),
                              ("gap_i2t_", fx.meta["seeds"]["gap_i2t_"], None, {"gap_thresh": 0.02})):
        u = DrawStream(seed).uniform((1, 28)).astype(np.float64)
        r, steps, pred, _ = o.img2txt(x, u, T, gt=gt, **kw)
        s = int(steps[0])
        n = min(s, T)
        assert [s, int(pred[0])] == list(fx[pre + "scalars"][:2])
        assert len(fx[pre + "p_top1"]) == n
        np.testing.assert_allclose(r["p1"][0, :n], fx[pre + "p_top1"], atol=1e-6)
        np.testing.assert_allclose(r["p2"][0, :n], fx[pre + "p_top2"], atol=1e-6)
        np.testing.assert_allclose(r["l1"][0, :n], fx[pre + "l1"], atol=1e-6)
        np.testing.assert_array_equal(r["k1"][0, :n], fx[pre + "top1_idx"])
        if gt is not None:
            np.testing.assert_allclose(r["p_gt"][0, :n], fx[pre + "p_gt"], atol=1e-6)


def test_oracle_txt2img_matches_the_reference(fx, small):
    o, _, _ = small
    T = fx.meta["max_steps"]
    x, y = fx["fixed_img"].reshape(1, -1), fx["fixed_lbl"]
    for pre, kw in (("fx_t2i_", {}), ("ema_t2i_", {"beta": 0.3}), ("nozcm_t2i_", {"zcm": False})):
        r = o.txt2img(x, y, T, **kw)
        s = int(r["steps"][0])
        assert s == int(fx[pre + "steps"]), pre
        n = min(s, T)
        np.testing.assert_allclose(r["z_l2"][0, :n], fx[pre + "z_l2"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(r["image_mse"][0, :n], fx[pre + "image_mse"], rtol=1e-5)
        np.testing.assert_allclose(r["best_mse"][0], fx[pre + "best_mse"], rtol=1e-5)


def test_oracle_panel_steps_match_the_reference(fx, small):
    o, _, _ = small
    T = fx.meta["max_steps"]
    x, y = fx["panel_img"].reshape(len(fx["panel_img"]), -1), fx["panel_lbl"]
    u = DrawStream(fx.meta["seeds"]["panel"]).uniform((len(x), 28)).astype(np.float64)
    _, steps, _, _ = o.img2txt(x, u, T, gt=y.argmax(1))
    np.testing.assert_array_equal(steps, fx["panel_i2t_steps"])
    np.testing.assert_array_equal(o.txt2img(x, y, T)["steps"], fx["panel_t2i_steps"])


def test_steps_stats_and_names_match_the_reference(fx):
    from imdbn.utils import conditional_steps as CS
    ex = fx.meta["steps_stats_example"]
    st, mask = CS._steps_stats(ex["steps"], fx.meta["max_steps"])
    assert st == ex["stats"]
    assert mask.tolist() == ex["mask"]
    st, _ = CS._steps_stats([fx.meta["max_steps"] + 1] * 3, fx.meta["max_steps"])
    assert st["n_converged"] == 0 and st["mean"] is None and st["frac_converged"] == 0.0
    for name, params in fx.meta["funcs"].items():
        assert list(inspect.signature(getattr(CS, name)).parameters) == params, name


def test_fixed_val_panel_and_case_match_the_reference(fx, small):
    from imdbn.utils import conditional_steps as CS
    _, X, Y = small

    class M:
        pass

    m = M()
    m.device = torch.device("cpu")
    m.num_labels = 8
    m.val_loader = DataLoader(TensorDataset(torch.from_numpy(X), torch.from_numpy(Y)), batch_size=8, shuffle=False)
    imgs, lbls = CS.build_or_get_fixed_val_panel(m, per_class=2)
    np.testing.assert_array_equal(imgs.numpy(), fx["panel_img"])
    np.testing.assert_array_equal(lbls.numpy(), fx["panel_lbl"])
    assert CS.build_or_get_fixed_val_panel(m, per_class=5)[0].shape[0] == 16          # cached on the model
    img, lbl = CS.pick_fixed_val_case(m)
    np.testing.assert_array_equal(img.numpy(), fx["fixed_img"])
    np.testing.assert_array_equal(lbl.numpy(), fx["fixed_lbl"])
