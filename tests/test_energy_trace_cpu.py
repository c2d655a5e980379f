"""CPU: the fp64 energy-trace oracle against the reference's recorded traces (energy_trace_small.npz), and the host logic of
imdbn.utils.energy_utils (the reference's function and parameter names, the fixed case, the cut of the curves, logging) --
plus the ISA listing of the new kernel (no scratch)."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import energy_oracle as EO
import trace_oracle as TO
from golden_utils import Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISA = os.path.join(ROOT, "multimodal-idbn_amd", "build", "engine-hip-amdgcn-amd-amdhsa-gfx950.s")


@pytest.fixture(scope="module")
def fx():
    return Fixture("energy_trace_small.npz")


@pytest.fixture(scope="module")
def small():
    w, X, Y = TO.small_model_arrays()
    return TO.SmallOracle(w), X, Y


def _oracle(o, x, T, **kw):
    z = np.clip(o.represent(np.asarray(x, np.float64).reshape(len(x), -1)), 1e-6, 1 - 1e-6)
    return EO.trace(o.W, o.hb, o.vb, z, 8, T, **kw)


def _check(e, b, fx, pre, i):
    ints, fl = fx[pre + "ints"][i], fx[pre + "floats"][i]
    T = fx.meta["steps"]
    assert [int(e["conv"][b]), int(e["kstar"][b]), int(e["predT"][b])] == ints[:3].tolist(), (pre, i)
    n = min(int(ints[0]), T)
    assert np.isnan(fx[pre + "p_top1"][i, n:]).all() and not np.isnan(fx[pre + "p_top1"][i, :n]).any()
    for k, ek in (("p_top1", "p1"), ("p_top2", "p2"), ("l1", "l1")) + ((("p_gt", "p_gt"),) if ints[3] >= 0 else ()):
        np.testing.assert_allclose(e[ek][b, :n], fx[pre + k][i, :n], atol=1e-6, err_msg=pre + k)
    np.testing.assert_allclose(e["p1"][b, :n] - e["p2"][b, :n], fx[pre + "p_gap"][i, :n], atol=1e-6)
    # free energies of this model are O(10): fp32 rounding of the reference is ~1e-6 relative
    np.testing.assert_allclose(e["F"][b], fx[pre + "F"][i], rtol=1e-5)
    np.testing.assert_allclose(e["dF"][b, :n], fx[pre + "deltaF_pred_traj"][i, :n], atol=2e-5 * np.abs(e["F"][b]).max())
    np.testing.assert_allclose([e["margin_energy"][b], e["dF"][b, n - 1]], fl[[0, 3]], atol=2e-5 * np.abs(e["F"][b]).max())
    np.testing.assert_allclose([e["fe_top1"][b], e["fe_gap"][b]], fl[[1, 2]], atol=1e-5 * np.abs(e["F"][b]).max())
    np.testing.assert_allclose([e["p1"][b, n - 1], e["p1"][b, n - 1] - e["p2"][b, n - 1]], fl[[4, 5]], atol=1e-6)


def test_oracle_matches_the_reference(fx, small):
    o, _, _ = small
    T = fx.meta["steps"]
    gt = fx["fixed_lbl"].argmax(1)
    _check(_oracle(o, fx["fixed_img"], T, gt=gt), 0, fx, "fx_", 0)
    _check(_oracle(o, fx["fixed_img"], T), 0, fx, "nl_", 0)
    assert int(fx["nl_ints"][0, 3]) == -1 and np.isnan(fx["nl_p_gt"]).all()
    e = _oracle(o, fx["gap_img"], T, gt=fx["gap_lbl"].argmax(1), gap_thresh=fx.meta["gap_small"])
    _check(e, 0, fx, "gp_", 0)
    assert e["predT"][0] != e["kstar"][0] and e["conv"][0] <= T                  # the gap branch of the stop rule
    e = _oracle(o, fx["panel_img"], T, gt=fx["panel_lbl"].argmax(1))
    assert len(fx["pn_ints"]) >= 32 and sorted(set(fx["pn_ints"][:, 0].tolist())) == [3, 4, T + 1]
    for i in range(len(fx["pn_ints"])):
        _check(e, i, fx, "pn_", i)
    np.testing.assert_array_equal(e["conv"], fx["pn_ints"][:, 0])
    assert min(fx.meta["min_room"].values()) >= fx.meta["room"] == 1e-5       # every recorded decision has room (the generator asserts it)


def test_names_parameters_and_dict_keys_match_the_reference(fx):
    """Fails before this module had the tracing half: the reference's names must exist with the reference's parameters."""
    from imdbn.utils import energy_utils as EU
    for name, params in fx.meta["funcs"].items():
        assert hasattr(EU, name), f"imdbn.utils.energy_utils.{name} is missing"
        assert list(inspect.signature(getattr(EU, name)).parameters) == params, name
    ref_defaults = {"steps": 30, "eps_l1": 1e-3, "stable_steps": 3, "gap_thresh": 0.25}
    sig = inspect.signature(EU.trace_single_img2txt).parameters
    assert {k: sig[k].default for k in ref_defaults} == ref_defaults
    sig = inspect.signature(EU.trace_img2txt_energy_batch).parameters
    assert list(sig)[:3] == ["model", "imgs", "lbls"] and {k: sig[k].default for k in ref_defaults} == ref_defaults
    assert inspect.signature(EU.run_and_log_energy_panel).parameters["per_class"].default == 4
    from imdbn.utils import conditional_steps as CS
    assert EU.pick_fixed_val_case is CS.pick_fixed_val_case                      # one function, not two copies


def _host(n_rows, T, conv, with_gt=True):
    g = np.random.Generator(np.random.PCG64(3))
    o = {k: torch.from_numpy(g.random((n_rows, T), dtype=np.float32)) for k in ("p_top1", "p_top2", "deltaF_pred", "l1")}
    o["p_gt"] = torch.from_numpy(g.random((n_rows, T), dtype=np.float32)) if with_gt else None
    o["k1"] = torch.zeros(n_rows, T, dtype=torch.int32)
    o["steps"] = torch.tensor(conv, dtype=torch.int32)
    o["kstar"] = torch.arange(n_rows, dtype=torch.int32)
    o["predT"] = torch.arange(n_rows, dtype=torch.int32) + 1
    for k in ("margin_energy", "fe_top1", "fe_gap"):
        o[k] = torch.from_numpy(g.random(n_rows, dtype=np.float32))
    o["F"] = torch.zeros(n_rows, 8)
    o["gt"] = torch.arange(n_rows) if with_gt else None
    return o


def test_host_cut_of_the_curves(fx):
    from imdbn.utils import energy_utils as EU
    T = 6
    o = _host(3, T, [2, T, T + 1])
    h = EU._to_host(o)
    for i, n in enumerate((2, T, T)):
        c = EU._case_dict(h, i, T, 8)
        assert list(c) == fx.meta["dict_keys"]
        assert [len(c[k]) for k in ("deltaF_pred_traj", "p_top1", "p_top2", "p_gap", "p_gt")] == [n] * 5
        assert c["p_top1"] == o["p_top1"][i, :n].double().tolist()
        assert c["p_gap"] == [a - b for a, b in zip(c["p_top1"], c["p_top2"])]
        assert c["p_top1_final"] == c["p_top1"][-1] and c["p_gap_final"] == c["p_gap"][-1]
        assert c["deltaF_pred_final"] == c["deltaF_pred_traj"][-1]
        assert (c["steps_to_converge"], c["kstar"], c["predT"], c["gt"]) == (int(o["steps"][i]), i, i + 1, i)
        assert c["margin_energy"] == float(o["margin_energy"][i]) and c["fe_gap_final"] == float(o["fe_gap"][i])
    c = EU._case_dict(EU._to_host(_host(1, T, [1], with_gt=False)), 0, T, 8)
    assert c["p_gt"] is None and c["gt"] is None and len(c["p_top1"]) == 1
    # the reference's empty-list fallbacks (:178, :184-185)
    h = EU._to_host(_host(1, T, [0]))
    c = EU._case_dict(h, 0, T, 8)
    assert c["deltaF_pred_final"] is None and c["p_top1_final"] == 1.0 / 8 and c["p_gap_final"] == 0.0


def test_fixed_case_alias_and_logging(fx, small):
    from imdbn.utils import energy_utils as EU
    _, X, Y = small

    class M:
        pass

    m = M()
    m.device = torch.device("cpu")
    m.num_labels = 8
    m.val_loader = DataLoader(TensorDataset(torch.from_numpy(X), torch.from_numpy(Y)), batch_size=8, shuffle=False)
    img, lbl = EU.pick_val_case(m, batch_idx=5)                                   # batch_idx is ignored
    np.testing.assert_array_equal(img.numpy(), fx["fixed_img"])
    np.testing.assert_array_equal(lbl.numpy(), fx["fixed_lbl"])
    img2, _ = EU.pick_val_case(m, target_label=3, batch_idx=1, within_batch_index=2)      # cached on the model
    assert torch.equal(img, img2)

    class Run:
        def __init__(self):
            self.logged = []

        def log(self, d):
            self.logged.append(d)

    case = EU._case_dict(EU._to_host(_host(1, 6, [4])), 0, 6, 8)
    assert EU.log_single_case_energy(m, case, epoch=2) is None                    # no wandb_run attribute: silent
    m.wandb_run = None
    assert EU.log_single_case_energy(m, case, epoch=2) is None
    m.wandb_run = Run()
    EU.log_single_case_energy(m, case, epoch=7, tag="fixed")
    assert len(m.wandb_run.logged) == 1
    got = m.wandb_run.logged[0]
    assert got["epoch"] == 7 and list(got["case/fixed/summary"]) == list(fx.meta["logged_summary"])
    assert got["case/fixed/summary"] == {k: case[k] for k in fx.meta["logged_summary"]}


def test_energy_kernel_has_no_scratch():
    import __graft_entry__ as ge
    if not (os.path.exists(ISA) and ge._fresh(ISA)):
        ge.build()
    fn, bodies = None, {}
    for line in open(ISA):
        m = re.match(r"^(_ZN5imdbn17energy_trace_rows\w+):\s", line)
        if m:
            fn = m.group(1)
            bodies[fn] = []
        elif fn is not None:
            if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                fn = None
            else:
                bodies[fn].append(line.strip())
    assert len(bodies) == 4, sorted(bodies)                                       # Wy in LDS / global x base, h in LDS / global
    for name, body in bodies.items():
        assert not any(l.startswith("scratch_") for l in body), f"{name} spills to scratch"
        assert any(l.startswith("v_readlane_b32") for l in body), f"{name}: the label broadcast is no longer a v_readlane"
