"""CPU-only: the numpy twin of imdbn_cross_metrics against the reference's recorded ``_log_snapshots`` (snapshots_small.npz), the
export's declaration and binding, and the host logic of imdbn/utils/cross_eval.py on a test double of the engine."""
import os
import re

import numpy as np
import pytest
import torch

import cross_eval_oracle as CO
from cross_eval_cases import Run, Tape, small_model as _small_model
from golden_utils import Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 1e-6


@pytest.fixture(scope="module")
def fx():
    return Fixture("snapshots_small.npz")


def _rel(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b) / np.abs(b)
    print(f"{what}: max relative error {err.max():.3g} (tolerance {tol:g})")
    assert err.max() <= tol, f"{what}: {err.max():.3g} > {tol:g}"


def test_fixture_has_room_on_all_rows(fx):
    p = fx["p_y_given_img"]
    top2 = np.sort(p, axis=1)[:, ::-1][:, :2]
    assert p.shape == (8, 8) and fx.meta["room"] == 1e-5
    assert float((top2[:, 0] - top2[:, 1]).min()) == fx.meta["min_margin"] >= fx.meta["room"]
    assert np.array_equal(fx["table_int"][:, 0], np.arange(8))
    assert fx.meta["signature"] == ["self", "epoch", "num"]


def test_oracle_twin_reproduces_the_recorded_snapshot(fx):
    s = CO.snapshot(fx["img_from_txt"], fx["p_y_given_img"], fx["imgs"], fx["lbls"])
    m = CO.metrics(fx["p_y_given_img"], y=fx["lbls"], row_mse=CO.row_mse(fx["img_from_txt"], fx["imgs"]), npix=fx["imgs"].shape[1])
    top1, top3, ce, mse_sum = fx["ref_metrics"]
    # decisions: exact
    assert np.array_equal(s["pred"], fx["cm_preds"]) and np.array_equal(s["gt"], fx["cm_y_true"])
    assert np.array_equal(s["pred"], fx["table_int"][:, 2]) and np.array_equal(s["gt"], fx["table_int"][:, 1])
    assert [row[:3] for row in s["table"]] == fx["table_int"].tolist()
    assert m["acc"][0] == 8 and m["acc"][1] == top1 and m["acc"][2] == top3 and m["acc"][5] == 0
    assert int((m["rank"] == 0).sum()) == top1 and int((m["rank"] < 3).sum()) == top3
    want = np.zeros((8, 8), np.int64)
    np.add.at(want, (fx["cm_y_true"], fx["cm_preds"]), 1)
    assert np.array_equal(s["confusion"], want) and np.array_equal(m["confusion"], want)
    assert np.array_equal(m["class_sums"][:, 0], want.sum(1)) and np.array_equal(m["class_sums"][:, 1], np.diag(want))
    # numbers
    _rel(m["acc"][3], ce, REL, "ce_sum vs the reference's F.binary_cross_entropy")
    _rel(m["acc"][4], mse_sum, REL, "mse_sum vs the reference's F.mse_loss")
    _rel(s["snap/image_mse"], fx["snap_image_mse"], REL, "snap/image_mse")
    _rel([row[3] for row in s["table"]], fx["table_p"][:, 0], REL, "p_pred")
    _rel([row[4] for row in s["table"]], fx["table_p"][:, 1], REL, "p_true")
    _rel(m["class_sums"][:, 2].sum() * fx["imgs"].shape[1], mse_sum, REL, "class sums of row_mse")
    # the same rows through evaluate(): what joint_history's scalars mean (reference :649-652)
    e = CO.evaluate([(fx["img_from_txt"][:5], fx["p_y_given_img"][:5], fx["imgs"][:5], fx["lbls"][:5]),
                     (fx["img_from_txt"][5:], fx["p_y_given_img"][5:], fx["imgs"][5:], fx["lbls"][5:])])
    assert e["n"] == 8 and e["text_top1"] == top1 / 8 and e["text_top3"] == top3 / 8
    _rel(e["text_ce"], ce / 8, REL, "text_ce")
    _rel(e["image_mse"], mse_sum / (8 * 100), REL, "image_mse")
    absent = want.sum(1) == 0
    assert np.isnan(e["per_class_acc"][absent]).all() and not np.isnan(e["per_class_acc"][~absent]).any()


def test_oracle_tie_and_clamp_rules():
    p = np.array([[0.5, 0.5, 0.1], [0.2, 0.7, 0.7], [0.3, 0.3, 0.3], [0.0, 1.0, 1e-8]], np.float32)
    m = CO.metrics(p, gt=np.array([1, 2, 1, 0]), topk=1)
    assert m["pred"].tolist() == [0, 1, 0, 1] and m["rank"].tolist() == [1, 1, 1, 2]
    assert m["acc"][1] == 0 and m["acc"][2] == 0
    assert m["p_true"][3] == np.float32(1e-9) and m["p_pred"][3] == 1.0
    row3 = -(np.log(np.float64(np.float32(1e-6))) + np.log(np.float64(np.float32(1) - np.float32(1.0 - 1e-6)))
             + np.log(np.float64(np.float32(1) - np.float32(1e-6))))
    assert abs(m["ce_rows"][3] - row3) < 1e-12
    o = CO.metrics(p, gt=np.array([1, 7, -1, 0]))
    assert o["acc"][0] == 2 and o["acc"][5] == 2 and o["rank"].tolist()[1:3] == [-1, -1] and np.isnan(o["p_true"][1])


def _declared_args(name):
    src = open(os.path.join(ROOT, "include", "imdbn_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m, f"{name} is not declared in include/imdbn_engine.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_export_is_declared_and_bound():
    import ctypes as C
    from imdbn.engine import native
    args = _declared_args("imdbn_cross_metrics")
    res, argtypes = native.SIGNATURES["imdbn_cross_metrics"]
    assert res is C.c_int and len(argtypes) == len(args) == 14, (len(argtypes), args)
    assert args[0].startswith("const float* p") and args[-1].endswith("stream") and "imdbn_cross_metrics_out" in args[10]
    assert [n for n, _ in native.CrossMetricsOut._fields_] == ["pred", "gt", "p_pred", "p_true", "rank", "acc", "confusion", "class_sums"]
    assert C.sizeof(native.CrossMetricsOut) == 8 * 8
    assert hasattr(native.lib(), "imdbn_cross_metrics")
    assert native.lib().imdbn_version() == native.ABI_VERSION == 4           # an additive export: the ABI version stays
    from imdbn.engine.hip_engine import HipEngine
    import inspect
    assert list(inspect.signature(HipEngine.cross_metrics).parameters) == ["self", "p", "y", "gt", "row_mse", "npix", "topk", "acc",
                                                                           "confusion", "class_sums"]


class _Counting:
    """An engine double that counts every attribute asked of it (any engine call starts with one)."""

    def __init__(self):
        object.__setattr__(self, "asked", [])

    def __getattr__(self, name):
        self.asked.append(name)
        raise AssertionError(f"engine.{name} was asked for")


class _Never:
    def uniform(self, shape):
        raise AssertionError("a draw was made")
    normal = categorical = uniform


def test_log_snapshots_without_a_run_does_nothing(fx):
    from imdbn import engine as E
    from imdbn.utils import cross_eval as CE
    stub = _Counting()
    E.set_engine_for_testing(stub)
    try:
        m = _small_model(fx)
        assert torch.equal(m.validation_images, torch.from_numpy(fx["imgs"]))
        assert stub.asked == []                                   # building the model calls no engine
        with E.use_rng(E.ReplayRng(_Never())):
            m.wandb_run = None
            assert CE.log_snapshots(m, epoch=1) is None and m._log_snapshots(1) is None
            m.wandb_run, keep = object(), m.validation_images
            m.validation_images = None
            assert CE.log_snapshots(m, epoch=1) is None
            m.validation_images, m.val_loader = keep, None
            assert CE.evaluate_cross_modal(m) is None and m.evaluate() is None
        assert stub.asked == []
    finally:
        E.set_engine_for_testing(None)


def _double():
    """tests/oracle_engine.OracleEngine plus the two calls cross_eval adds, through the numpy twin."""
    from oracle_engine import OracleEngine

    class Double(OracleEngine):
        calls = 0

        def decode_sqerr(self, idbn_layers, z, ref, ref_row=None, chunk=1024):
            cur = z
            for rbm in reversed(list(idbn_layers)):
                cur = self.prop_down(rbm, cur)
            return torch.from_numpy(CO.row_mse(cur.numpy(), ref.numpy()).astype(np.float32))

        def cross_metrics(self, p, y=None, gt=None, row_mse=None, npix=1, topk=3, acc=None, confusion=None, class_sums=None):
            type(self).calls += 1
            m = CO.metrics(p.numpy(), y=None if y is None else y.numpy(), gt=None if gt is None else gt.numpy(),
                           row_mse=None if row_mse is None else row_mse.numpy(), npix=npix, topk=topk)
            K = p.size(1)
            acc = torch.zeros(8, dtype=torch.float64) if acc is None else acc
            confusion = torch.zeros(K, K, dtype=torch.int64) if confusion is None else confusion
            class_sums = torch.zeros(K, 3, dtype=torch.float64) if class_sums is None else class_sums
            acc += torch.from_numpy(m["acc"]); confusion += torch.from_numpy(m["confusion"]); class_sums += torch.from_numpy(m["class_sums"])
            o = {k: torch.from_numpy(np.asarray(m[k]).astype(np.float32 if k.startswith("p_") else np.int32)) for k in
                 ("pred", "gt", "p_pred", "p_true", "rank")}
            o.update(acc=acc, confusion=confusion, class_sums=class_sums)
            return o

    return Double()


def test_host_logic_on_the_engine_double(fx):
    """log_snapshots and evaluate_cross_modal end to end on the CPU double: the recorded draws, the reference's numbers."""
    from imdbn import engine as E
    from imdbn.utils import cross_eval as CE
    eng = _double()
    E.set_engine_for_testing(eng)
    try:
        m = _small_model(fx, n_rows=21)
        m.wandb_run = Run()
        tape = Tape(fx)
        with E.use_rng(E.ReplayRng(tape)):
            s = m._log_snapshots(fx.meta["epoch"], fx.meta["num"])
        assert tape.done()
        assert list(s) == ["snap/image_mse", "confusion", "table", "pred", "gt"]
        assert np.array_equal(s["pred"], fx["cm_preds"]) and np.array_equal(s["gt"], fx["cm_y_true"])
        assert [row[:3] for row in s["table"]] == fx["table_int"].tolist() and all(len(row) == 5 for row in s["table"])
        assert np.abs(np.array([row[3:5] for row in s["table"]]) - fx["table_p"]).max() <= 1e-5
        _rel(s["snap/image_mse"], fx["snap_image_mse"], 1e-4, "snap/image_mse on the double")
        assert m.wandb_run.logged == [{"snap/image_mse": s["snap/image_mse"], "epoch": fx.meta["epoch"]}]
        m.class_names = [f"c{i}" for i in range(8)]
        with E.use_rng(E.ReplayRng(Tape(fx))):
            named = m._log_snapshots(0)
        assert named["table"][0][5:] == [f"c{fx['cm_y_true'][0]}", f"c{fx['cm_preds'][0]}"]
        # evaluate: batches of 8, 8, 5; a seed of its own leaves the ambient counter alone, no seed consumes it
        m.wandb_run = Run()
        E.manual_seed(3)
        before = E.get_rng().offset
        type(eng).calls = 0
        r = m.evaluate(seed=11)
        assert E.get_rng().offset == before and type(eng).calls == 3
        assert r["n"] == 21 == len(r["pred"]) == int(r["confusion"].sum()) == int(r["per_class_n"].sum())
        assert r["text_top1"] == float((r["pred"] == r["gt"]).mean()) == float((r["rank"] == 0).mean())
        assert r["text_top3"] == float((r["rank"] < 3).mean())
        assert sorted(m.wandb_run.logged[0]) == ["eval/image_mse", "eval/text_ce", "eval/text_top1", "eval/text_top3"]
        assert np.array_equal(r["per_class_acc"], CO.evaluate([(np.zeros((21, 100)), np.eye(8)[r["pred"]], np.zeros((21, 100)),
                                                                 np.eye(8)[r["gt"]])])["per_class_acc"], equal_nan=True)
        again = m.evaluate(seed=11)
        assert again["text_ce"] == r["text_ce"] and again["image_mse"] == r["image_mse"]
        two = m.evaluate(seed=11, max_batches=2)
        assert two["n"] == 16 and np.array_equal(two["pred"], r["pred"][:16])
        m.evaluate()
        assert E.get_rng().offset > before
        # the decoded-rows path gives the same image error
        z = m.image_idbn.represent(torch.from_numpy(fx["imgs"]))
        y, img = torch.from_numpy(fx["lbls"]), torch.from_numpy(fx["imgs"])
        with E.use_rng(E.PhiloxRng(5)):
            a, _ = CE.row_image_error(m, z, y, img, fused=True)
        with E.use_rng(E.PhiloxRng(5)):
            b, _ = CE.row_image_error(m, z, y, img, fused=False)
        _rel(a.numpy(), b.numpy(), 1e-5, "row_mse: decode_sqerr vs decoded rows")
        assert CE.fused_decode_ok(m)
        m.z_affine_scale, m.z_affine_bias = torch.ones(20), torch.zeros(20)
        assert not CE.fused_decode_ok(m)
    finally:
        E.set_engine_for_testing(None)
