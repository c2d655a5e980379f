"""CPU-only: the engine contract (DESIGN "The engine contract").  ``HipEngine`` defines the calls the models and utils make; the
test doubles under tests/ follow it; the product never asks an engine what it can do.  This file holds the two sides together: a
renamed or re-shaped engine method fails here instead of selecting a fallback somewhere.

1. every public method a double defines that ``HipEngine`` also defines accepts the engine's parameters, by the same names, in
   the same order, with a default wherever the engine has one -- and none the engine lacks (``EXTRA_PARAMETERS``: empty);
2. every ``<engine>.<name>`` the model and utils modules reference exists on ``HipEngine``.  "<engine>" is: a call of ``_eng``,
   ``get_engine`` or ``get_hip_engine`` (``self._eng().chain(...)``), a name bound from such a call, and -- because an engine also
   travels as an argument (``RBM._negative_chains(eng, ...)``) -- any name spelt ``eng``;
3. no ``hasattr(eng`` / ``getattr(eng`` in the package."""
import ast
import glob
import importlib
import inspect
import os

import pytest

from imdbn.engine.hip_engine import HipEngine

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "multimodal-idbn_amd", "imdbn")

# a double class defined inside a function cannot be imported by name: how to get at it
NESTED = {("test_cross_eval_cpu", "Double"): lambda mod: type(mod._double())}
# (double class name, method, parameter) a double may take although the engine does not
EXTRA_PARAMETERS = set()


def _is_double(node: ast.ClassDef) -> bool:
    bases = [b.id if isinstance(b, ast.Name) else getattr(b, "attr", "") for b in node.bases]
    return node.name.endswith("OracleEngine") or any(b.endswith("Engine") for b in bases)


def _doubles():
    """Every engine double under tests/: a class named ``*OracleEngine`` or derived from a class named ``*Engine``."""
    out = []
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        mod = os.path.splitext(os.path.basename(path))[0]
        tree = ast.parse(open(path).read())
        top = {n.name for n in tree.body if isinstance(n, ast.ClassDef)}
        for node in ast.walk(tree):
            if isinstance(node, ast.ClassDef) and _is_double(node):
                if node.name in top:
                    out.append(getattr(importlib.import_module(mod), node.name))
                else:
                    assert (mod, node.name) in NESTED, f"{mod}.{node.name}: a nested engine double needs an entry in NESTED"
                    out.append(NESTED[(mod, node.name)](importlib.import_module(mod)))
    return out


DOUBLES = _doubles()


def _own_methods(cls):
    for name, v in vars(cls).items():
        if not name.startswith("_") and callable(getattr(cls, name)) and callable(getattr(HipEngine, name, None)):
            yield name


def test_the_doubles_are_found():
    names = {c.__name__ for c in DOUBLES}
    assert {"OracleEngine", "PcdOracleEngine", "UpDownOracleEngine", "BackpropOracleEngine", "DiscrimOracleEngine", "CenteredOracleEngine",
            "RetrievalOracleEngine", "LikelihoodOracleEngine", "PllOracleEngine", "LabelGradOracleEngine", "TracingOracleEngine",
            "Double"} <= names
    assert sum(1 for c in DOUBLES for _ in _own_methods(c)) > 40


@pytest.mark.parametrize("cls,name", [(c, n) for c in DOUBLES for n in _own_methods(c)], ids=lambda v: getattr(v, "__name__", v))
def test_a_double_takes_what_the_engine_takes(cls, name):
    P = inspect.Parameter
    eng = list(inspect.signature(getattr(HipEngine, name)).parameters.values())
    dbl = list(inspect.signature(getattr(cls, name)).parameters.values())
    assert not any(p.kind in (P.VAR_POSITIONAL, P.VAR_KEYWORD) for p in eng)
    open_ended = {P.VAR_POSITIONAL, P.VAR_KEYWORD} <= {p.kind for p in dbl}      # (self, rbm, *args, **kw): hands everything on
    named = [p for p in dbl if p.kind not in (P.VAR_POSITIONAL, P.VAR_KEYWORD)]
    extra = [p.name for p in named if p.name not in {q.name for q in eng}]
    assert all((cls.__name__, name, x) in EXTRA_PARAMETERS for x in extra), f"parameters the engine does not have: {extra}"
    named = [p for p in named if p.name not in extra]
    want = eng[:len(named)] if open_ended else eng
    assert [p.name for p in named] == [p.name for p in want], "names / order differ from HipEngine." + name
    for d, e in zip(named, want):
        assert d.kind == e.kind, f"{d.name}: {d.kind.description} here, {e.kind.description} in the engine"
        assert e.default is P.empty or d.default is not P.empty, f"{d.name}: the engine has a default, the double needs the argument"


_ENGINE_CALLS = ("_eng", "get_engine", "get_hip_engine")


def _is_engine_call(node) -> bool:
    if not isinstance(node, ast.Call):
        return False
    f = node.func
    return (f.attr if isinstance(f, ast.Attribute) else getattr(f, "id", None)) in _ENGINE_CALLS


def engine_references(path):
    """{attribute name: first line} of everything `path` reads off an engine (see the module docstring, 2)."""
    tree = ast.parse(open(path).read())
    bound = {"eng"}
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign):
            for tgt in node.targets:
                pairs = zip(tgt.elts, node.value.elts) if isinstance(tgt, ast.Tuple) and isinstance(node.value, ast.Tuple) else [(tgt, node.value)]
                bound |= {t.id for t, v in pairs if isinstance(t, ast.Name) and _is_engine_call(v)}
    refs = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and (_is_engine_call(node.value) or (isinstance(node.value, ast.Name) and node.value.id in bound)):
            refs.setdefault(node.attr, node.lineno)
    return refs


def _sources():
    return sorted(glob.glob(os.path.join(PKG, "models", "*.py")) + glob.glob(os.path.join(PKG, "utils", "*.py")))


def test_every_engine_call_of_the_models_and_utils_exists_on_the_engine():
    seen = set()
    for path in _sources():
        for name, line in engine_references(path).items():
            assert callable(getattr(HipEngine, name, None)), f"{os.path.relpath(path, PKG)}:{line}: HipEngine has no {name}"
            seen.add(name)
    # the scan sees the three spellings: a bound name, a direct call, an argument called eng
    assert {"cd_step", "forward", "binary_hint", "chain_pair", "cd_factors_wire", "apply_wire", "packed_buffer", "prop_down", "skip_draws",
            "pt_sweep", "updown_step", "pair_scores", "pseudo_loglik"} <= seen
    # and every one of them that the base double is asked for in the CPU suite is there (the subclass doubles add their own)
    from oracle_engine import OracleEngine
    rbm_calls = set(engine_references(os.path.join(PKG, "models", "rbm.py")))
    later = {"pcd_step", "pt_sweep", "centered_step", "label_step", "label_backprop_step"}          # pcd / centered / labelgrad / discrim doubles
    assert rbm_calls - later <= {n for n in dir(OracleEngine) if not n.startswith("_")}


def test_no_capability_probe_of_the_engine_is_left():
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)):
        text = open(path).read()
        assert "hasattr(eng" not in text and "getattr(eng" not in text, os.path.relpath(path, PKG)
    text = open(os.path.join(PKG, "engine", "hip_engine.py")).read()
    assert 'hasattr(self, "forward")' not in text and not hasattr(HipEngine, "fused_forward")
