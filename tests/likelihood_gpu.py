"""What the GPU tests of the likelihood family share: the engine fixtures, RBMs and tensors on the device, the closeness check and
a cache of twin results.

TEST INFRASTRUCTURE ONLY.  A test module imports ``_native`` and ``eng`` by name, so that ``_native`` is autouse in that module."""
import numpy as np
import pytest
import torch

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    E.set_engine_for_testing(None)
    yield E.get_hip_engine()


@pytest.fixture(scope="module")
def eng(_native):
    return _native


def device_rbm(c, pitch=None, groups=None):
    """The RBM of a case dict, or of (W, b, c) arrays, on the device.  `pitch`: weight rows that many floats apart (None: the
    case's, else the constructor's padded pitch); `groups`: the softmax groups (None: the case's)."""
    from imdbn.models import RBM
    if not isinstance(c, dict):
        c = dict(zip("Wbc", c))
    V, H = c["W"].shape
    pitch = c.get("pitch") if pitch is None else pitch
    groups = c.get("groups") if groups is None else groups
    r = RBM(V, H, 0.1, 0.0, 0.5, softmax_groups=groups or None).to(DEV)
    if pitch is not None:
        r.W.data = torch.empty(V, pitch, device=DEV)[:, :H]
    r.W.data.copy_(torch.from_numpy(c["W"]))
    r.vis_bias.data.copy_(torch.from_numpy(c["b"]))
    r.hid_bias.data.copy_(torch.from_numpy(c["c"]))
    return r


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def base_bias(c):
    return None if c["bA"] is None else dev(c["bA"])


def close(got, want, tol, what):
    """|got - want| <= tol elementwise, the largest error printed first."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = np.broadcast_to(tol, want.shape)
    err = np.abs(got - want)
    print(f"{what}: max |device - twin| {np.nanmax(err):.3g} (tolerance {tol.min():.3g})")
    assert (err <= tol).all(), f"{what}: {np.nanmax(err):.3g}"


_TWIN = {}


def twin(key, compute):
    """compute() once per key: the twin's result of a pinned case, shared by the tests of a run and left unchanged."""
    if key not in _TWIN:
        _TWIN[key] = compute()
    return _TWIN[key]
