"""The CPU test double with ``exact_log_z``: what ``HipEngine.exact_log_z`` returns, from the float64 reference of exact_oracle.py."""
import numpy as np
import torch

import exact_oracle as X
from gauss_engine_double import GaussOracleEngine
from imdbn.engine.native import EngineError
from oracle_engine import _np


class ExactOracleEngine(GaussOracleEngine):
    name = "oracle-test-double-exact"

    def exact_log_z(self, rbm, logvar=None, side="auto", marginals=False, max_bits=24):
        groups = [(int(s), int(e)) for s, e in (getattr(rbm, "softmax_groups", None) or [])]
        W = _np(rbm.W.data)
        z = None if logvar is None else _np(logvar)
        if side not in ("auto", "hidden", "visible"):
            raise EngineError(f"exact_log_z: side must be 'auto', 'hidden' or 'visible', got {side!r}")
        name = X.sides(W, None, None, side, groups, z)[0]
        n = W.shape[1] if name == "hidden" else W.shape[0]
        self.calls.append(("exact_log_z", name, n, bool(marginals), logvar is not None))
        if n > int(max_bits):
            raise EngineError(f"exact_log_z: n = {n} units on the enumerated ({name}) side is above max_bits = {int(max_bits)}: "
                              f"2^{n} states; pass max_bits={n} to allow it (the library's limit is 30)")
        if name == "visible" and (groups or z is not None):
            raise EngineError("imdbn_rbm_exact_logz failed (rc=-5): exact_logz: the visible side cannot be enumerated with softmax "
                              "groups or Gaussian visibles")
        r = X.reference(W, _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), name, groups, z, marginals=marginals)
        f32 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float32))
        return {"log_z": torch.tensor(r["log_z"], dtype=torch.float64), "log_w_max": torch.tensor(r["log_w_max"], dtype=torch.float64),
                "side": name, "bits": n, "vis_mean": f32(r["vis_mean"]), "hid_mean": f32(r["hid_mean"])}
