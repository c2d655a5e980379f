"""``tests/updown_engine_double.UpDownOracleEngine`` plus the two backprop calls of ``HipEngine`` (backprop_step, autoencoder_step) on
the twin of tests/backprop_oracle.py: the CPU suite runs the host logic of ``iDBN.autoencoder_step`` / ``finetune_autoencoder`` through
it.  ``autoencoder_step`` IS the engine's method -- it is host logic over the other calls -- run on this double's calls.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import backprop_oracle as Bp
from imdbn.engine.hip_engine import HipEngine
from oracle_engine import _np
from updown_engine_double import UpDownOracleEngine


class BackpropOracleEngine(UpDownOracleEngine):
    name = "oracle-test-double-backprop"

    def backprop_step(self, rbm, up=None, down=None, lr=0.0, mom=0.0, apply=True, want_v=False, want_h=False):
        shape = lambda p: None if p is None else tuple(p[0].shape)
        self.calls.append(("backprop_step", shape(up), shape(down), bool(apply), bool(want_v), bool(want_h)))
        st = self._state(rbm, bool(apply))
        pair = lambda p: None if p is None else (_np(p[0]), _np(p[1]))
        out = Bp.backprop_step(st, pair(up), pair(down), lr, mom, apply)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        return (t(out["err_v"]) if want_v else None), (t(out["err_h"]) if want_h else None)

    def autoencoder_step(self, *args, **kw):
        self.calls.append(("autoencoder_step",))
        return HipEngine.autoencoder_step(self, *args, **kw)
