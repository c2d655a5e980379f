"""``tests/gauss_engine_double.GaussOracleEngine`` plus the backprop calls a Gaussian-bottomed stack makes (``gauss_backprop_step``,
``gauss_autoencoder_step``, and ``backprop_step`` for the Bernoulli layers above) on the twins of tests/gauss_backprop_oracle.py and
tests/backprop_oracle.py: the CPU suite runs the host logic of ``iDBN.gaussian_autoencoder_step`` / ``finetune_gaussian_autoencoder``
through it.  ``gauss_autoencoder_step`` IS the engine's method -- host logic over the other calls -- run on this double's calls.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import backprop_oracle as Bp
import gauss_backprop_oracle as Go
from gauss_engine_double import GaussOracleEngine
from imdbn.engine.hip_engine import HipEngine
from oracle_engine import _np


class GaussBackpropOracleEngine(GaussOracleEngine):
    name = "oracle-test-double-gauss-backprop"

    def backprop_step(self, rbm, up=None, down=None, lr=0.0, mom=0.0, apply=True, want_v=False, want_h=False):
        shape = lambda p: None if p is None else tuple(p[0].shape)
        self.calls.append(("backprop_step", shape(up), shape(down), bool(apply), bool(want_v), bool(want_h)))
        pair = lambda p: None if p is None else (_np(p[0]), _np(p[1]))
        out = Bp.backprop_step(self._state(rbm, bool(apply)), pair(up), pair(down), lr, mom, apply)
        return (self._t(out["err_v"]) if want_v else None), (self._t(out["err_h"]) if want_h else None)

    def gauss_backprop_step(self, rbm, logvar, logvar_m, data, up=None, down=None, lr=0.0, mom=0.0, lr_z=0.0, z_lo=float("-inf"),
                            z_hi=float("inf"), apply=True, want_h=False, monitor=False):
        shape = lambda p: None if p is None else tuple(p.shape)
        self.calls.append(("gauss_backprop_step", shape(up), shape(down), bool(apply), bool(want_h), bool(monitor), float(lr_z)))
        st = self._gstate(rbm, logvar, logvar_m, need_m=bool(apply))
        st.sparsity = False
        arr = lambda p: None if p is None else _np(p)
        out = Go.gauss_backprop_step(st, _np(data), arr(up), arr(down), lr, mom, lr_z if apply else 0.0, z_lo, z_hi, apply)
        s = lambda x: torch.from_numpy(np.array(x, np.float32)).reshape(())
        return (self._t(out["err_h"]) if want_h else None), (s(out["nll"]) if monitor else None), (s(out["mse"]) if monitor else None)

    def gauss_autoencoder_step(self, *args, **kw):
        self.calls.append(("gauss_autoencoder_step",))
        return HipEngine.gauss_autoencoder_step(self, *args, **kw)
