"""``tests/gauss_ais_engine_double.GaussAisOracleEngine`` plus ``HipEngine.gauss_bound_step`` on the float32 restatement of
tests/gauss_bound_oracle.py, and the Bernoulli likelihood calls of ``tests/bound_oracle.LikelihoodOracleEngine`` (``bound_step``,
``ais``) for the layers above: the CPU suite runs the host logic of the Gaussian stack bounds (imdbn/utils/likelihood.py)
through it.  ``calls`` records the order of the bracket calls and of ``free_energy`` with the shapes they saw.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import gauss_bound_oracle as GB
from bound_oracle import LikelihoodOracleEngine
from gauss_ais_engine_double import GaussAisOracleEngine
from oracle_engine import _Src, _np

F32 = np.float32


class GaussBoundOracleEngine(GaussAisOracleEngine, LikelihoodOracleEngine):
    name = "oracle-test-double-gauss-bound"

    def gauss_bound_step(self, rbm, logvar, v, rng, acc=None, mode="entropy"):
        self.calls.append(("gauss_bound_step", tuple(v.shape), mode))
        s = _Src(rng)
        a, h, self.last_margin, _, _ = GB.gauss_bound_step(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(logvar),
                                                           _np(v), mode, s, dt=F32)
        s.done()
        a = torch.from_numpy(np.ascontiguousarray(a, np.float64))
        if acc is None:
            acc = a
        else:
            acc += a
        return acc, self._t(h)

    def bound_step(self, rbm, v, rng, acc=None, mode="entropy"):
        self.calls.append(("bound_step", tuple(v.shape), mode))
        return LikelihoodOracleEngine.bound_step(self, rbm, v, rng, acc=acc, mode=mode)

    def free_energy(self, rbm, v):
        self.calls.append(("free_energy", tuple(v.shape)))
        return LikelihoodOracleEngine.free_energy(self, rbm, v)
