"""``tests/pcd_engine_double.PcdOracleEngine`` plus ``HipEngine.centered_step`` on the twin of tests/centered_oracle.py: the CPU
suite runs the host logic of ``RBM.train_epoch_centered`` and of ``iDBN.train`` through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import centered_oracle as Tc
from oracle_engine import _Src, _np
from pcd_engine_double import PcdOracleEngine

F32 = np.float32


class CenteredOracleEngine(PcdOracleEngine):
    name = "oracle-test-double-centered"

    def centered_step(self, rbm, data, particles, lr, mom, cd_k, rng, mu, lam, slide, mode, data_binary=None, monitor=True):
        self.calls.append(("centered_step", None if particles is None else tuple(particles.shape), int(cd_k), float(slide), int(mode), bool(monitor)))
        st = self._state(rbm, True)
        s = _Src(rng)
        loss, v, mu2, lam2 = Tc.centered_step(st, _np(data), None if particles is None else _np(particles), cd_k, s, lr, mom,
                                              _np(mu), _np(lam), slide, mode)
        s.done()
        if particles is not None:
            particles.copy_(torch.from_numpy(v))                   # in place, as the engine
        mu.copy_(torch.from_numpy(mu2))
        lam.copy_(torch.from_numpy(lam2))
        return self._t(np.array(loss, F32)).reshape(()) if monitor else None
