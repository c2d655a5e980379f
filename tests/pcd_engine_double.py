"""``tests/oracle_engine.OracleEngine`` plus the two persistent-chain calls of ``HipEngine`` (pcd_step, pt_sweep), on the twin of
tests/pcd_oracle.py: the CPU suite runs the host logic of ``RBM.train_epoch_persistent`` through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import pcd_oracle as T
from oracle_engine import OracleEngine, _Src, _np

F32 = np.float32


class PcdOracleEngine(OracleEngine):
    name = "oracle-test-double-pcd"

    def pcd_step(self, rbm, data, particles, lr, mom, cd_k, rng, data_binary=None, monitor=True):
        self.calls.append(("pcd_step", tuple(particles.shape), int(cd_k), bool(monitor)))
        st = self._state(rbm, True)
        s = _Src(rng)
        loss, v = T.pcd_step(st, _np(data), _np(particles), cd_k, s, lr, mom)
        s.done()
        particles.copy_(torch.from_numpy(v))                       # in place, as the engine
        return self._t(np.array(loss, F32)).reshape(()) if monitor else None

    def pt_sweep(self, rbm, state, betas, n_sweeps, rng, swap_try=None, swap_acc=None):
        self.calls.append(("pt_sweep", tuple(state.shape), len(betas), int(n_sweeps)))
        s = _Src(rng)
        v, tries, accs, _ = T.pt_sweep(self._state(rbm), _np(state), betas, n_sweeps, s)
        s.done()
        state.copy_(torch.from_numpy(v))
        n = max(len(betas) - 1, 1)
        swap_try = torch.zeros(n, dtype=torch.int64) if swap_try is None else swap_try
        swap_acc = torch.zeros(n, dtype=torch.int64) if swap_acc is None else swap_acc
        swap_try += torch.from_numpy(tries)
        swap_acc += torch.from_numpy(accs)
        return swap_try, swap_acc
