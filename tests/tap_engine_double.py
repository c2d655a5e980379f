"""``tests/centered_engine_double.CenteredOracleEngine`` plus ``HipEngine.tap_iterate`` / ``tap_step`` on the fp32 twin of
tests/tap_oracle.py: the CPU suite runs the host logic of ``imdbn.utils.tap`` and of ``iDBN.train`` through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import tap_oracle as Tt
from centered_engine_double import CenteredOracleEngine
from oracle_engine import _np

F32 = np.float32


class TapOracleEngine(CenteredOracleEngine):
    name = "oracle-test-double-tap"

    def tap_iterate(self, rbm, mv, mh, n_iters, damp=0.5, order=2, want_gamma=True, want_res=True):
        self.calls.append(("tap_iterate", tuple(mv.shape), int(n_iters), float(damp), int(order)))
        st = self._state(rbm)
        v, h, res = Tt.iterate(st.W, st.vis_bias, st.hid_bias, _np(mv), _np(mh), n_iters, damp, order, F32)
        mv.copy_(torch.from_numpy(v))                          # in place, as the engine
        mh.copy_(torch.from_numpy(h))
        gamma = torch.from_numpy(Tt.gamma(st.W, st.vis_bias, st.hid_bias, v, h, order)) if want_gamma else None
        return gamma, (torch.from_numpy(np.asarray(res, F32)) if want_res else None)

    def tap_step(self, rbm, data, mv, mh, lr, mom, n_iters, damp=0.5, order=2, data_binary=None, monitor=True):
        self.calls.append(("tap_step", tuple(data.shape), int(n_iters), float(damp), int(order), bool(monitor)))
        st = self._state(rbm, True)
        loss, v, h = Tt.tap_step(st, _np(data), _np(mv), _np(mh), lr, mom, n_iters, damp, order)
        mv.copy_(torch.from_numpy(v))
        mh.copy_(torch.from_numpy(h))
        return self._t(np.array(loss, F32)).reshape(()) if monitor else None
