"""``tests/oracle_engine.OracleEngine`` plus the ``HipEngine.gauss_*`` calls on the twin of tests/gauss_oracle.py in float32: the CPU
suite runs the host logic of ``GaussianRBM`` and of ``iDBN(GAUSSIAN_VISIBLE)`` through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import gauss_oracle as G
from oracle_engine import OracleEngine, _Src, _np

F32 = np.float32


class GaussOracleEngine(OracleEngine):
    name = "oracle-test-double-gauss"

    @staticmethod
    def _gstate(rbm, logvar, logvar_m=None, need_m=False):
        """A float32 twin state whose arrays ARE the tensors' memory: in-place updates reach the model."""
        if need_m:
            for nm, ref in (("W_m", rbm.W.data), ("hb_m", rbm.hid_bias.data), ("vb_m", rbm.vis_bias.data)):
                m = getattr(rbm, nm, None)
                if m is None or m.shape != ref.shape or m.device != ref.device:
                    setattr(rbm, nm, torch.zeros_like(ref))
        st = G.GState.__new__(G.GState)
        st.dt = F32
        st.W, st.b, st.c, st.z = rbm.W.data.numpy(), rbm.vis_bias.data.numpy(), rbm.hid_bias.data.numpy(), logvar.numpy()
        if need_m:
            st.W_m, st.vb_m, st.hb_m, st.z_m = rbm.W_m.numpy(), rbm.vb_m.numpy(), rbm.hb_m.numpy(), logvar_m.numpy()
        st.weight_decay, st.sparsity, st.target = rbm.weight_decay, bool(getattr(rbm, "sparsity", False)), getattr(rbm, "sparsity_factor", 0.0)
        return st

    def gauss_forward(self, rbm, logvar, v, T=1.0, sample=False, rng=None):
        self.calls.append(("gauss_forward", tuple(v.shape), bool(sample)))
        p = G.prop_up(self._gstate(rbm, logvar), _np(v), T)
        if sample:
            s = _Src(rng)
            h = (p > s.uniform(p.shape)).astype(F32)
            s.done()
            return self._t(p), self._t(h)
        return self._t(p)

    def gauss_backward(self, rbm, logvar, h, sample=False, rng=None):
        self.calls.append(("gauss_backward", tuple(h.shape), bool(sample)))
        st = self._gstate(rbm, logvar)
        m = G.prop_down(st, _np(h))
        if sample:
            s = _Src(rng)
            v = G.sample_visible(st, m, s)
            s.done()
            return self._t(m), self._t(v)
        return self._t(m)

    def gauss_sample_visible(self, rbm, logvar, mean, rng):
        self.calls.append(("gauss_sample_visible", tuple(mean.shape)))
        s = _Src(rng)
        v = G.sample_visible(self._gstate(rbm, logvar), _np(mean), s)
        s.done()
        return self._t(v)

    def gauss_free_energy(self, rbm, logvar, v):
        return self._t(G.free_energy(self._gstate(rbm, logvar), _np(v)))

    def gauss_cd_step(self, rbm, logvar, logvar_m, data, lr, mom, cd_k, rng, lr_z, z_lo=float("-inf"), z_hi=float("inf"),
                      sample_v=True, monitor=True):
        self.calls.append(("gauss_cd_step", tuple(data.shape), int(cd_k), bool(sample_v), float(lr_z), bool(monitor)))
        st = self._gstate(rbm, logvar, logvar_m, need_m=True)
        s = _Src(rng)
        loss = G.cd_step(st, _np(data), cd_k, s, lr, mom, lr_z, z_lo, z_hi, sample_v)
        s.done()
        return self._t(np.array(loss, F32)).reshape(()) if monitor else None
