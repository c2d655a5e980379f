"""``tests/oracle_engine.OracleEngine`` plus the ``HipEngine.gauss_*`` calls in float32 -- the twin of tests/gauss_oracle.py,
``gauss_ais`` on the restatement of tests/gauss_ais_oracle.py, ``gauss_bound_step`` on that of tests/gauss_bound_oracle.py -- and the
Bernoulli likelihood calls of ``tests/bound_oracle.LikelihoodOracleEngine`` (``bound_step``, ``ais``) for the layers above a Gaussian
one: the CPU suite runs the host logic of ``GaussianRBM``, of ``iDBN(GAUSSIAN_VISIBLE)`` and of the Gaussian likelihood functions
(imdbn/utils/likelihood.py) through it.  ``calls`` records the order of the bracket calls and of ``free_energy`` with
the shapes they saw.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import gauss_ais_oracle as GA
import gauss_bound_oracle as GB
import gauss_oracle as G
from bound_oracle import LikelihoodOracleEngine
from oracle_engine import _Src, _np

F32 = np.float32


class GaussOracleEngine(LikelihoodOracleEngine):
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

    def gauss_ais(self, rbm, logvar, betas, n_chains: int, rng, base_vis_bias=None, return_state: bool = False):
        b = np.asarray(betas.tolist() if hasattr(betas, "tolist") else betas, F32)
        self.calls.append(("gauss_ais", int(n_chains), int(b.size - 1), base_vis_bias is not None))
        s = _Src(rng)
        logw, v, _ = GA.gauss_ais_logw(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(logvar),
                                       None if base_vis_bias is None else _np(base_vis_bias), b, int(n_chains), s, dt=F32)
        s.done()
        lw = torch.from_numpy(np.ascontiguousarray(logw, np.float64))
        return (lw, self._t(v)) if return_state else lw

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
