"""``tests/tap_engine_double.TapOracleEngine`` plus ``HipEngine.dbm_layer`` / ``dbm_gibbs`` / ``dbm_infer`` / ``dbm_step`` (and the
stand-alone ``assoc_update`` they end in) on the fp32 twin of tests/dbm_oracle.py: the CPU suite runs the host logic of
``imdbn.models.dbm`` through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import dbm_oracle as Dt
import oracle.rbm_oracle as O
from oracle_engine import _Src, _np
from tap_engine_double import TapOracleEngine

F32 = np.float32


class DbmOracleEngine(TapOracleEngine):
    name = "oracle-test-double-dbm"

    def prop_down(self, rbm, h, T=1.0, logits_only=False):
        self.calls.append(("prop_down", tuple(h.shape)))
        return super().prop_down(rbm, h, T=T, logits_only=logits_only)

    def assoc_update(self, rbm, vpos, hpos, vneg, hneg, lr, mom):
        self._assoc(rbm, vpos, hpos, vneg, hneg, lr, mom, getattr(rbm, "sparsity", False))

    def _assoc(self, rbm, vpos, hpos, vneg, hneg, lr, mom, sparsity):
        self.calls.append(("assoc_update", tuple(vpos.shape), tuple(hpos.shape)))
        st = self._state(rbm, True)
        vp, hp, vn, hn = (_np(t) for t in (vpos, hpos, vneg, hneg))
        s = {"pos_assoc": (vp.T @ hp).astype(F32), "neg_assoc": (vn.T @ hn).astype(F32), "pos_h_sum": hp.sum(0, dtype=F32),
             "neg_h_sum": hn.sum(0, dtype=F32), "data_sum": vp.sum(0, dtype=F32), "v_sum": vn.sum(0, dtype=F32)}
        O.apply_cd_update(st, s, lr, mom, vp.shape[0], bool(sparsity))

    def dbm_layer(self, lo, hi, x_lo, x_hi, bias, m=None, damp=0.0, s_lo=1.0, s_hi=1.0, sample=False, rng=None, want_p=False,
                  want_res=False):
        return self._dbm_layer(lo, hi, x_lo, x_hi, bias, m, damp, s_lo, s_hi, sample, rng, want_p, want_res)

    def _dbm_layer(self, lo, hi, x_lo, x_hi, bias, m, damp, s_lo, s_hi, sample, rng, want_p, want_res, s_out=None):
        self.calls.append(("dbm_layer", lo is not None, hi is not None, bool(sample)))
        W_lo = None if lo is None else lo.W.data.numpy()
        W_hi = None if hi is None else hi.W.data.numpy()
        xl = None if lo is None else _np(x_lo)
        xh = None if hi is None else _np(x_hi)
        b = _np(bias.data if isinstance(bias, torch.nn.Parameter) else bias)
        if sample:
            p = Dt.sigmoid(Dt.pre(W_lo, xl, s_lo, W_hi, xh, s_hi, b, F32))
            src = _Src(rng)
            s = (p > src.uniform(p.shape)).astype(F32)
            src.done()
            smp = self._t(s)
            if s_out is not None:
                smp = s_out.copy_(smp)                         # in place, as the engine
            return (self._t(p), smp) if want_p else smp
        new, _, res = Dt.mean_field(W_lo, xl, s_lo, W_hi, xh, s_hi, b, _np(m), damp, F32)
        m.copy_(torch.from_numpy(new))                         # in place, as the engine
        return self._t(res) if want_res else None

    # the three compositions are the engine's own host code, run on this double's calls
    def dbm_gibbs(self, layers, biases, particles, n_sweeps, rng, clamp_bottom=None):
        from imdbn.engine.hip_engine import HipEngine
        self.calls.append(("dbm_gibbs", int(n_sweeps), clamp_bottom is not None))
        return HipEngine.dbm_gibbs(self, layers, biases, particles, n_sweeps, rng, clamp_bottom=clamp_bottom)

    def dbm_infer(self, layers, biases, v, n_mf, damp=0.0, init=None, want_res=True):
        from imdbn.engine.hip_engine import HipEngine
        self.calls.append(("dbm_infer", tuple(v.shape), int(n_mf), float(damp)))
        return HipEngine.dbm_infer(self, layers, biases, v, n_mf, damp=damp, init=init, want_res=want_res)

    def dbm_step(self, layers, data, particles, epoch_scalars, n_mf, damp, gibbs_k, rng, monitor=True):
        from imdbn.engine.hip_engine import HipEngine
        self.calls.append(("dbm_step", tuple(data.shape), int(n_mf), float(damp), int(gibbs_k), bool(monitor)))
        return HipEngine.dbm_step(self, layers, data, particles, epoch_scalars, n_mf, damp, gibbs_k, rng, monitor=monitor)

    @staticmethod
    def _dbm_check(who, layers, biases):
        from imdbn.engine.hip_engine import HipEngine
        return HipEngine._dbm_check(who, layers, biases)
