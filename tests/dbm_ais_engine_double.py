"""``tests/dbm_engine_double.DbmOracleEngine`` plus ``HipEngine.dbm_rowsum_layer`` / ``dbm_ais`` / ``dbm_bound`` on the fp32 twin of
tests/dbm_ais_oracle.py: the CPU suite runs the host logic of ``imdbn.utils.likelihood``'s DBM functions through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import dbm_ais_oracle as At
from dbm_engine_double import DbmOracleEngine
from oracle_engine import _Src, _np

F32 = np.float32


class DbmAisOracleEngine(DbmOracleEngine):
    name = "oracle-test-double-dbm-ais"

    def dbm_rowsum_layer(self, lo, hi, x_lo, x_hi, bias, mode, acc=None, beta=1.0, beta_prev=0.0, dbeta_next=0.0, base=None, mu=None,
                         sample=True, rng=None, want_p=False, s_out=None):
        self.calls.append(("dbm_rowsum_layer", mode, lo is not None, hi is not None))
        W_lo = None if lo is None else lo.W.data.numpy()
        W_hi = None if hi is None else hi.W.data.numpy()
        xl = None if lo is None else _np(x_lo)
        xh = None if hi is None else _np(x_hi)
        b = _np(bias.data if isinstance(bias, torch.nn.Parameter) else bias)
        a = None if base is None else _np(base)
        B = (xl if xl is not None else xh).shape[0]
        add = np.zeros(B)
        smp = p = None
        if mode == "bound":
            add = At.bound_layer(W_lo, xl, b, _np(mu), F32, bias_lo=a)
        if mode == "weigh":
            add = At.weigh(W_lo, xl, W_hi, xh, b, beta, beta_prev, a, F32)
        if mode == "sample" or (mode == "weigh" and sample):
            pr = At.sample_p(W_lo, xl, W_hi, xh, b, beta, a, F32)
            src = _Src(rng)
            s = (pr > src.uniform(pr.shape)).astype(F32)
            src.done()
            smp = self._t(s) if s_out is None else s_out.copy_(self._t(s))
            p = self._t(pr) if want_p else None
            if mode == "sample":
                add = float(dbeta_next) * At.bias_dot(b, s)
        if acc is None and mode != "sample":
            acc = torch.zeros(B, dtype=torch.float64)
        if acc is not None:
            acc += torch.from_numpy(add)
        return acc, smp, p

    def dbm_ais(self, layers, biases, betas, n_chains, rng, base_bias=None, return_state=False):
        self._dbm_check("dbm_ais", layers, biases)
        self.calls.append(("dbm_ais", int(n_chains), len(betas) - 1, base_bias is not None))
        Ws = [r.W.data.numpy() for r in layers]
        bs = [_np(b.data if isinstance(b, torch.nn.Parameter) else b) for b in biases]
        src = _Src(rng)
        logw, s = At.ais(Ws, bs, _np(torch.as_tensor(betas)), int(n_chains), src, None if base_bias is None else _np(base_bias), F32)
        src.done()
        logw = torch.from_numpy(logw)
        return (logw, [self._t(x) for x in s[1::2]]) if return_state else logw

    def dbm_bound(self, layers, biases, v, mus):
        from imdbn.engine.hip_engine import HipEngine
        self.calls.append(("dbm_bound", tuple(v.shape)))
        return HipEngine.dbm_bound(self, layers, biases, v, mus)
