"""``tests/gauss_engine_double.GaussOracleEngine`` plus ``HipEngine.gauss_ais`` on the float32 restatement of tests/gauss_ais_oracle.py:
the CPU suite runs the host logic of the Gaussian likelihood functions (imdbn/utils/likelihood.py) through it.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import gauss_ais_oracle as GA
from gauss_engine_double import GaussOracleEngine
from oracle_engine import _Src, _np

F32 = np.float32


class GaussAisOracleEngine(GaussOracleEngine):
    name = "oracle-test-double-gauss-ais"

    def gauss_ais(self, rbm, logvar, betas, n_chains: int, rng, base_vis_bias=None, return_state: bool = False):
        b = np.asarray(betas.tolist() if hasattr(betas, "tolist") else betas, F32)
        self.calls.append(("gauss_ais", int(n_chains), int(b.size - 1), base_vis_bias is not None))
        s = _Src(rng)
        logw, v, _ = GA.gauss_ais_logw(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(logvar),
                                       None if base_vis_bias is None else _np(base_vis_bias), b, int(n_chains), s, dt=F32)
        s.done()
        lw = torch.from_numpy(np.ascontiguousarray(logw, np.float64))
        return (lw, self._t(v)) if return_state else lw
