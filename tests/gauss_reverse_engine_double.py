"""``tests/gauss_engine_double.GaussOracleEngine`` plus ``HipEngine.gauss_reverse_ais`` on the float32 restatement of
tests/gauss_reverse_ais_oracle.py: the CPU suite runs the host logic of the Gaussian reverse-AIS functions (imdbn/utils/likelihood.py,
DESIGN §33) through it.  ``calls`` records ``("gauss_reverse_ais", rows, K, with base bias)``; ``last_margin`` is the twin's.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import gauss_reverse_ais_oracle as GR
from gauss_engine_double import GaussOracleEngine
from oracle_engine import _Src, _np

F32 = np.float32


class GaussReverseOracleEngine(GaussOracleEngine):
    name = "oracle-test-double-gauss-reverse"

    def gauss_reverse_ais(self, rbm, logvar, v_rows, betas, rng, base_vis_bias=None, return_state: bool = False):
        b = np.asarray(betas.tolist() if hasattr(betas, "tolist") else betas, F32)
        self.calls.append(("gauss_reverse_ais", int(v_rows.shape[0]), int(b.size - 1), base_vis_bias is not None))
        s = _Src(rng)
        logw, u1, self.last_margin = GR.gauss_reverse_ais_logw(_np(rbm.W.data), _np(rbm.vis_bias.data), _np(rbm.hid_bias.data), _np(logvar),
                                                               None if base_vis_bias is None else _np(base_vis_bias), b, _np(v_rows), s, dt=F32)
        s.done()
        lw = torch.from_numpy(np.ascontiguousarray(logw, np.float64))
        return (lw, self._t(u1)) if return_state else lw
