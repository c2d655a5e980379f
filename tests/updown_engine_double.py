"""``tests/pcd_engine_double.PcdOracleEngine`` plus the two up-down calls of ``HipEngine`` (delta_step, updown_step) and ``bound_step``
on the twins of tests/updown_oracle.py and tests/bound_oracle.py: the CPU suite runs the host logic of ``iDBN.untie`` /
``updown_step`` / ``finetune_updown`` and of the untied likelihood functions through it.  ``updown_step`` IS the engine's method -- it
is host logic over the other calls -- run on this double's calls.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import bound_oracle as B
import updown_oracle as U
from imdbn.engine.hip_engine import HipEngine
from oracle_engine import _Src, _np
from pcd_engine_double import PcdOracleEngine


class UpDownOracleEngine(PcdOracleEngine):
    name = "oracle-test-double-updown"

    def delta_step(self, rbm, direction, x, target, lr=0.0, mom=0.0, apply=True, rowlp=True):
        self.calls.append(("delta_step", direction, tuple(x.shape), bool(apply), bool(rowlp)))
        st = self._state(rbm, bool(apply))
        lp = U.delta_step(st, direction, _np(x), _np(target), lr if apply else None, mom)
        return torch.from_numpy(lp) if rowlp else None

    def bound_step(self, rbm, v, rng, acc=None, mode="entropy"):
        s = _Src(rng)
        st = self._state(rbm)
        a, h, _ = B.bound_step(st.W, st.vis_bias, st.hid_bias, _np(v), mode, s.p)
        s.done()
        a = torch.from_numpy(np.asarray(a, np.float64))
        return (a if acc is None else acc + a), self._t(h)

    def updown_step(self, *args, **kw):
        self.calls.append(("updown_step",))
        return HipEngine.updown_step(self, *args, **kw)
