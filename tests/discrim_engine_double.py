"""``tests/backprop_engine_double.BackpropOracleEngine`` plus the two discriminative calls of ``HipEngine`` (label_backprop_step,
discriminative_step) on the twin of tests/discrim_oracle.py: the CPU suite runs the
host logic of ``RBM.label_backprop`` / ``iMDBN.discriminative_step`` / ``finetune_discriminative`` through it.
``discriminative_step`` IS the engine's method -- it is host logic over the other calls -- run on this double's calls.

TEST INFRASTRUCTURE ONLY."""
import numpy as np
import torch

import discrim_oracle as D
from backprop_engine_double import BackpropOracleEngine
from imdbn.engine.hip_engine import HipEngine
from oracle_engine import _np


class DiscrimOracleEngine(BackpropOracleEngine):
    name = "oracle-test-double-discriminative"

    def label_backprop_step(self, rbm, z, K, gt, lr=0.0, mom=0.0, apply=True, want_pred=False):
        self.calls.append(("label_backprop_step", tuple(z.shape), int(K), float(lr), float(mom), bool(apply), bool(want_pred)))
        x = self._state(rbm, bool(apply))
        st = dict(W=x.W, b=x.vis_bias, c=x.hid_bias, Wm=x.W_m, bm=x.vb_m, cm=x.hb_m)
        out, new = D.label_backprop_step(st, _np(z), int(K), gt.cpu().numpy(), lr, mom, float(rbm.weight_decay), bool(apply))
        if apply:
            for k, arr in st.items():
                arr[...] = new[k].astype(np.float32)
        return (torch.from_numpy(out["logp"]), torch.from_numpy(np.ascontiguousarray(out["err_z"], dtype=np.float32)),
                torch.from_numpy(out["pred"].astype(np.int32)) if want_pred else None)

    def discriminative_step(self, *args, **kw):
        self.calls.append(("discriminative_step",))
        return HipEngine.discriminative_step(self, *args, **kw)
