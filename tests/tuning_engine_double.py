"""Engine double with HipEngine.unit_moments: the base double plus the numpy moments of tests/tuning_oracle.py, so that
imdbn.utils.unit_tuning and the models' unit_tuning run on a CPU-only machine."""
import torch

import tuning_oracle as TO
from oracle_engine import OracleEngine


class TuningOracleEngine(OracleEngine):
    def unit_moments(self, act, cls=None, n_classes=0, x=None, acc=None):
        B, H = act.shape
        K = int(n_classes) if cls is not None else 0
        xs = None if x is None else x.detach().cpu().float().reshape(B, -1).numpy()
        m = TO.unit_moments(act.detach().cpu().float().numpy(), None if cls is None else cls.detach().cpu().numpy(), K, xs)
        new = {k: torch.from_numpy(m[k]) for k in TO.KEYS}
        if acc is None:
            return new
        for k in TO.KEYS:
            if acc[k].shape != new[k].shape or acc[k].dtype != new[k].dtype:
                raise ValueError(f"unit_moments: acc[{k!r}] is {tuple(acc[k].shape)} {acc[k].dtype}, this call needs "
                                 f"{tuple(new[k].shape)} {new[k].dtype}")
            acc[k] += new[k]
        return acc
