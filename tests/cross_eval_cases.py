"""Shared by test_cross_eval_cpu.py and test_cross_eval_gpu.py: the small model over the fixture's validation order, the replay of
the fixture's recorded draws, a stub run."""
import os

import numpy as np
import torch

from golden_utils import GOLDEN


def small_model(fx, dev="cpu", n_rows=None):
    """The project's iMDBN with the weights of ref_imdbn_small.pkl over the fixture's validation order."""
    import trace_oracle as TO
    from imdbn.models import iMDBN
    from torch.utils.data import DataLoader, TensorDataset
    _, X, Y = TO.small_model_arrays()
    perm = fx["perm"][:n_rows] if n_rows else fx["perm"]
    dl = DataLoader(TensorDataset(torch.from_numpy(X[perm]), torch.from_numpy(Y[perm])), batch_size=fx.meta["batch"], shuffle=False)
    mt = fx.meta
    m = iMDBN(mt["sizes"], mt["joint_hidden"], params=dict(mt["params"]), dataloader=dl, val_loader=dl, device=torch.device(dev),
              num_labels=mt["K"])
    pl = iMDBN.load_model(os.path.join(GOLDEN, "ref_imdbn_small.pkl"), device=torch.device(dev))
    m.image_idbn.layers = pl["image_idbn"].layers
    m.joint_rbm = pl["joint_rbm"]
    m.z_class_mean = pl["z_class_mean"].to(dev)
    return m


class Tape:
    """The fixture's recorded draws, handed out in order; kind and shape of every request must be the recorded ones."""

    def __init__(self, fx):
        self.log, self.flat, self.i, self.at = fx.meta["draw_log"], fx["draws"], 0, 0

    def _next(self, kind, shape):
        want_kind, want_shape = self.log[self.i]
        assert (kind, list(shape)) == (want_kind, want_shape), (self.i, kind, shape, want_kind, want_shape)
        n = int(np.prod(shape))
        out = self.flat[self.at:self.at + n].reshape(shape)
        self.i, self.at = self.i + 1, self.at + n
        return out

    def uniform(self, shape):
        return self._next("u", tuple(int(s) for s in shape))

    def normal(self, shape):
        return self._next("n", tuple(int(s) for s in shape))

    def done(self):
        return self.i == len(self.log) and self.at == len(self.flat)


class Run:
    def __init__(self):
        self.logged = []

    def log(self, d):
        self.logged.append(d)
