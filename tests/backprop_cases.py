"""Shapes and inputs of the backprop tests (tests/test_backprop_cpu.py, tests/test_backprop_gpu.py): the stacks of
tests/updown_cases.py -- `odd` (unaligned rows), `h130` (four layers, crosses a 128 chunk), `rows67` (more than 64 rows), `wide`
(V 1100: the bit-plane route on the 0/1 batch while the errors are real), `one` (a single row), `odd_real` -- with their parameters,
momenta and data.

The single-call tests feed a layer directly: error rows are signed normal values (PCG64, std 0.3), inputs uniform in (0.02, 0.98) so
that x (1 - x) is nowhere zero -- on a 0/1 input err_out would be all zeros and the test blind.  Nothing here draws on the device:
there are no seeds to pin and no Bernoulli margins."""
import numpy as np

from pcd_cases import LR, MOM, WEIGHT_DECAY  # noqa: F401  (re-exported)
from updown_cases import CASES, SCALARS, STEPS, case, states  # noqa: F401  (imported, not copied)

F32 = np.float32
E_STD = 0.3


def layer_io(c, li):
    """The inputs of a single backprop_step on directed layer `li` of case `c`: dict(l: the layer dict, x_v [B, V], e_h [B, H],
    x_h [B, H], e_v [B, V])."""
    l = c["rec"][li]
    V, H = l["W"].shape
    B = c["B"]
    g = np.random.Generator(np.random.PCG64(900 + 10 * li + list(CASES).index(c["name"])))
    u = lambda n: g.uniform(0.02, 0.98, (B, n)).astype(F32)
    e = lambda n: (g.standard_normal((B, n)) * E_STD).astype(F32)
    return dict(l=l, x_v=u(V), e_h=e(H), x_h=u(H), e_v=e(V))


def layers_of(name):
    """The directed layers a single-call test visits: the bottom one and the top one (the layers below the top RBM)."""
    n = len(CASES[name][0]) - 2
    return sorted({0, n - 1})


def twin_run(c):
    """STEPS consecutive twin autoencoder_steps: dict(steps: the per-step results, rec, gen: the final states)."""
    import backprop_oracle as Bp
    rec, gen = states(c)
    steps = [Bp.autoencoder_step(rec, gen, c["data"], [SCALARS] * len(rec)) for _ in range(STEPS)]
    return dict(steps=steps, rec=rec, gen=gen)
