"""Shapes and pinned seeds of the up-down tests (tests/test_updown_cpu.py, tests/test_updown_gpu.py).

The stacks are the smallest at which the kernels can still go wrong: `odd` has unaligned weight rows, `h130` is four layers and
crosses a 128-unit chunk, `rows67` has more than 64 rows, `wide` takes the V > 1024 bit-plane route on a 0/1 batch, `one` is a single
row; `odd_real` is `odd` on data in (0, 1).  Parameters, momenta and data are made as pcd_cases.case makes them (LR, MOM, WEIGHT_DECAY
from there; non-zero starting momenta on every trained tensor); the generative twins get parameters of their own.

The Philox seed of a case is pinned on the CPU from the twin alone (tests/updown_oracle.py): the first seed, counting from 1, at
which every Bernoulli margin |p - u| of STEPS consecutive updown_steps stays above pcd_cases.MARGIN, with CD-1 from the wake state
and with persistent chains alike.  `python tests/updown_cases.py` prints the first such seed next to the pinned one."""
import numpy as np

from anneal_cases import params, start_rows
from pcd_cases import LR, MARGIN, MOM, WEIGHT_DECAY

F32 = np.float32
STEPS = 3
CD = 1

# name -> (layer sizes, batch, real-valued data, pinned seed)
CASES = {
    "odd": ((37, 33, 21), 5, False, 1),
    "h130": ((20, 130, 40, 12), 6, False, 1),
    "rows67": ((130, 200, 40), 67, False, 1),
    "wide": ((1100, 96, 24), 3, False, 1),
    "one": ((8, 4, 3), 1, False, 1),
    "odd_real": ((37, 33, 21), 5, True, 1),
}
SCALARS = (LR, MOM)


def _layer(V, H, gen_seed):
    W, b, c, _ = params(V, H, gen_seed, min(0.5, 1.5 / np.sqrt(V)))
    g = np.random.Generator(np.random.PCG64(gen_seed + 5))
    return dict(W=W, b=b, c=c, groups=[], W_m=(g.standard_normal((V, H)) * 0.01).astype(F32),
                hb_m=(g.standard_normal(H) * 0.01).astype(F32), vb_m=(g.standard_normal(V) * 0.01).astype(F32))


def case(name):
    """dict(name, sizes, B, seed, rec: L layer dicts (W, b, c, W_m, hb_m, vb_m, groups), gen: L - 1 of them, data [B, V_0])."""
    sizes, B, real, seed = CASES[name]
    idx = list(CASES).index(name) % 5          # odd_real shares odd's parameters
    rec = [_layer(sizes[l], sizes[l + 1], 2000 + 100 * idx + 10 * l) for l in range(len(sizes) - 1)]
    gen = [_layer(sizes[l], sizes[l + 1], 3000 + 100 * idx + 10 * l) for l in range(len(sizes) - 2)]
    if real:
        data = np.random.Generator(np.random.PCG64(75 + idx)).uniform(0.02, 0.98, (B, sizes[0])).astype(F32)
    else:
        data = start_rows(B, sizes[0], 70 + idx, (), p=0.3)
    return dict(name=name, sizes=sizes, B=B, seed=seed, rec=rec, gen=gen, data=data)


def states(c):
    """Fresh oracle states (rec, gen) of a case, with the cases' weight decay."""
    import pcd_oracle as P
    mk = lambda l: P.rbm_state(l, LR, WEIGHT_DECAY, MOM)
    return [mk(l) for l in c["rec"]], [mk(l) for l in c["gen"]]


def twin_run(c, seed, persistent):
    """STEPS consecutive twin updown_steps under Philox seed `seed`: dict(margin, steps: the per-step results, rec, gen: the final
    states, offset: the draws consumed)."""
    import oracle.rbm_oracle as O
    import updown_oracle as U
    from oracle.draws import PhiloxStream
    O.reset_margin()
    rec, gen = states(c)
    rng = PhiloxStream(seed)
    chains = {} if persistent else None
    steps = [U.updown_step(rec, gen, c["data"], [SCALARS] * len(rec), CD, rng, chains) for _ in range(STEPS)]
    return dict(margin=O.BERNOULLI_MARGIN["min"], steps=steps, rec=rec, gen=gen, offset=rng.offset)


def first_seed(c, limit=65):
    for seed in range(1, limit):
        m = min(twin_run(c, seed, p)["margin"] for p in (False, True))
        if m > MARGIN:
            return seed, m
    return None, m


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in CASES:
        c = case(name)
        seed, m = first_seed(c)
        print(f"{name}: first seed {seed} (pinned {c['seed']}), smallest margin {m:.3g}")
