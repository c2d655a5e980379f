"""Cases and pinned seeds of the centered-update tests (tests/test_centered_cpu.py, tests/test_centered_gpu.py).

The shapes, parameters, data and particles are those of tests/pcd_cases.py -- the smallest that reach each code path: `one` 8 x 4
with one row, `odd` 37 x 33 (scalar kernel, ragged stripes), `groups` 26 x 40 with a softmax group (float4 kernel), `h130` 20 x 130,
`rows67` 130 x 200 with 67 rows (two 64-row statistics passes), `wide` 1100 x 96 (V > 1024, the bit-plane positive phase).  Added
here: offsets on entry drawn uniformly in (0.05, 0.95), a slide per case out of {0, 0.01, 1} and the sparsity term in `h130`.

Seeds.  The persistent phases draw what pcd_cases' PCD steps draw, so their pinned seed serves; the CD phases get the first seed,
counting from 1, at which the twin's smallest Bernoulli margin |p - u| and its smallest categorical margin stay above
pcd_cases.MARGIN over a CD-CD_K pass.  `python tests/centered_cases.py` prints the first such seed next to the pinned one."""
import numpy as np

import pcd_cases as P

F32 = np.float32
CD_K = 1
PCD_KS = (0, 1, 2)
SPARSITY_TARGET = 0.1
# name -> (slide, sparsity, pinned seed of the CD phases)
EXTRA = {
    "odd": (0.01, False, 1),
    "groups": (0.0, False, 1),
    "h130": (0.01, True, 1),
    "rows67": (1.0, False, 1),
    "wide": (0.01, False, 1),
    "one": (1.0, False, 1),
}
assert list(EXTRA) == list(P.CASES)


def case(name):
    """pcd_cases.case plus mu [V], lam [H] (the offsets on entry), slide, sparsity, cd_seed."""
    c = P.case(name)
    g = np.random.Generator(np.random.PCG64(990 + list(P.CASES).index(name)))
    slide, sparsity, cd_seed = EXTRA[name]
    c.update(mu=(0.05 + 0.9 * g.random(c["V"])).astype(F32), lam=(0.05 + 0.9 * g.random(c["H"])).astype(F32), slide=slide,
             sparsity=sparsity, cd_seed=cd_seed)
    return c


def seed_of(c, kind):
    return c["cd_seed"] if kind == "cd" else c["seed"]


def twin_run(c, kind, cd_k, mode, seed=None, mu=None, lam=None, slide=None):
    """The twin on a case: kind "cd" (CD-cd_k from the data) or "pcd" (cd_k Gibbs steps on the particles).  dict(st: the oracle
    state after the step, loss, v: the particles after it (None for "cd"), mu, lam: the new offsets, offset: draws used, bern, cat:
    the smallest margins)."""
    import oracle.rbm_oracle as O
    import centered_oracle as Tc
    import pcd_oracle as T
    from oracle.draws import CATEGORICAL_MARGIN, PhiloxStream
    O.reset_margin()
    st = T.rbm_state(c, P.LR, P.WEIGHT_DECAY, P.MOM, sparsity=c["sparsity"], sparsity_factor=SPARSITY_TARGET)
    ps = PhiloxStream(seed_of(c, kind) if seed is None else seed)
    loss, v, mu2, lam2 = Tc.centered_step(st, c["data"], None if kind == "cd" else c["particles"], cd_k, ps, P.LR, P.MOM,
                                          c["mu"] if mu is None else mu, c["lam"] if lam is None else lam,
                                          c["slide"] if slide is None else slide, mode)
    return dict(st=st, loss=loss, v=v, mu=mu2, lam=lam2, offset=ps.offset, bern=O.BERNOULLI_MARGIN["min"], cat=CATEGORICAL_MARGIN["min"])


def margins_ok(t):
    return t["bern"] >= P.MARGIN and t["cat"] >= P.MARGIN


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in P.CASES:
        c = case(name)
        for seed in range(1, 65):
            t = twin_run(c, "cd", CD_K, 0, seed=seed)
            if margins_ok(t):
                break
        print(f"{name}: CD first seed {seed} (pinned {c['cd_seed']}), margins {t['bern']:.3g} / {t['cat']:.3g}")
        for k in PCD_KS:
            t = twin_run(c, "pcd", k, 0)
            print(f"   PCD-{k} under seed {c['seed']}: margins {t['bern']:.3g} / {t['cat']:.3g}")
