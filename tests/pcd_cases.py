"""Shapes and pinned seeds of the persistent-chain tests (tests/test_pcd_cpu.py, tests/test_pcd_gpu.py).

(V, H, M, R, groups) sit at the edges of the exchange kernel (kernels_pt.hpp: one wave per (pair, chain), four per block, hidden
units in chunks of 128) and of the propagation routes: `odd` has unaligned weight rows, `h130` crosses a 128-unit chunk, `rows67`
has more than 64 rows per replica (its 134 rows span several 64-row chunks), `wide` is the V > 1024 bit-plane route, `one` is a
single chain without an exchange.

The Philox seeds are pinned on the CPU from the twin alone (tests/pcd_oracle.py): the first seed, counting from 1, at which over
SWEEPS sweeps and over a PCD step of CD_MAX Gibbs steps the twin's smallest Bernoulli margin |p - u| and its smallest categorical
margin stay above MARGIN, its smallest exchange margin |log U - Delta| stays above 8 H 1e-5 (twice the sum of the four softplus
sums' bounds under the project's eps = H 1e-5 convention: no decision is a near tie), and every case with R >= 2 both accepts and
rejects an exchange.  `python tests/pcd_cases.py` prints, for every case, the first such seed next to the pinned one."""
import numpy as np

from anneal_cases import params, start_rows

F32 = np.float32
MARGIN = 1e-6
SWEEPS = 3
CD_MAX = 2
LR, MOM, WEIGHT_DECAY = 0.05, 0.9, 1e-4

# name -> (V, H, M, R, groups, weight scale, pinned seed)
CASES = {
    "odd": (37, 33, 5, 3, (), 0.5, 1),
    "groups": (26, 40, 4, 4, ((20, 26),), 0.5, 1),
    "h130": (20, 130, 6, 2, (), 0.4, 1),
    "rows67": (130, 200, 67, 2, (), 0.1, 1),
    "wide": (1100, 96, 3, 2, (), 0.05, 18),
    "one": (8, 4, 1, 1, (), 1.0, 1),
}
LADDERS = {1: (1.0,), 2: (0.6, 1.0), 3: (0.4, 0.7, 1.0), 4: (0.3, 0.5, 0.75, 1.0)}


def exchange_margin(H):
    return 8 * H * 1e-5


def case(name):
    """dict(V, H, M, R, groups, W, b, c, W_m, hb_m, vb_m, betas, state [R M, V], data [M, V], particles [M, V], seed)."""
    V, H, M, R, groups, scale, seed = CASES[name]
    idx = list(CASES).index(name)
    W, b, c, _ = params(V, H, 900 + 10 * idx, scale)
    g = np.random.Generator(np.random.PCG64(950 + idx))
    groups = [tuple(x) for x in groups]
    return dict(name=name, V=V, H=H, M=M, R=R, groups=groups, W=W, b=b, c=c, seed=seed,
                W_m=(g.standard_normal((V, H)) * 0.01).astype(F32), hb_m=(g.standard_normal(H) * 0.01).astype(F32),
                vb_m=(g.standard_normal(V) * 0.01).astype(F32), betas=np.asarray(LADDERS[R], F32),
                state=start_rows(R * M, V, 60 + idx, groups), data=start_rows(M, V, 70 + idx, groups, p=0.3),
                particles=start_rows(M, V, 80 + idx, groups))


def twin_run(c, seed):
    """The twin on a case under Philox seed `seed`: dict(bern, cat, exch: the three smallest margins; tries, accs; state: after
    SWEEPS sweeps; pcd: {cd_k: (oracle state, loss, particles)} for cd_k = 0 .. CD_MAX)."""
    import oracle.rbm_oracle as O
    import pcd_oracle as T
    from oracle.draws import CATEGORICAL_MARGIN, PhiloxStream
    O.reset_margin()
    state, tries, accs, exch = T.pt_sweep(T.rbm_state(c), c["state"], c["betas"], SWEEPS, PhiloxStream(seed))
    pcd = {}
    for k in range(CD_MAX + 1):
        st = T.rbm_state(c, LR, WEIGHT_DECAY, MOM)
        loss, v = T.pcd_step(st, c["data"], c["particles"], k, PhiloxStream(seed), LR, MOM)
        pcd[k] = (st, loss, v)
    return dict(bern=O.BERNOULLI_MARGIN["min"], cat=CATEGORICAL_MARGIN["min"], exch=exch, tries=tries, accs=accs, state=state, pcd=pcd)


def seed_ok(c, t):
    both = c["R"] < 2 or (t["accs"].sum() > 0 and (t["tries"] - t["accs"]).sum() > 0)
    return t["bern"] > MARGIN and t["cat"] > MARGIN and t["exch"] > exchange_margin(c["H"]) and both


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in CASES:
        c = case(name)
        for seed in range(1, 65):
            t = twin_run(c, seed)
            if seed_ok(c, t):
                break
        print(f"{name}: first seed {seed} (pinned {c['seed']}), margins {t['bern']:.3g} / {t['cat']:.3g} / {t['exch']:.3g} "
              f"(needs {exchange_margin(c['H']):.3g}), accepted {t['accs'].tolist()} of {t['tries'].tolist()}")
