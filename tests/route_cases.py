"""Cases shared by test_routes_cpu.py and test_routes_gpu.py: single propagations, Gibbs steps, wide-layer chains and the clamped
update on every kernel route of prop() (csrc/host_prop.hpp), each naming the route it must take as HipEngine.last_route() reports it.

Parameters come from fixed PCG64 generators (W ~ N(0, 1) / sqrt(V), biases ~ 0.1 N(0, 1), as _mk of test_parity_gpu.py).  The shapes
are the smallest that still cross the edge a route depends on:

  130 x 70    gemm_up_fused with ragged tiles;  130 x 72: the same with float4 weight rows (k2_stream behind it)
  130 x 36    k1_stream with ONE K slice (no_fused_up; Vpad / 192 = 0 clamps the slice count to 1), second 32-column tile ragged
  1040 x 36   smallest Vpad > 1024: k1_stream with 5 slices of 256 rows, the last one short (last-arriver combine); with no_k1s
              gemm_up4_partial + finish; down: gemm_down_fused with float4 rows
  1040 x 37   H % 4 != 0: the scalar-row kernels on both sides (gemm_up_partial + finish, gemm_down_fused)
  4100 x 72   smallest V with Vpad >= 4096 (its last 128-row tile holds 4 real rows): gemm_down_tiled, and with no_down_tiled the
              gemm_down_fused forms that take 2 / 4 batch chunks per block
  1089 x 36   a wide joint layer with 14 labels in one softmax group at the end: chains run one launch per half step

Which epilogue a launch runs ("lean" / "general" in last_route()) is what the launcher passes to the kernel: the streaming kernels
(k1_stream, k2_stream) are lean at T = 1 with nothing sampled or written besides the probabilities; every other kernel branches on
FinishArgs::simple (T = 1, no noise, no mu-pull, no clamp, no softmax group, no raw logits), whether or not it samples.

Every Philox seed is pinned on the CPU with the oracle alone (`python tests/route_cases.py` prints the table): the first seed for
which the oracle's smallest Bernoulli margin |p - u| and its smallest categorical margin are both at least MARGIN, so that the
device must take every decision as the references do.  test_routes_cpu.py asserts that; a seed that fails is replaced, never skipped."""
import functools

import numpy as np

import oracle.rbm_oracle as O
from oracle.draws import CATEGORICAL_MARGIN, PhiloxStream

F32 = np.float32
MARGIN = 1e-6
TEMPS = (1.0, 0.7, 3.0)
STREAMS = ("stream_bits", "stream_real", "k2_stream")       # kernels with an epilogue instantiation of their own (finish_lean)
UP_ROUTES = ("fused", "stream_bits", "stream_real", "partial4", "partial")
DOWN_ROUTES = ("k2_stream", "down_fused", "down_chunks2", "down_chunks4", "down_tiled")


def prob_bound(T):
    """|p - float64 reference|: 5e-7 is the bound of test_products_are_fp32_exact at K = 2000 (these K are smaller); the logit error is
    divided by T and the slope of the sigmoid is at most 1/4."""
    return 5e-7 * max(1.0, 1.0 / T)


def logit_bound(ref_untempered, T):
    """|logits - float64 reference| of raw logits: the bound of test_products_are_fp32_exact, divided by T with the logits."""
    return (2e-5 * float(np.abs(ref_untempered).max()) + 2e-6) / T


# ---- parameters and operands ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def params(V, H):
    g = np.random.Generator(np.random.PCG64(7 * V + H))
    W = (g.standard_normal((V, H), dtype=F32) / F32(np.sqrt(V))).astype(F32)
    hb = (g.standard_normal(H, dtype=F32) * F32(0.1)).astype(F32)
    vb = (g.standard_normal(V, dtype=F32) * F32(0.1)).astype(F32)
    for a in (W, hb, vb):
        a.setflags(write=False)
    return W, hb, vb


def state(V, H, groups=(), W=None):
    W0, hb, vb = params(V, H)
    W = W0 if W is None else W
    return O.RBMState.create(W, 0.1, 1e-4, 0.5, dynamic_lr=True, final_momentum=0.95, softmax_groups=list(groups), hid_bias=hb, vis_bias=vb)


@functools.lru_cache(maxsize=None)
def operand(kind, B, N):
    """[B, N] fp32: "real" in [0, 1); "binary" 0/1; "mixed" 0/1 in columns [0, N/2) and real elsewhere (the exactness map then has
    one-term and three-term 64-column items and one that straddles)."""
    g = np.random.Generator(np.random.PCG64(1000 * B + N))
    x = g.random((B, N), dtype=F32)
    if kind == "binary":
        x = (x > 0.6).astype(F32)
    elif kind == "mixed":
        x[:, : N // 2] = (x[:, : N // 2] > 0.6)
    else:
        assert kind == "real", kind
    x.setflags(write=False)
    return x


def sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x))


@functools.lru_cache(maxsize=None)
def _up_logits64(V, H, kind, B):
    W, hb, _ = params(V, H)
    return operand(kind, B, V).astype(np.float64) @ W.astype(np.float64) + hb.astype(np.float64)


def case_params(c):
    """(W, hb, vb) of a case: params(V, H), with the weights the case carries under "W" in their place (rowoffset_cases.py: the bf16
    weights of FAST mode)."""
    W, hb, vb = params(c["V"], c["H"])
    return c.get("W", W), hb, vb


def _case_up_logits64(c):
    if "W" not in c:
        return _up_logits64(c["V"], c["H"], c["operand"], c["B"])
    W, hb, _ = case_params(c)
    return operand(c["operand"], c["B"], c["V"]).astype(np.float64) @ W.astype(np.float64) + hb.astype(np.float64)


def case_stream(c):
    """The PhiloxStream of a case: its seed, keyed from global row c["row0"] (0 where the case names none)."""
    return PhiloxStream(c["seed"], row0=c.get("row0", 0))


def _down64(W, vb, h):
    return np.asarray(h, np.float64) @ W.astype(np.float64).T + vb.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _down_logits64(V, H, B):
    W, _, vb = params(V, H)
    return _down64(W, vb, operand("real", B, H))


def probs64(logits, T, groups):
    """sigmoid(logits / max(1e-6, T)) with softmax over the groups, float64."""
    l = logits / max(1e-6, T)
    p = sigmoid64(l)
    for s, e in groups:
        z = np.exp(l[:, s:e] - l[:, s:e].max(axis=1, keepdims=True))
        p[:, s:e] = z / z.sum(axis=1, keepdims=True)
    return p


def _lean(route, simple, nothing_else):
    """The epilogue name last_route() must report: `simple` = FinishArgs::simple, `nothing_else` = the streaming kernels' further
    conditions (no sample / final output besides the probabilities, no operand form written)."""
    return "lean" if (simple and (nothing_else or route not in STREAMS)) else "general"


# ---- up steps (eng.prop_up; eng.forward for the asserted-0/1 bit plane) -----------------------------------------------------------
UP_SHAPES = [    # route, V, H, options
    ("fused", 130, 70, {}),
    ("stream_real", 130, 36, {"no_fused_up": 1}),
    ("stream_real", 1040, 36, {}),
    ("partial4", 1040, 36, {"no_k1s": 1}),
    ("partial", 1040, 37, {}),
]
BATCHES = (1, 33, 130)      # 130: three 64-row chunks, the last one ragged
OPERANDS = ("real", "binary", "mixed")


def up_cases():
    out = []
    for route, V, H, opts in UP_SHAPES:
        for i, (T, sample) in enumerate((T, s) for s in (False, True) for T in TEMPS):
            B, kind = BATCHES[i % 3], OPERANDS[(i + i // 3) % 3]      # every batch and every operand kind twice per route
            out.append(dict(kind="up", id=f"up-{route}-{V}x{H}-B{B}-T{T}-{kind}{'-sample' if sample else ''}", V=V, H=H, B=B, T=T,
                            sample=sample, operand=kind, opts=opts, groups=(),
                            route={"up": route, "up_epilogue": _lean(route, T == 1.0, not sample)}))
    # the bit plane of a batch the caller asserts to be 0/1 (forward(data_binary=True), T = 1): k1_stream's lean bit-plane instantiation.
    # Its general instantiation runs only inside the CD pass, which test_cd_routes_gpu.py pins on every route (cd_cases.py).
    for B in (33, 130):
        out.append(dict(kind="forward", id=f"forward-stream_bits-1040x36-B{B}", V=1040, H=36, B=B, T=1.0, sample=False, operand="binary",
                        opts={}, groups=(), route={"up": "stream_bits", "up_epilogue": "lean"}))
    return out


def ref_up(c):
    """float64 probabilities, and with a sample the reference's decisions 1[p > u] on the PhiloxStream draw."""
    p = sigmoid64(_case_up_logits64(c) / max(1e-6, c["T"]))
    s = (p > case_stream(c).uniform((c["B"], c["H"]))).astype(F32) if c["sample"] else None
    return p, s


def oracle_up(c):
    st = state(c["V"], c["H"], W=c.get("W"))
    p = O.forward(st, operand(c["operand"], c["B"], c["V"]), c["T"])
    s = O._bern(p, case_stream(c).uniform(p.shape)) if c["sample"] else None
    return p, s


# ---- down steps (eng.prop_down on a real-valued h) -----------------------------------------------------------------------------------
DOWN_SHAPES = [  # route, V, H, B, options
    ("down_fused", 1040, 36, 33, {}),             # float4 rows, one chunk
    ("down_fused", 1040, 37, 33, {}),             # scalar rows
    ("down_fused", 1040, 36, 130, {}),            # one block per (tile, chunk)
    ("down_chunks2", 4100, 72, 128, {"no_down_tiled": 1}),
    ("down_chunks4", 4100, 72, 256, {"no_down_tiled": 1}),
    ("down_tiled", 4100, 72, 128, {}),
    ("down_tiled", 4100, 72, 192, {}),
]


def down_groups(V):
    """none; one group at the end; two groups, one of them straddling a 32-row tile boundary."""
    return [(), ((V - 10, V),), ((1020, 1030), (V - 10, V)) if V == 1040 else ((2040, 2056), (V - 10, V))]


def down_cases():
    out = []
    for route, V, H, B, opts in DOWN_SHAPES:
        for gi, groups in enumerate(down_groups(V)):
            for T in TEMPS:
                for lo in (0, 1):
                    out.append(dict(kind="down", id=f"down-{route}-{V}x{H}-B{B}-g{gi}-T{T}{'-logits' if lo else ''}", V=V, H=H, B=B, T=T,
                                    logits_only=lo, groups=groups, opts=opts,
                                    route={"down": route, "down_epilogue": _lean(route, T == 1.0 and not groups and not lo, True),
                                           "finish_groups": bool(groups) and not lo}))
    return out


def ref_down(c):
    """(float64 reference, un-tempered float64 logits): raw logits / T with logits_only (the group columns included), else probabilities."""
    l = _down_logits64(c["V"], c["H"], c["B"])
    return (l / max(1e-6, c["T"]) if c["logits_only"] else probs64(l, c["T"], c["groups"])), l


def oracle_down(c):
    st = state(c["V"], c["H"], c["groups"])
    h = operand("real", c["B"], c["H"])
    return O.visible_logits(st, h, c["T"]) if c["logits_only"] else O.visible_probs(st, h, c["T"])


# ---- Gibbs steps (eng.gibbs_step) ---------------------------------------------------------------------------------------------------
GIBBS_DOWN = [   # name, sample_h, options, down route
    ("k2s", True, {}, "k2_stream"),
    ("k2s24", True, {"k2s_rows": 24}, "k2_stream"),              # two MFMA tiles per block
    ("bits", True, {"no_k2s": 1}, "down_fused"),                 # from the bit plane
    ("bf16", True, {"no_bits": 1}, "down_fused"),                # from the one-term bf16 form
    ("mf", False, {}, "down_fused"),                             # mean-field h: the three-term operand
]


def gibbs_cases():
    out = []

    def add(V, H, B, name, sample_h, sample_v, opts, up, down, groups):
        out.append(dict(kind="gibbs", id=f"gibbs-{V}x{H}-B{B}-{name}{'-sv' if sample_v else ''}{'-grp' if groups else ''}", V=V, H=H, B=B,
                        sample_h=sample_h, sample_v=sample_v, groups=groups, opts=opts, operand="mixed",
                        # both propagations write a final state next to the probabilities: never the streaming kernels' lean epilogue
                        route={"up": up, "up_epilogue": _lean(up, True, False), "down": down,
                               "down_epilogue": _lean(down, not groups, False), "finish_groups": bool(groups)}))

    for V, H, up in ((1040, 36, "stream_real"), (130, 72, "fused")):
        for name, sample_h, opts, down in GIBBS_DOWN:
            for sample_v, grp, B in ((False, False, 33), (True, False, 130), (False, True, 130), (True, True, 33)):
                add(V, H, B, name, sample_h, sample_v, opts, up, down, ((V - 10, V),) if grp else ())
    # the scalar-row kernels on both sides
    add(1040, 37, 33, "bits", True, True, {}, "partial", "down_fused", ((1030, 1040),))
    return out


def gibbs_draws(c):
    """Draw tensors the step consumes (rng.py's schedule)."""
    return (1 if c["sample_h"] else 0) + ((1 + len(c["groups"])) if c["sample_v"] else 0)


def ref_gibbs(c):
    """float64 (v_next, v_prob, h, h_prob) with the decisions taken on the PhiloxStream draws."""
    V, H, B = c["V"], c["H"], c["B"]
    W, hb, vb = case_params(c)
    ps = case_stream(c)
    h_prob = sigmoid64(_case_up_logits64(c))
    h = (h_prob > ps.uniform((B, H))).astype(np.float64) if c["sample_h"] else h_prob
    v_prob = probs64(_down64(W, vb, h), 1.0, c["groups"])
    v_next = v_prob
    if c["sample_v"]:
        v_next = (v_prob > ps.uniform((B, V))).astype(np.float64)
        for s, e in c["groups"]:
            idx = ps.categorical(np.clip(v_prob[:, s:e], 1e-8, 1.0).astype(F32))
            v_next[:, s:e] = 0.0
            v_next[np.arange(B), s + idx] = 1.0
    assert ps.offset == gibbs_draws(c)
    return v_next, v_prob, h, h_prob


def oracle_gibbs(c):
    st = state(c["V"], c["H"], c["groups"], W=c.get("W"))
    return O.gibbs_step(st, operand(c["operand"], c["B"], c["V"]), case_stream(c), c["sample_h"], c["sample_v"])


# ---- wide chains and the clamped update (through the RBM methods) -------------------------------------------------------------------
CHAIN_V, CHAIN_LABELS = 1089, 14
CHAIN_DZ = CHAIN_V - CHAIN_LABELS
CHAIN_GROUPS = ((CHAIN_DZ, CHAIN_V),)
CHAIN_CALLS = [  # name, method, keyword arguments
    ("cg", "conditional_gibbs", dict(n_steps=3, sample_h=False, sample_v=False)),
    ("cg-h", "conditional_gibbs", dict(n_steps=3, sample_h=True, sample_v=False)),
    ("cg-v", "conditional_gibbs", dict(n_steps=3, sample_h=False, sample_v=True)),
    ("cg-hv", "conditional_gibbs", dict(n_steps=3, sample_h=True, sample_v=True)),
    ("nmf-mu", "noisy_meanfield_annealed", dict(n_steps=5)),                                     # with the mu-pull, eta0 = 0.15
    ("cga", "conditional_gibbs_annealed", dict(n_steps=4, sample_h_until=2, sample_v_every=2)),
    ("clamped-mf", "train_epoch_clamped", dict(CD=2, cond_init_steps=4, sample_h=False, sample_v=False, reclamp_negative=True)),
    ("clamped-hv", "train_epoch_clamped", dict(CD=2, cond_init_steps=4, sample_h=True, sample_v=True, reclamp_negative=True)),   # vmode 2
]
CHAIN_ROUTES = [  # name, H, options, up route
    ("default", 36, {}, "stream_real"),
    ("no_k1s", 36, {"no_k1s": 1}, "partial4"),
    ("no_k2s", 36, {"no_k2s": 1}, "stream_real"),
    ("h37", 37, {}, "partial"),
]
CLAMPED_EPOCH, CLAMPED_MAX_EPOCHS = 1, 10


def chain_cases():
    """last_route() sees the LAST propagation pair of the call.  Chains: the final mean-field pass (conditional_gibbs: T = 1, unclamped;
    conditional_gibbs_annealed: T = 1; noisy_meanfield_annealed: T = 0.9), whose K1 also writes the hidden operand form and whose K2 has
    the softmax group.  Clamped update: H- = up(v-) at T = 1 writing probabilities alone, behind the last clamped K2 of the CD loop, which
    reads the bit plane of a sampled h (k2_stream where it applies)."""
    out = []
    for ci, (cname, method, kw) in enumerate(CHAIN_CALLS):
        for ri, (rname, H, opts, up) in enumerate(CHAIN_ROUTES):
            B = (27, 130)[(ci + ri) % 2]
            known = ("labels", "features")[(ci + ri // 2) % 2]
            clamped = method == "train_epoch_clamped"
            t1 = clamped or method != "noisy_meanfield_annealed"
            k2s = clamped and kw["sample_h"] and H % 4 == 0 and not opts.get("no_k2s")
            out.append(dict(kind="chain", id=f"chain-{cname}-{rname}-B{B}-{known}", V=CHAIN_V, H=H, B=B, groups=CHAIN_GROUPS, opts=opts,
                            call=cname, variant=rname, method=method, kw=kw, known=known, mu=cname == "nmf-mu",
                            route={"up": up, "up_epilogue": _lean(up, t1, clamped), "down": "k2_stream" if k2s else "down_fused",
                                   "down_epilogue": "general", "finish_groups": True}))
    return out


def chain_inputs(c):
    """(v_known, known_mask, mu or None)"""
    B, V, Dz = c["B"], c["V"], CHAIN_DZ
    g = np.random.Generator(np.random.PCG64(31 * B + c["H"]))
    z = g.random((B, Dz), dtype=F32)
    y = np.eye(V - Dz, dtype=F32)[np.arange(B) % (V - Dz)]
    mu = g.random((B, Dz), dtype=F32)
    vk = np.zeros((B, V), F32); km = np.zeros((B, V), F32)
    if c["known"] == "labels":
        vk[:, Dz:] = y; km[:, Dz:] = 1
    else:
        vk[:, :Dz] = z; km[:, :Dz] = 1
    return vk, km, (mu if c["mu"] else None)


def oracle_chain(c):
    """(final state or loss, oracle state after the call)"""
    st = state(c["V"], c["H"], c["groups"])
    vk, km, mu = chain_inputs(c)
    ps = case_stream(c)
    if mu is not None:
        st.mu_pull = {"mu_k": mu, "eta0": 0.15}
    if c["method"] == "train_epoch_clamped":
        out = O.train_epoch_clamped(st, vk, km, CLAMPED_EPOCH, ps, **c["kw"])
    else:
        out = getattr(O, c["method"])(st, vk, km, ps, **c["kw"])
    st.mu_pull = None
    return out, st, ps.offset


# ---- the table --------------------------------------------------------------------------------------------------------------------
# Philox seed per case that draws: the first seed >= 1 whose margins pass (printed by `python tests/route_cases.py`)
SEEDS = {
    "chain-cg-v-no_k1s-B130-labels": 3,
    "chain-cg-v-h37-B130-features": 3,
    "chain-cg-hv-no_k2s-B130-labels": 2,
    "chain-clamped-hv-default-B130-features": 5,
}


def has_draws(c):
    return c["kind"] == "chain" or (c["kind"] == "gibbs" and gibbs_draws(c) > 0) or bool(c.get("sample"))


def run_oracle(c):
    """Run the case's oracle with its seed; returns (result, smallest Bernoulli margin, smallest categorical margin)."""
    O.reset_margin()
    res = {"up": oracle_up, "forward": oracle_up, "down": oracle_down, "gibbs": oracle_gibbs, "chain": oracle_chain}[c["kind"]](c)
    return res, O.BERNOULLI_MARGIN["min"], CATEGORICAL_MARGIN["min"]


@functools.lru_cache(maxsize=None)
def _all():
    cs = up_cases() + down_cases() + gibbs_cases() + chain_cases()
    for c in cs:
        c["seed"] = SEEDS.get(c["id"], 1)
    assert len({c["id"] for c in cs}) == len(cs)
    return tuple(cs)


def cases(kind=None):
    return [c for c in _all() if kind is None or c["kind"] == kind or (kind == "up" and c["kind"] == "forward")]


if __name__ == "__main__":      # pin the seeds: prints the SEEDS table
    print("SEEDS = {")
    for c in _all():
        if not has_draws(c):
            continue
        for seed in range(1, 200):
            c["seed"] = seed
            _, bm, cm = run_oracle(c)
            if bm >= MARGIN and cm >= MARGIN:
                break
        else:
            raise SystemExit(f"no seed for {c['id']}")
        if seed != 1:
            print(f'    "{c["id"]}": {seed},')
    print("}")
