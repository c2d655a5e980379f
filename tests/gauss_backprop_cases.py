"""Cases of the Gaussian backprop tests (tests/test_gauss_backprop_cpu.py, tests/test_gauss_backprop_gpu.py).

Single calls.  The five shapes of tests/gauss_cases.py (imported, not copied: `one`, `odd`, `h130`, `rows67`, `wide`; parameters,
momenta, real data, logvar and its momentum as there) and `offw`, 70 x 36 with 9 rows, whose W starts one float off 16-byte
alignment on the device: H is a multiple of 4, so only the pointer sends the statistics pass and gauss_apply down their scalar
forms.  Each shape runs the four FORMS: `up` (e_h), `down` (x_h), `both`, and `eval` (down pair, no update, err_h wanted).  Error rows
are signed normal values (std 0.3), hidden inputs uniform in (0.02, 0.98) so that x (1 - x) is nowhere zero.

Composed steps.  STEPS consecutive gaussian_autoencoder_steps on the STACKS: [37, 33, 21] on `odd`, [130, 200, 70] on `rows67` (67
rows) and the single layer [37, 33] on `odd` (L = 1: z tied).  Layer 0 is the shape's Gaussian layer, the layer above is drawn here.

Nothing draws on the device: no seeds, no Bernoulli margins.

fp32 restatement against the float64 twin over every single call and every composed run (`python tests/gauss_backprop_cases.py`
prints it; the GPU tolerances are 8 x these, computed when the tests run):
    logvar    7.8e-06 absolute     logvar_m  4.4e-06 absolute
    nll       1.7e-07 relative to max(1, |nll|)     mse   2.0e-07 relative to max(1, |mse|)
The largest logvar errors come from the composed runs (three chained fp32 steps); over the single calls alone logvar is within 2.0e-07."""
import numpy as np

import gauss_cases as Gc
import gauss_backprop_oracle as Go

F32, F64 = np.float32, np.float64
LR, MOM, WEIGHT_DECAY, LR_Z_MULT = Gc.LR, Gc.MOM, Gc.WEIGHT_DECAY, Gc.LR_Z_MULT
LR_Z = LR_Z_MULT * LR
E_STD = 0.3
SHAPES = list(Gc.CASES) + ["offw"]
FORMS = ("up", "down", "both", "eval")
RUNS = [(s, f) for s in SHAPES for f in FORMS]
STEPS = 3
# name -> (gauss case of layer 0, hidden sizes above it)
STACKS = {"odd3": ("odd", (21,)), "rows67_3": ("rows67", (70,)), "odd1": ("odd", ())}
HYPER = (LR_Z_MULT, -np.inf, np.inf)


def case(name):
    """gauss_cases.case plus e_h, x_h [B, H] and w_offset (floats W starts off alignment on the device)."""
    if name == "offw":
        V, H, B = 70, 36, 9
        g = np.random.Generator(np.random.PCG64(3511))
        n = lambda *s: g.standard_normal(s)
        c = dict(name=name, V=V, H=H, B=B, W=(n(V, H) * 0.2).astype(F32), b=(n(V) * 0.3).astype(F32), c=(n(H) * 0.3).astype(F32),
                 W_m=(n(V, H) * 0.01).astype(F32), hb_m=(n(H) * 0.01).astype(F32), vb_m=(n(V) * 0.01).astype(F32),
                 data=((-1 + 2 * g.random(V)) + (0.3 + 2.7 * g.random(V)) * n(B, V)).astype(F32), z=(-1 + 2 * g.random(V)).astype(F32),
                 z_m=(n(V) * 0.01).astype(F32), sparsity=False, w_offset=1)
    else:
        c = Gc.case(name)
        c["w_offset"] = 0
    g = np.random.Generator(np.random.PCG64(3520 + SHAPES.index(name)))
    c["e_h"] = (g.standard_normal((c["B"], c["H"])) * E_STD).astype(F32)
    c["x_h"] = g.uniform(0.02, 0.98, (c["B"], c["H"])).astype(F32)
    return c


def gstate(c, dt=F64):
    import gauss_oracle as G
    return G.GState(c["W"], c["b"], c["c"], c["z"], c["W_m"], c["vb_m"], c["hb_m"], c["z_m"], weight_decay=WEIGHT_DECAY, dt=dt)


def form_args(c, form):
    """The keywords of one call of `form`: the pairs, apply and what it returns."""
    up = c["e_h"] if form in ("up", "both") else None
    down = c["x_h"] if form in ("down", "both", "eval") else None
    return dict(up=up, down=down, apply=form != "eval")


def twin_call(c, form, dt=F64, lr_z=LR_Z, z_lo=-np.inf, z_hi=np.inf):
    """One twin call of `form` on the case: dict(st: the state after, out: what the call returned)."""
    st = gstate(c, dt)
    out = Go.gauss_backprop_step(st, c["data"], lr=LR, mom=MOM, lr_z=lr_z, z_lo=z_lo, z_hi=z_hi, dt=dt, **form_args(c, form))
    return dict(st=st, out=out)


def stack(name):
    """dict(name, sizes, B, data, layers: [gauss case dict, then dicts of W, hid_bias, vis_bias and momenta])."""
    base, above = STACKS[name]
    c = case(base)
    g = np.random.Generator(np.random.PCG64(3540 + list(STACKS).index(name)))
    layers, n_in = [c], c["H"]
    for n_out in above:
        n = lambda *s: g.standard_normal(s)
        layers.append(dict(W=(n(n_in, n_out) * 0.3).astype(F32), hid_bias=(n(n_out) * 0.2).astype(F32), vis_bias=(n(n_in) * 0.2).astype(F32),
                           W_m=(n(n_in, n_out) * 0.01).astype(F32), hb_m=(n(n_out) * 0.01).astype(F32), vb_m=(n(n_in) * 0.01).astype(F32)))
        n_in = n_out
    return dict(name=name, sizes=[c["V"], c["H"], *above], B=c["B"], data=c["data"], layers=layers)


def states(s, dt=F64):
    """(rec, gen) twin states of a stack: the twins copy W, the biases and logvar and start with zero momenta (gaussian_untie)."""
    import gauss_oracle as G
    rec = [gstate(s["layers"][0], dt)]
    for l in s["layers"][1:]:
        rec.append(Go.bern_state(l["W"], l["hid_bias"], l["vis_bias"], WEIGHT_DECAY, dt, l["W_m"], l["hb_m"], l["vb_m"]))
    gen = []
    for i, r in enumerate(rec[:-1]):
        if i == 0:
            gen.append(G.GState(r.W, r.b, r.c, r.z, weight_decay=WEIGHT_DECAY, dt=dt))
        else:
            gen.append(Go.bern_state(r.W, r.hid_bias, r.vis_bias, WEIGHT_DECAY, dt))
    return rec, gen


def twin_stack_run(s, dt=F64, steps=STEPS):
    """`steps` consecutive twin steps: dict(steps: the per-step results, rec, gen: the final states)."""
    rec, gen = states(s, dt)
    out = [Go.autoencoder_step(rec, gen, s["data"], [(LR, MOM)] * len(rec), HYPER, dt=dt) for _ in range(steps)]
    return dict(steps=out, rec=rec, gen=gen)


def fp32_errors():
    """What fp32 arithmetic alone costs: the float32 restatement against the float64 twin over every single call of RUNS and every
    composed run of STACKS.  {"z", "z_m": max absolute error of logvar / logvar_m, "nll", "mse": max error relative to max(1, |twin|)}."""
    err = {"z": 0.0, "z_m": 0.0, "nll": 0.0, "mse": 0.0}
    up = lambda k, v: err.__setitem__(k, max(err[k], float(v)))
    rel = lambda a, b: abs(a - b) / max(1.0, abs(b))

    def states_err(a, b):
        up("z", np.abs(b.z.astype(F64) - a.z).max())
        up("z_m", np.abs(b.z_m.astype(F64) - a.z_m).max())

    for name, form in RUNS:
        c = case(name)
        a, b = twin_call(c, form), twin_call(c, form, dt=F32)
        states_err(a["st"], b["st"])
        if a["out"]["nll"] is not None:
            up("nll", rel(b["out"]["nll"], a["out"]["nll"]))
            up("mse", rel(b["out"]["mse"], a["out"]["mse"]))
    for name in STACKS:
        s = stack(name)
        a, b = twin_stack_run(s), twin_stack_run(s, dt=F32)
        states_err(a["rec"][0], b["rec"][0])
        if a["gen"]:
            states_err(a["gen"][0], b["gen"][0])
        for x, y in zip(a["steps"], b["steps"]):
            up("nll", rel(y["nll"], x["nll"]))
            up("mse", rel(y["mse"], x["mse"]))
    return err


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("fp32 restatement vs float64 twin:", {k: f"{v:.3g}" for k, v in fp32_errors().items()})
