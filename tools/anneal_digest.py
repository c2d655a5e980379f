"""One SHA-256 per likelihood call and test case over the bytes HipEngine returns (log weights and final state of the annealing calls,
Gaussian included; acc and h of bound_step / gauss_bound_step; the rows of free_energy, gauss_free_energy and pseudo_loglik), on the
GPU.  Two builds of the engine compute the same thing bit for bit exactly when their listings are equal: run it in a checkout of either
commit and compare.  The cases are the parity cases of the test suite, each under its pinned Philox seed."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multimodal-idbn_amd"), os.path.join(ROOT, "tests")]


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    import __graft_entry__ as ge
    ge.build()
    import torch
    import anneal_cases as Cs
    import gauss_ais_cases as Ga
    import gauss_bound_cases as Gb
    from imdbn import engine as E
    from imdbn.models import RBM
    if not torch.cuda.is_available():
        raise SystemExit("anneal_digest needs a GPU")
    dev = "cuda:0"
    eng = E.get_hip_engine()

    def rbm(c, pitch=None):
        V, H = c["W"].shape
        r = RBM(V, H, 0.1, 0.0, 0.5, softmax_groups=c.get("groups") or None).to(dev)
        pitch = c.get("pitch") if pitch is None else pitch
        if pitch is not None:
            r.W.data = torch.empty(V, pitch, device=dev)[:, :H]
        for p, k in ((r.W, "W"), (r.vis_bias, "b"), (r.hid_bias, "c")):
            p.data.copy_(torch.from_numpy(c[k]))
        return r

    def ladder(c):
        return dict(betas=torch.from_numpy(c["betas"]), rng=E.PhiloxRng(c["seed"]), return_state=True,
                    base_vis_bias=None if c["bA"] is None else torch.from_numpy(c["bA"]).to(dev))

    for name in Cs.FORWARD:
        c = Cs.case(Cs.FORWARD, name)
        print("ais", name, digest(*eng.ais(rbm(c), n_chains=c["M"], **ladder(c))), flush=True)
    for name in Cs.GROUPS:
        c = Cs.case(Cs.GROUPS, name)
        print("ais_groups", name, digest(*eng.ais_groups(rbm(c), n_chains=c["M"], **ladder(c))), flush=True)
    for name in Cs.REVERSE:
        c = Cs.case(Cs.REVERSE, name)
        x = torch.from_numpy(c["x"]).to(dev)
        print("reverse_ais", name, digest(*eng.reverse_ais(rbm(c), x, **ladder(c))), flush=True)
        for mode in () if c["groups"] else ("entropy", "logq"):      # bound_step takes no softmax groups
            print("bound_step", mode, name, digest(*eng.bound_step(rbm(c), x, E.PhiloxRng(c["seed"]), mode=mode)), flush=True)
        print("free_energy", name, digest(eng.free_energy(rbm(c), x)), flush=True)
        print("pseudo_loglik", name, digest(*eng.pseudo_loglik(rbm(c), x, return_sites=True)), flush=True)
    for name, with_bA in Ga.RUNS:
        c = Ga.case(name, with_bA)
        seed = c["philox_seed"] if c["philox_seed"] is not None else c["seed"]
        z, bA = torch.from_numpy(c["z"]).to(dev), None if c["bA"] is None else torch.from_numpy(c["bA"]).to(dev)
        for pitch in c["pitches"]:
            out = eng.gauss_ais(rbm(c, pitch), z, torch.from_numpy(c["betas"]), c["M"], E.PhiloxRng(seed), base_vis_bias=bA, return_state=True)
            print("gauss_ais", name, "bA" if with_bA else "b", pitch, digest(*out), flush=True)
    for name in Gb.NAMES:
        c = Gb.case(name)
        z, v = torch.from_numpy(c["z"]).to(dev), torch.from_numpy(c["v"]).to(dev)
        for pitch in c["pitches"]:
            for mode in Gb.MODES:
                out = eng.gauss_bound_step(rbm(c, pitch), z, v, E.PhiloxRng(c["philox_seed"]), mode=mode)
                print("gauss_bound_step", mode, name, pitch, digest(*out), flush=True)
            print("gauss_free_energy", name, pitch, digest(eng.gauss_free_energy(rbm(c, pitch), z, v)), flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
