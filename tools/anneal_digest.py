"""One SHA-256 per annealing call and test case over the bytes HipEngine returns (log weights and final state; acc and h for
bound_step), on the GPU.  Two builds of the engine compute the same thing bit for bit exactly when their listings are equal: run it in
a checkout of either commit and compare.  The cases are the parity cases of the test suite, each under its pinned Philox seed."""
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
    from imdbn import engine as E
    from imdbn.models import RBM
    if not torch.cuda.is_available():
        raise SystemExit("anneal_digest needs a GPU")
    dev = "cuda:0"
    eng = E.get_hip_engine()

    def rbm(c):
        V, H = c["W"].shape
        r = RBM(V, H, 0.1, 0.0, 0.5, softmax_groups=c.get("groups") or None).to(dev)
        if c.get("pitch") is not None:
            r.W.data = torch.empty(V, c["pitch"], device=dev)[:, :H]
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
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
