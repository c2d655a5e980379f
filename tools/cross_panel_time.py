#!/usr/bin/env python3
"""Time of the batched cross-modal convergence panel (imdbn.utils.conditional_steps) at the config-3 shapes: [10000, 1500, 500]
image stack, 532 <-> 256 joint RBM with K = 32 labels, N = 128 samples, 70 steps, both directions -- against the B = 1 wrappers
called N times per direction on the same engine.  Prints one JSON line: panel total and its chain / decode-error / scan parts
(HIP events), and the loop time."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multimodal-idbn_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    import __graft_entry__ as ge
    ge.build()
    from imdbn import engine as E
    from imdbn.models import RBM, iDBN
    from imdbn.utils import conditional_steps as CS
    dev = torch.device("cuda")
    sizes, Dz, K, JH, N, T = [10000, 1500, 500], 500, 32, 256, 128, 70
    g = np.random.Generator(np.random.PCG64(1))

    def rbm(V, H, scale, groups=None):
        r = RBM(V, H, 0.1, 1e-4, 0.5, softmax_groups=groups).to(dev)
        r.W.data.copy_(torch.from_numpy((g.standard_normal((V, H)) * scale).astype(np.float32)))
        r.vis_bias.data.copy_(torch.from_numpy((g.standard_normal(V) * 0.3).astype(np.float32)))
        return r

    class M:
        pass

    m = M()
    m.device = dev
    m.image_idbn = iDBN.__new__(iDBN)
    m.image_idbn.device = dev
    m.image_idbn.layers = [rbm(sizes[i], sizes[i + 1], 2.0 / np.sqrt(sizes[i])) for i in range(2)]
    m.joint_rbm = rbm(Dz + K, JH, 0.15, [(Dz, Dz + K)])
    m.Dz_img, m.num_labels = Dz, K
    m.z_class_mean = torch.rand(K, Dz, device=dev)
    m.wandb_run = None
    imgs = (torch.rand(N, 10000, device=dev) < 0.15).float()
    lbls = torch.eye(K, device=dev)[torch.arange(N, device=dev) % K]
    eng = E.get_hip_engine()
    E.manual_seed(7)

    # the panel's parts, each between HIP events (same calls as CS.trace_cross_panel_batch)
    def parts():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        a, _, _ = CS._img2txt_spec(m, imgs, K, T, False, False)
        b, z0, _ = CS._txt2img_spec(m, lbls, T, False, False)
        (_, tra), (_, trb) = eng.chain_traced(m.joint_rbm, a, b, m.joint_rbm._rng(N))
        ev[1].record()
        i2t = CS._img2txt_result(eng, tra, lbls, 1e-3, 3, 0.25)
        zn, dz = eng.code_scan(trb, z0, 0.0)
        ev[2].record()
        rows = torch.arange(N, dtype=torch.int32, device=dev).repeat(T)
        mse = eng.decode_sqerr(m.image_idbn.layers, zn.reshape(T * N, Dz), imgs, rows).view(T, N).t().contiguous()
        ev[3].record()
        eng.patience_scan(dz, mse, 1e-3, 1e-5, 3)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3])

    def panel():
        CS.trace_cross_panel_batch(m, imgs, lbls, max_steps=T)
        torch.cuda.synchronize()

    for _ in range(3):
        panel()
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        panel()
    panel_ms = (time.perf_counter() - t0) * 1e3 / reps
    pr = [parts() for _ in range(reps)]
    med = [float(np.median([p[i] for p in pr])) for i in range(3)]

    def loop():
        for i in range(N):
            CS.trace_img2txt_cross(m, imgs[i:i + 1], lbls[i:i + 1], max_steps=T)
            CS.trace_txt2img_cross(m, imgs[i:i + 1], lbls[i:i + 1], max_steps=T)
        torch.cuda.synchronize()

    loop()
    t0 = time.perf_counter()
    loop()
    loop_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"what": "cross_panel_time", "N": N, "max_steps": T, "image_stack": sizes, "joint": [Dz + K, JH], "K": K,
                      "panel_ms": round(panel_ms, 3),
                      "parts_ms": {"chain_pair": round(med[0], 3), "label_and_code_scan": round(med[1], 3),
                                   "decode_error": round(med[2], 3)},
                      "b1_loop_ms": round(loop_ms, 1), "speedup": round(loop_ms / panel_ms, 1),
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
