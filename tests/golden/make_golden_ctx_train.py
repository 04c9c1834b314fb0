#!/usr/bin/env python3
"""Generates the training fixtures of the conditional NSF coupling layer (tests/golden/grad_ctx_*.npz) by running the REAL reference
(normflows 1.7.3, PyTorch CPU) under autograd, as make_golden.py gen_train_nsf_wide does for the context-free layers.  Run in the
build container only (the GPU box has no reference):
    python tests/golden/make_golden_ctx_train.py
Single layers: the weights of the inference fixtures tests/golden/ctx_*.npz (init_identity=False, perturbed), new inputs, the loss
sum(z * cz) + sum(log_det * cl) in the density (inv_) and the sampling (fwd_) direction.  The notebook model
(examples/conditional_flow.ipynb: 4 x [CoupledRationalQuadraticSpline(2, 2, 128, context 4) + LULinearPermute(2)], DiagGaussian base)
under forward_kld(x, context), weights by seeded construction (too large to store) with a checksum of every parameter.
Each holds, in a float32 and a float64 leg: the loss, g_x, g_context, and of every parameter gradient a strided sample (every
STRIDE-th element) plus its sum and absolute sum."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import normflows as nf  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
STRIDE = 37
torch.set_num_threads(4)

# fixture, inference fixture with the weights, D, C, hidden, blocks, bins, rows
LAYERS = (("grad_ctx_d6_c3_h40", "ctx_d6_c3_h40", 6, 3, 40, 2, 8, 96),
          ("grad_ctx_d64_c16_h136", "ctx_d64_c16_h136", 64, 16, 136, 1, 4, 96),
          ("grad_ctx_d17_c33_h200", "ctx_d17_c33_h200", 17, 33, 200, 1, 16, 96))
MODEL_SEED, MODEL_ROWS = 11, 512


def npz(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote %-34s %6.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 1 << 20


def inputs(B, D, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = 1.2 * torch.randn(B, D, generator=g)
    x[: B // 4] *= 4.0                          # rows beyond the tail bound (3): linear tails
    return x, torch.randn(B, C, generator=g)


def grads(out, prefix, module, x, c, loss):
    out["loss_" + prefix] = loss.detach().double()
    out["gx_" + prefix] = x.grad
    out["gc_" + prefix] = c.grad
    for k, p in module.named_parameters():
        gflat = (torch.zeros_like(p) if p.grad is None else p.grad).reshape(-1)
        key = k.replace(".", "__")
        out["g_%s__%s" % (prefix, key)] = gflat[::STRIDE].clone()
        out["chk_%s__%s" % (prefix, key)] = torch.tensor([float(gflat.double().sum()), float(gflat.double().abs().sum())],
                                                         dtype=torch.float64)


def gen_layers():
    for name, src, D, C, H, NB, K, B in LAYERS:
        w = dict(np.load(os.path.join(OUT, src + ".npz")))
        state = {k[4:].replace("__", "."): torch.from_numpy(v) for k, v in w.items() if k.startswith("sd__")}
        x, c = inputs(B, D, C, 100 + D)
        g = torch.Generator().manual_seed(200 + D)
        cz, cl = torch.randn(B, D, generator=g), torch.randn(B, generator=g)
        out = dict(stride=np.array(STRIDE), x=x, context=c, cz=cz, cl=cl)
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            for direction in ("inv", "fwd"):
                layer = nf.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False)
                layer.load_state_dict(state, strict=True)
                layer = layer.to(dt)
                xx, cc = x.detach().clone().to(dt).requires_grad_(True), c.detach().clone().to(dt).requires_grad_(True)
                z, ld = (layer.inverse if direction == "inv" else layer.forward)(xx, cc)
                loss = (z * cz.to(dt)).sum() + (ld * cl.to(dt)).sum()
                loss.backward()
                grads(out, "%s_%s" % (tag, direction), layer, xx, cc, loss)
        npz(name, **out)


def build_model(lib):
    """The notebook's model by seeded construction; the same calls give the same weights in normflows_amd."""
    torch.manual_seed(MODEL_SEED)
    flows = []
    for _ in range(4):
        flows += [lib.flows.CoupledRationalQuadraticSpline(2, 2, 128, num_context_channels=4, init_identity=False),
                  lib.flows.LULinearPermute(2)]
    m = lib.ConditionalNormalizingFlow(lib.distributions.DiagGaussian(2), flows)
    g = torch.Generator().manual_seed(MODEL_SEED + 1)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return m


def gen_model():
    x, c = inputs(MODEL_ROWS, 2, 4, MODEL_SEED + 2)
    out = dict(stride=np.array(STRIDE), x=x, context=c)
    m = build_model(nf)
    for k, p in m.named_parameters():
        out["w__" + k.replace(".", "__")] = torch.tensor([float(p.detach().double().sum()), float(p.detach().double().abs().sum())],
                                                      dtype=torch.float64)
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        mm = build_model(nf).to(dt)
        xx, cc = x.detach().clone().to(dt).requires_grad_(True), c.detach().clone().to(dt).requires_grad_(True)
        loss = mm.forward_kld(xx, cc)
        loss.backward()
        grads(out, tag + "_kld", mm, xx, cc, loss)
    npz("grad_ctx_model_nsf", **out)


if __name__ == "__main__":
    gen_layers()
    gen_model()
