#!/usr/bin/env python3
"""Generates the fixtures of the conditional NSF coupling layer (tests/golden/ctx_*.npz) by running the REAL reference (normflows
1.7.3, PyTorch CPU), as make_golden.py does for the other layers.  Run in the build container only (the GPU box has no reference):
    python tests/golden/make_golden_context.py
Each fixture holds the float32 state dict, the inputs (a quarter of the rows beyond the tail bound), the context, and the reference's
outputs in float32 and float64 on the same weights and inputs (the float64 leg runs on the float32 weights cast up)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import normflows as nf  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)

# name, D, C, hidden, blocks, bins, rows: Hp 128, Hp 256 (PC 32), Hp 256 with PC 64 and 16 bins
LAYERS = (("ctx_d6_c3_h40", 6, 3, 40, 2, 8, 64), ("ctx_d64_c16_h136", 64, 16, 136, 1, 4, 48),
          ("ctx_d17_c33_h200", 17, 33, 200, 1, 16, 48))


def npz(name, **arrs):
    out = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote %-34s %6.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))
    assert os.path.getsize(path) < 1 << 20


def sd(module, prefix="sd__"):
    return {prefix + k.replace(".", "__"): v.float() for k, v in module.state_dict().items()}


def perturb(module, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.add_(sigma * torch.randn(p.shape, generator=g, dtype=p.dtype))


def inputs(B, D, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = 1.2 * torch.randn(B, D, generator=g)
    x[: B // 4] *= 4.0                          # rows beyond the tail bound (3): linear tails
    return x, torch.randn(B, C, generator=g)


def gen_layers():
    for name, D, C, H, NB, K, B in LAYERS:
        torch.manual_seed(D + C + H)
        layer = nf.flows.CoupledRationalQuadraticSpline(D, NB, H, num_context_channels=C, num_bins=K, init_identity=False)
        perturb(layer, 0.05, D + H)
        layer.eval()
        x, c = inputs(B, D, C, 7 + D)
        out = dict(x=x, context=c, **sd(layer))
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            m = layer.to(dt)
            with torch.no_grad():
                zi, ldi = m.inverse(x.to(dt), c.to(dt))           # density direction (prqct.forward)
                zf, ldf = m.forward(x.to(dt), c.to(dt))           # sampling direction (prqct.inverse)
            out.update({"z_inv_" + tag: zi, "ld_inv_" + tag: ldi, "z_fwd_" + tag: zf, "ld_fwd_" + tag: ldf})
        npz(name, **out)


def gen_model():
    """2 x [CoupledRationalQuadraticSpline(8, 2, 64, C = 4) + LULinearPermute(8)] over ConditionalDiagGaussian (core.py:216-366)."""
    torch.manual_seed(61)
    flows = []
    for _ in range(2):
        flows += [nf.flows.CoupledRationalQuadraticSpline(8, 2, 64, num_context_channels=4, num_bins=8, init_identity=False),
                  nf.flows.LULinearPermute(8)]
    q0 = nf.distributions.base.ConditionalDiagGaussian(8, torch.nn.Linear(4, 16))
    m = nf.ConditionalNormalizingFlow(q0, flows)
    perturb(m, 0.1, 62)
    m.eval()
    x, c = inputs(80, 8, 4, 63)
    out = dict(x=x, context=c, **sd(m))
    for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        mm = m.to(dt)
        with torch.no_grad():
            lp = mm.log_prob(x.to(dt), c.to(dt))
            z, ld = mm.inverse_and_log_det(x.to(dt), c.to(dt))
            xf, ldf = mm.forward_and_log_det(x.to(dt), c.to(dt))
        out.update({"log_prob_" + tag: lp, "z_inv_" + tag: z, "ld_inv_" + tag: ld, "z_fwd_" + tag: xf, "ld_fwd_" + tag: ldf})
    npz("ctx_model_nsf", **out)


if __name__ == "__main__":
    gen_layers()
    gen_model()
