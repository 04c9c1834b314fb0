#!/usr/bin/env python3
"""Generates tests/golden/ar_perm_lin.npz by running the REAL reference (normflows 1.7.3, PyTorch CPU) like make_golden_circ_ar.py:
AutoregressiveRationalQuadraticSpline (wrapper.py:186-244) with permute_mask=True and scalar linear tails -- 3K - 1 rows per feature,
the identity outside the interval -- the second layer family the per-feature one-launch kernels take.

Needs the reference checkout at /root/reference:
    python tests/golden/make_golden_ar_perm_lin.py
Stores the input (two rows with an entry outside the bound), both directions' outputs and log-dets in float32, the same in float64
(the reference's own float32 error) and the state dict: `mask` and `degrees` are buffers, so the permutation travels with it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import normflows as nf  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)

D, HIDDEN, K, BOUND = 6, 20, 4, 2.5


def build(dtype=torch.float32):
    torch.manual_seed(31)
    layer = nf.flows.AutoregressiveRationalQuadraticSpline(D, 2, HIDDEN, num_bins=K, tail_bound=BOUND, permute_mask=True,
                                                           init_identity=False)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return layer.to(dtype)


def main():
    layer = build()
    deg = layer.mprqat.autoregressive_net.final_layer.degrees[::3 * K - 1]
    assert not torch.equal(deg, torch.arange(1, D + 1)), "the seed must give a non-identity degree permutation"
    g = torch.Generator().manual_seed(33)
    x = (torch.rand(16, D, generator=g) * 2 - 1) * BOUND * 0.98
    x[0, 2], x[3, 5] = 7.0, -4.0                      # outside the bound: linear tails pass the value through, log-det 0
    with torch.no_grad():
        zf, ldf = layer.forward(x)
        zi, ldi = layer.inverse(x)
        l64 = build(torch.float64)
        zf64, ldf64 = l64.forward(x.double())
        zi64, ldi64 = l64.inverse(x.double())
    assert float(zi[0, 2]) == 7.0 and float(zi[3, 5]) == -4.0
    print("degrees", deg.tolist())
    print("float32 vs float64 (density): z %.2e  ld %.2e" % (float((zi.double() - zi64).abs().max()), float((ldi.double() - ldi64).abs().max())))
    out = dict(x=x, z_fwd=zf, ld_fwd=ldf, z_inv=zi, ld_inv=ldi, z_fwd_f64=zf64, ld_fwd_f64=ldf64, z_inv_f64=zi64, ld_inv_f64=ldi64)
    out.update({"sd__" + k.replace(".", "__"): v for k, v in layer.state_dict().items()})
    path = os.path.join(OUT, "ar_perm_lin.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
