#!/usr/bin/env python3
"""Generates tests/golden/circ_ar_perm_tb.npz by running the REAL reference (normflows 1.7.3, PyTorch CPU) like make_golden.py:
CircularAutoregressiveRationalQuadraticSpline (wrapper.py:247-311) with everything the one-launch sampling kernel reads from its
per-feature table at once -- a permuted mask (nets/made.py:250-252), list tails (utils/splines.py:48-57), a tensor tail bound
(:61-66) and the periodic preprocessing of the circular coordinates (utils/nn.py:64-129).

Run in the build container only (the GPU box has no reference):
    python tests/golden/make_golden_circ_ar.py
Stores the input, both directions' outputs and log-dets in float32, the same in float64 (the reference's own float32 error) and the
state dict: `mask` and `degrees` are buffers, so the permutation travels with it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, "/root/reference")
import normflows as nf  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
torch.set_num_threads(4)

D, HIDDEN, K, IND_CIRC = 7, 24, 6, [0, 2, 5]
BOUND = [np.pi, 2.0, np.pi, 3.0, 2.5, np.pi, 1.5]


def build(dtype=torch.float32):
    torch.manual_seed(21)
    layer = nf.flows.CircularAutoregressiveRationalQuadraticSpline(D, 2, HIDDEN, ind_circ=IND_CIRC, num_bins=K,
                                                                   tail_bound=torch.tensor(BOUND, dtype=torch.float32),
                                                                   permute_mask=True, init_identity=False)
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        for p in layer.parameters():
            p.add_(0.3 * torch.randn(p.shape, generator=g, dtype=p.dtype))
    return layer.to(dtype)


def main():
    layer = build()
    deg = layer.mprqat.autoregressive_net.final_layer.degrees[::3 * K + 1]
    assert not torch.equal(deg, torch.arange(1, D + 1)), "the seed must give a non-identity degree permutation"
    g = torch.Generator().manual_seed(23)
    x = (torch.rand(16, D, generator=g) * 2 - 1) * torch.tensor(BOUND, dtype=torch.float32) * 0.98     # inside every interval
    x[0, 1], x[1, 3] = 50.0, -60.0                    # linear features outside their interval: the list branch gives 0, log-det 0
    with torch.no_grad():
        zf, ldf = layer.forward(x)                    # sampling direction: the D-pass inverse of the transform
        zi, ldi = layer.inverse(x)
        l64 = build(torch.float64)
        zf64, ldf64 = l64.forward(x.double())
        zi64, ldi64 = l64.inverse(x.double())
        back, _ = layer.inverse(zf)
    assert float(zf[0, 1]) == 0.0 and float(zf[1, 3]) == 0.0
    print("degrees", deg.tolist())
    print("round trip (rows without an outside entry) %.2e" % float((back - x)[2:].abs().max()))
    print("float32 vs float64: x %.2e  ld %.2e" % (float((zf.double() - zf64).abs().max()), float((ldf.double() - ldf64).abs().max())))
    out = dict(x=x, z_fwd=zf, ld_fwd=ldf, z_inv=zi, ld_inv=ldi, z_fwd_f64=zf64, ld_fwd_f64=ldf64, z_inv_f64=zi64, ld_inv_f64=ldi64)
    out.update({"sd__" + k.replace(".", "__"): v for k, v in layer.state_dict().items()})
    path = os.path.join(OUT, "circ_ar_perm_tb.npz")
    np.savez_compressed(path, **{k: v.detach().cpu().numpy() for k, v in out.items()})
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
