#!/usr/bin/env python3
"""A residual flow on tabular-sized rows (d = 8) at inference: K x [Residual(LipschitzMLP([8, 64, 64, 8])), ActNorm(8)] in evaluation
mode, `log_prob` of one batch on both routes under one seed pair, printed side by side.

    python examples/residual_tabular.py [--batch 8] [--layers 4]

`config.set_residual_nd(True)` runs the density pass of the whole stack as one launch of csrc/lipmlp_nd.hip (Hutchinson's power
series by forward-mode tangents); the default, off, runs the torch formulas: one autograd pass through the network per series term.
Both routes draw the same truncations and the same noise, so the two columns differ by float32 rounding alone.  Runs on cuda:0.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import normflows_amd as nf  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.manual_seed(a.seed)
    flows = []
    for _ in range(a.layers):
        net = nf.nets.LipschitzMLP([8, 64, 64, 8], init_zeros=False, lipschitz_const=0.9)
        flows += [nf.flows.Residual(net, reduce_memory=True), nf.flows.ActNorm(8)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(8, trainable=False), flows).to(dev).eval()
    x = torch.randn(a.batch, 8, device=dev)
    with torch.no_grad():
        model.log_prob(x)               # the ActNorm layers take their statistics from the first batch
    nf.utils.update_lipschitz(model, 50)
    out = {}
    for route in (False, True):
        nf.config.set_residual_nd(route)
        np.random.seed(a.seed)
        torch.manual_seed(a.seed)
        with torch.no_grad():
            out[route] = model.log_prob(x).cpu()
    nf.config.set_residual_nd(False)
    print("%4s  %14s  %14s  %10s" % ("row", "torch formulas", "one launch", "difference"))
    for i in range(a.batch):
        print("%4d  %14.6f  %14.6f  %10.2e" % (i, out[False][i], out[True][i], abs(out[False][i] - out[True][i])))
    return out


if __name__ == "__main__":
    res = main()
    assert torch.allclose(res[False], res[True], rtol=1e-4, atol=1e-4), "the two routes disagree"
