#!/usr/bin/env python3
"""The reference's real_nvp.ipynb loop at small size on the MI355X path: K x [MaskedAffineFlow(b, t, s), ActNorm] layers with
MLP([2, 4, 2]) conditioners, trained by reverse KL (samples of the model, Adam) against the prior TwoModes(2, 0.1), `normflows_amd`
in place of `normflows`.

    python examples/reverse_kld_two_modes.py [--steps 300] [--batch 1024] [--layers 8]

`--kernels 1` (config.set_target_density(True)) evaluates the target's log-density and its input gradient in one launch of
nf_density2d per step; `--kernels 0` runs the torch formulas, the reference's arithmetic.  Runs on cuda:0.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import normflows_amd as nf  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args(argv)
    nf.config.set_target_density(bool(a.kernels))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    b = torch.Tensor([1 if i % 2 == 0 else 0 for i in range(2)])
    flows = []
    for i in range(a.layers):
        s = nf.nets.MLP([2, 4, 2], init_zeros=True)
        t = nf.nets.MLP([2, 4, 2], init_zeros=True)
        flows += [nf.flows.MaskedAffineFlow(b if i % 2 == 0 else 1 - b, t, s)]
        flows += [nf.flows.ActNorm(2)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), flows, nf.distributions.TwoModes(2, 0.1)).to(dev)
    with torch.no_grad():                       # ActNorm's data-dependent initialisation, as in the notebook
        model.sample(a.batch)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-6)
    first = last = None
    for step in range(a.steps):
        opt.zero_grad()
        loss = model.reverse_kld(num_samples=a.batch)
        if ~(torch.isnan(loss) | torch.isinf(loss)):
            loss.backward()
            opt.step()
        if step % 50 == 0 or step == a.steps - 1:
            print("step %4d  reverse KL %.4f nats" % (step, loss.item()), flush=True)
        first = loss.item() if first is None else first
        last = loss.item()
    with torch.no_grad():
        z, _ = model.sample(8192)
        print("mean |z0| of the samples %.3f (modes at -2 and 2), mean log p %.3f" % (float(z[:, 0].abs().mean()),
                                                                                     float(model.p.log_prob(z).mean())))
    return first, last


if __name__ == "__main__":
    first, last = main()
    assert last < first, "the reverse KL did not fall: %.4f -> %.4f" % (first, last)
