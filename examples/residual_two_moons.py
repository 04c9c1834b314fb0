#!/usr/bin/env python3
"""The reference's residual.ipynb loop on the MI355X path: K x [Residual(LipschitzMLP([2, 128, 128, 2])), ActNorm(2)] trained by
forward KL on samples of TwoMoons (Adamax, update_lipschitz after every step), `normflows_amd` in place of `normflows`.

    python examples/residual_two_moons.py [--steps 300] [--batch 1024] [--layers 16]

`--kernels 1` (config.set_residual_train(True)) runs every Residual layer's training pass as one forward and one backward launch of
csrc/lipmlp_train.hip; `--kernels 0` runs the torch formulas, the reference's arithmetic.  Runs on cuda:0.
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
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args(argv)
    nf.config.set_residual_train(bool(a.kernels))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    flows = []
    for _ in range(a.layers):
        net = nf.nets.LipschitzMLP([2, 128, 128, 2], init_zeros=True, lipschitz_const=0.9)
        flows += [nf.flows.Residual(net, reduce_memory=True), nf.flows.ActNorm(2)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2, trainable=False), flows).to(dev)
    target = nf.distributions.TwoMoons()
    opt = torch.optim.Adamax(model.parameters(), lr=3e-3, weight_decay=1e-5)
    losses = []
    for step in range(a.steps):
        opt.zero_grad()
        x = target.sample(a.batch).to(dev)
        loss = model.forward_kld(x)
        if ~(torch.isnan(loss) | torch.isinf(loss)):
            loss.backward()
            opt.step()
        nf.utils.update_lipschitz(model, 50)
        losses.append(loss.item())
        if step % 50 == 0 or step == a.steps - 1:
            print("step %4d  forward KL %.4f nats" % (step, losses[-1]), flush=True)
    n = max(1, len(losses) // 10)
    return sum(losses[:n]) / n, sum(losses[-n:]) / n


if __name__ == "__main__":
    first, last = main()
    assert last < first, "the forward KL did not fall: %.4f -> %.4f" % (first, last)
