#!/usr/bin/env python3
"""The reference README's quick-start model on the MI355X path -- 32 x [AffineCouplingBlock(MLP([1, 64, 64, 2])), Permute(2, 'swap')]
trained on the two-moons density with the reference's loop (forward KL, Adam), `normflows_amd` in place of `normflows`.

    python examples/realnvp_quickstart.py [--steps 400] [--batch 1024]

Each [block, Permute] pair is one record of the RealNVP chain kernels (config.realnvp_blocks): a training step is one forward and one
backward launch for the 64 layers, `log_prob` / `sample` under no_grad one launch.  Runs on cuda:0; the layers have no CPU path.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import normflows_amd as nf  # noqa: E402


def two_moons_log_prob(z):
    """log p(z) = -1/2 ((|z| - 2) / 0.2)^2 + log(exp(-1/2 ((z_0 - 2) / 0.3)^2) + exp(-1/2 ((z_0 + 2) / 0.3)^2)), maximum 0."""
    a = z[:, 0].abs()
    return -0.5 * ((z.norm(dim=1) - 2) / 0.2) ** 2 - 0.5 * ((a - 2) / 0.3) ** 2 + torch.log1p(torch.exp(-4 * a / 0.09))


def sample_two_moons(n, gen):
    """n rows of the two-moons density by rejection from the uniform density on [-3, 3]^2."""
    rows = []
    while sum(len(r) for r in rows) < n:
        z = 6.0 * torch.rand(4 * n, 2, generator=gen) - 3.0
        rows.append(z[torch.rand(4 * n, generator=gen).log() < two_moons_log_prob(z)])
    return torch.cat(rows)[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=32)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    flows = []
    for _ in range(a.layers):
        param_map = nf.nets.MLP([1, 64, 64, 2], init_zeros=True)
        flows.append(nf.flows.AffineCouplingBlock(param_map))
        flows.append(nf.flows.Permute(2, mode="swap"))
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), flows).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=5e-4, weight_decay=1e-5)
    gen = torch.Generator().manual_seed(1)
    first = last = None
    for step in range(a.steps):
        x = sample_two_moons(a.batch, gen).to(dev)
        opt.zero_grad()
        loss = model.forward_kld(x)
        if ~(torch.isnan(loss) | torch.isinf(loss)):
            loss.backward()
            opt.step()
        if step % 50 == 0 or step == a.steps - 1:
            print("step %4d  forward KL %.4f nats" % (step, loss.item()), flush=True)
        first = loss.item() if first is None else first
        last = loss.item()
    with torch.no_grad():
        x = sample_two_moons(8192, gen).to(dev)
        nll = -model.log_prob(x).mean()
        xs, lq = model.sample(8192)
        print("held-out NLL %.4f nats; log_prob(sample) - log_q max diff %.2e" % (
            float(nll), float((model.log_prob(xs) - lq).abs().max())))
    return first, last


if __name__ == "__main__":
    main()
