#!/usr/bin/env python3
"""Hamiltonian annealed importance sampling from a DiagGaussian prior to the prior TwoModes(2, 0.1) on the MI355X path,
`normflows_amd` in place of `normflows`: the log-mean-exp of the log-weights estimates the log of TwoModes' normalising constant
(its log_prob is unnormalised), and the samples land on the two modes at z0 = -2 and 2.

    python examples/hais_two_modes.py [--layers 20] [--leapfrog 5] [--samples 8192] [--kernels 1]

`--kernels 1` (config.set_stochastic_kernels(True)) runs every HamiltonianMonteCarlo transition of the chain -- the leapfrog
trajectory on the interpolated target, the Metropolis correction and the log-weight increment -- as one launch of nf_hmc2d;
`--kernels 0` runs the torch formulas, the reference's arithmetic.  Keep `betas` on the CPU: the kernel route reads each
interpolation weight on the host.  Runs on cuda:0.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import normflows_amd as nf  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=20)
    ap.add_argument("--leapfrog", type=int, default=5)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--kernels", type=int, default=1)
    a = ap.parse_args(argv)
    nf.config.set_stochastic_kernels(bool(a.kernels))
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    prior = nf.distributions.DiagGaussian(2, trainable=False).to(dev)
    with torch.no_grad():
        prior.log_scale.fill_(math.log(1.5))     # wide enough to cover both modes
    target = nf.distributions.TwoModes(2.0, 0.1)
    betas = torch.linspace(1.0, 0.0, a.layers + 2)          # 1 = beta_0 > ... > beta_n = 0: n - 1 = `layers` transitions
    hais = nf.HAIS(betas, prior, target, a.leapfrog, torch.tensor([0.08, 0.08], device=dev), torch.zeros(2, device=dev))
    with torch.no_grad():
        z, log_w = hais.sample(a.samples)
    log_mean_exp = float(torch.logsumexp(log_w, 0)) - math.log(a.samples)
    ess = float(torch.exp(2 * torch.logsumexp(log_w, 0) - torch.logsumexp(2 * log_w, 0)))
    print("%d transitions of %d leapfrog steps, %d samples" % (len(hais.layers), a.leapfrog, a.samples))
    print("log-mean-exp of the log-weights %.4f (log of TwoModes' normalising constant), effective sample size %.0f" % (log_mean_exp, ess))
    print("mean |z0| of the samples %.3f (modes at -2 and 2)" % float(z[:, 0].abs().mean()))
    return log_mean_exp, ess, z


if __name__ == "__main__":
    lme, ess, z = main()
    # a loose window around one seeded run (0.79, 2 590 of 8 192 samples, mean |z0| 1.87): a chain that lost the modes, or weights that
    # collapsed onto a few samples, falls outside it
    assert bool(torch.isfinite(z).all()) and 0.3 < lme < 1.3, lme
    assert ess > 0.05 * len(z) and 1.5 < float(z[:, 0].abs().mean()) < 2.3, ess
