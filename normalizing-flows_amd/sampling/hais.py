"""Hamiltonian annealed importance sampling (normflows/sampling/hais.py): a chain of HamiltonianMonteCarlo transitions whose
targets interpolate, in log space, from the prior to the target.

The chain is a host loop over flows.HamiltonianMonteCarlo layers; on 2-D float32 CUDA batches each of them is one launch
(config.stochastic_kernels), the interpolated target evaluated inside it from the two densities' records and `betas[i]` read on the
host (keep `betas` on the CPU: a device tensor keeps the torch formulas)."""
import torch

from .. import distributions
from .. import flows


class HAIS:
    """HAIS (hais.py:8-52).  betas: the annealing schedule 1 = beta_0 > beta_1 > ... > beta_n = 0, the j-th intermediate target is
    f_0^beta_j f_n^(1 - beta_j) with f_0 the target and f_n the prior.  `layers` is a plain list built for i = n-1 .. 1, each a
    HamiltonianMonteCarlo(LinearInterpolation(target, prior, betas[i]), num_leapfrog, log(step_size), log_mass)."""

    def __init__(self, betas, prior, target, num_leapfrog, step_size, log_mass):
        self.prior = prior
        self.target = target
        self.layers = []
        n = betas.shape[0] - 1
        for i in range(n - 1, 0, -1):
            intermediate_target = distributions.LinearInterpolation(self.target, self.prior, betas[i])
            self.layers += [flows.HamiltonianMonteCarlo(intermediate_target, num_leapfrog, torch.log(step_size), log_mass)]

    def sample(self, num_samples):
        """(samples, log_weights) of num_samples weighted draws from the target."""
        samples, log_weights = self.prior.forward(num_samples)
        log_weights = -log_weights
        for i in range(len(self.layers)):
            samples, log_weights_addition = self.layers[i].forward(samples)
            log_weights += log_weights_addition
        log_weights += self.target.log_prob(samples)
        return samples, log_weights
