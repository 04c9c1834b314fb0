"""The distributions the stochastic flow layers are built from: the Metropolis-Hastings proposals
(normflows/distributions/mh_proposal.py: MHProposal, DiagGaussianProposal) and the log-space interpolation of two densities that
HAIS anneals along (normflows/distributions/linear_interpolation.py: LinearInterpolation).

Torch statements with the reference's arithmetic and its random draws in its order; they serve every shape, dtype and device.  On
2-D float32 CUDA batches flows.MetropolisHastings / flows.HamiltonianMonteCarlo evaluate these classes inside their one launch
(stochastic_route.py, csrc/hmc2d.hip) and never call them."""
import numpy as np
import torch
from torch import nn


class MHProposal(nn.Module):
    """Proposal distribution of the Metropolis-Hastings algorithm (mh_proposal.py:6-47): the interface."""

    def __init__(self):
        super().__init__()

    def sample(self, z):
        """A new value given the previous z."""
        raise NotImplementedError

    def log_prob(self, z_, z):
        """Log-probability of the proposal z_ given the previous sample z."""
        raise NotImplementedError

    def forward(self, z):
        """(proposal, log p(z | z_new) - log p(z_new | z))."""
        raise NotImplementedError


class DiagGaussianProposal(MHProposal):
    """Diagonal Gaussian centred on the previous value (mh_proposal.py:50-82).  Buffer `scale` of shape (1, ...) and the attribute
    `scale_cpu` as there; `sample` and `forward` draw `randn((len(z),) + shape)` once each."""

    def __init__(self, shape, scale):
        super().__init__()
        self.shape = shape
        self.scale_cpu = torch.tensor(scale)
        self.register_buffer("scale", self.scale_cpu.unsqueeze(0))

    def sample(self, z):
        num_samples = len(z)
        eps = torch.randn((num_samples,) + self.shape, dtype=z.dtype, device=z.device)
        z_ = eps * self.scale + z
        return z_

    def log_prob(self, z_, z):
        log_p = -0.5 * np.prod(self.shape) * np.log(2 * np.pi) - torch.sum(
            torch.log(self.scale) + 0.5 * torch.pow((z_ - z) / self.scale, 2), list(range(1, z.dim())))
        return log_p

    def forward(self, z):
        num_samples = len(z)
        eps = torch.randn((num_samples,) + self.shape, dtype=z.dtype, device=z.device)
        return self._propose(z, eps)

    def _propose(self, z, eps):
        """forward on given standard-normal noise (the proposal is symmetric: the log-probability difference is zero)."""
        z_ = eps * self.scale + z
        log_p_diff = torch.zeros(len(z), dtype=z.dtype, device=z.device)
        return z_, log_p_diff


class LinearInterpolation:
    """alpha log p_1 + (1 - alpha) log p_2 (linear_interpolation.py:1-28).  A plain object, not a Module, as in the reference."""

    def __init__(self, dist1, dist2, alpha):
        self.alpha = alpha
        self.dist1 = dist1
        self.dist2 = dist2

    def log_prob(self, z):
        return self.alpha * self.dist1.log_prob(z) + (1 - self.alpha) * self.dist2.log_prob(z)
