"""Target distributions to train models against (normflows/distributions/target.py): Target with its rejection sampler, TwoMoons,
CircularGaussianMixture, RingMixture, TwoIndependent and the target-side ConditionalDiagGaussian.

Every log_prob keeps a torch-formula route (`_log_prob_torch`) that does the reference's arithmetic op for op; it serves CPU,
float64, non-contiguous or non-(B, 2) inputs, subclasses, config.higher_order_gradients() and config.target_density turned off.
The closed-form 2-D densities otherwise run as one launch of nf_density2d (dist_route.py, csrc/density2d.hip).  Sampling is torch
statements with the random draws in the reference's order."""
import numpy as np
import torch
from torch import nn

from . import dist_route
from .flows.reshape import Split


class Target(nn.Module):
    """A target with a uniform proposal box for rejection sampling (target.py:8-73): buffers prop_scale, prop_shift; subclasses
    set n_dims and max_log_prob."""

    def __init__(self, prop_scale=torch.tensor(6.0), prop_shift=torch.tensor(-3.0)):
        super().__init__()
        self.register_buffer("prop_scale", prop_scale)
        self.register_buffer("prop_shift", prop_shift)

    def log_prob(self, z):
        raise NotImplementedError("The log probability is not implemented yet.")

    def rejection_sampling(self, num_steps=1):
        """One round: `rand((num_steps, n_dims))` for the proposals, then `rand(num_steps)` for the accept test (target.py:43-55)."""
        dtype, device = self.prop_scale.dtype, self.prop_scale.device
        eps = torch.rand((num_steps, self.n_dims), dtype=dtype, device=device)
        z_ = self.prop_scale * eps + self.prop_shift
        prob = torch.rand(num_steps, dtype=dtype, device=device)
        prob_ = torch.exp(self.log_prob(z_) - self.max_log_prob)
        accept = prob_ > prob
        return z_[accept, :]

    def sample(self, num_samples=1):
        z = torch.zeros((0, self.n_dims), dtype=self.prop_scale.dtype, device=self.prop_scale.device)
        while len(z) < num_samples:
            z_ = self.rejection_sampling(num_samples)
            ind = np.min([len(z_), num_samples - len(z)])
            z = torch.cat([z, z_[:ind, :]], 0)
        return z


class _Routed:
    """log_prob of a closed-form 2-D density: the kernel where dist_route.eligible says so, the torch formulas otherwise."""

    def log_prob(self, z):
        if dist_route.eligible(self, z):
            return dist_route.log_prob(self, z)
        return self._log_prob_torch(z)


class TwoIndependent(Target):
    """Two independent targets of equal size side by side (target.py:76-96), split and merged by flows.Split('channel')."""

    def __init__(self, target1, target2):
        super().__init__()
        self.target1 = target1
        self.target2 = target2
        self.split = Split(mode="channel")

    def log_prob(self, z):
        z1, z2 = self.split(z)[0]
        return self.target1.log_prob(z1) + self.target2.log_prob(z2)

    def sample(self, num_samples=1):
        z1 = self.target1.sample(num_samples)
        z2 = self.target2.sample(num_samples)
        return self.split.inverse([z1, z2])[0]


class TwoMoons(_Routed, Target):
    """Bimodal two-dimensional density (target.py:99-129); the same formula as prior.TwoModes(2, 0.1)."""

    def __init__(self):
        super().__init__()
        self.n_dims = 2
        self.max_log_prob = 0.0

    def _log_prob_torch(self, z):
        a = torch.abs(z[:, 0])
        return (-0.5 * ((torch.norm(z, dim=1) - 2) / 0.2) ** 2
                - 0.5 * ((a - 2) / 0.3) ** 2
                + torch.log(1 + torch.exp(-4 * a / 0.09)))


class CircularGaussianMixture(_Routed, nn.Module):
    """n_modes Gaussians on a circle of radius 2 (target.py:132-173); buffer `scale`."""

    def __init__(self, n_modes=8):
        super().__init__()
        self.n_modes = n_modes
        self.register_buffer("scale", torch.tensor(2 / 3 * np.sin(np.pi / self.n_modes)).float())

    def _log_prob_torch(self, z):
        d = torch.zeros((len(z), 0), dtype=z.dtype, device=z.device)
        for i in range(self.n_modes):
            d_ = ((z[:, 0] - 2 * np.sin(2 * np.pi / self.n_modes * i)) ** 2
                  + (z[:, 1] - 2 * np.cos(2 * np.pi / self.n_modes * i)) ** 2) / (2 * self.scale ** 2)
            d = torch.cat((d, d_[:, None]), 1)
        return -torch.log(2 * np.pi * self.scale ** 2 * self.n_modes) + torch.logsumexp(-d, 1)

    def sample(self, num_samples=1):
        eps = torch.randn((num_samples, 2), dtype=self.scale.dtype, device=self.scale.device)
        phi = 2 * np.pi / self.n_modes * torch.randint(0, self.n_modes, (num_samples,), device=self.scale.device)
        loc = torch.stack((2 * torch.sin(phi), 2 * torch.cos(phi)), 1).type(eps.dtype)
        return eps * self.scale + loc


class RingMixture(_Routed, Target):
    """n_rings concentric rings (target.py:176-195)."""

    def __init__(self, n_rings=2):
        super().__init__()
        self.n_dims = 2
        self.max_log_prob = 0.0
        self.n_rings = n_rings
        self.scale = 1 / 4 / self.n_rings

    def _log_prob_torch(self, z):
        d = torch.zeros((len(z), 0), dtype=z.dtype, device=z.device)
        for i in range(self.n_rings):
            d_ = ((torch.norm(z, dim=1) - 2 / self.n_rings * (i + 1)) ** 2) / (2 * self.scale ** 2)
            d = torch.cat((d, d_[:, None]), 1)
        return torch.logsumexp(-d, 1)


class ConditionalDiagGaussian(Target):
    """Gaussian whose mean and standard deviation are the two halves of the context (target.py:198-224).  Torch formulas only.
    Reachable as distributions.target.ConditionalDiagGaussian; distributions.ConditionalDiagGaussian is the base distribution."""

    def log_prob(self, z, context=None):
        d = z.shape[-1]
        loc = context[:, :d]
        scale = context[:, d:]
        return -0.5 * d * np.log(2 * np.pi) - torch.sum(torch.log(scale) + 0.5 * torch.pow((z - loc) / scale, 2), dim=-1)

    def sample(self, num_samples=1, context=None):
        d = context.shape[-1] // 2
        loc = context[:, :d]
        scale = context[:, d:]
        eps = torch.randn((num_samples, d), dtype=context.dtype, device=context.device)
        return loc + scale * eps
