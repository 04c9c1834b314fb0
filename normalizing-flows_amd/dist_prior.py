"""Prior densities in two dimensions (normflows/distributions/prior.py): PriorDistribution, ImagePrior, TwoModes, Sinusoidal,
Sinusoidal_gap, Sinusoidal_split, Smiley.

The analytic priors are plain classes, not modules.  Every log_prob keeps a torch-formula route (`_log_prob_torch`) that does the
reference's arithmetic op for op, the permute that accepts (..., 2) inputs included; a contiguous float32 CUDA (B, 2) input
otherwise runs as one launch of nf_density2d (dist_route.py, csrc/density2d.hip).  ImagePrior is a table lookup without a gradient:
torch formulas only."""
import numpy as np
import torch
from torch import nn

from .dist_target import _Routed


class PriorDistribution:
    def __init__(self):
        raise NotImplementedError

    def log_prob(self, z):
        raise NotImplementedError


class ImagePrior(nn.Module):
    """The intensities of an image as a density on [x_range] x [y_range] (prior.py:21-104); buffers image, image_size, density,
    scale, shift."""

    def __init__(self, image, x_range=[-3, 3], y_range=[-3, 3], eps=1.0e-10):
        super().__init__()
        image_ = np.flip(image, 0).transpose() + eps
        self.image_cpu = torch.tensor(image_ / np.max(image_))
        self.image_size_cpu = self.image_cpu.size()
        self.x_range = torch.tensor(x_range)
        self.y_range = torch.tensor(y_range)
        self.register_buffer("image", self.image_cpu)
        self.register_buffer("image_size", torch.tensor(self.image_size_cpu).unsqueeze(0))
        self.register_buffer("density", torch.log(self.image_cpu / torch.sum(self.image_cpu)))
        self.register_buffer("scale", torch.tensor([[self.x_range[1] - self.x_range[0], self.y_range[1] - self.y_range[0]]]))
        self.register_buffer("shift", torch.tensor([[self.x_range[0], self.y_range[0]]]))

    def log_prob(self, z):
        z_ = torch.clamp((z - self.shift) / self.scale, max=1, min=0)
        ind = (z_ * (self.image_size - 1)).long()
        return self.density[ind[:, 0], ind[:, 1]]

    def rejection_sampling(self, num_steps=1):
        z_ = torch.rand((num_steps, 2), dtype=self.image.dtype, device=self.image.device)
        prob = torch.rand(num_steps, dtype=self.image.dtype, device=self.image.device)
        ind = (z_ * (self.image_size - 1)).long()
        intensity = self.image[ind[:, 0], ind[:, 1]]
        accept = intensity > prob
        return z_[accept, :] * self.scale + self.shift

    def sample(self, num_samples=1):
        z = torch.ones((0, 2), dtype=self.image.dtype, device=self.image.device)
        while len(z) < num_samples:
            z_ = self.rejection_sampling(num_samples)
            ind = np.min([len(z_), num_samples - len(z)])
            z = torch.cat([z, z_[:ind, :]], 0)
        return z


def _last_first(z):
    """The last dimension in front (prior.py:183-186): z_[0], z_[1] are the two coordinates whatever the leading shape."""
    if z.dim() > 1:
        return z.permute((z.dim() - 1,) + tuple(range(0, z.dim() - 1)))
    return z


def _envelope(z_, scale):
    return 0.5 * (torch.norm(z_, dim=0, p=4) / (20 * scale)) ** 4


def _two_bumps(a, eps, scale):
    return -0.5 * ((a - eps) / scale) ** 2 + torch.log(1 + torch.exp(-2 * (eps * a) / scale ** 2))


class TwoModes(_Routed, PriorDistribution):
    """Two modes at z[0] = -loc and z[0] = loc (prior.py:107-149)."""

    def __init__(self, loc, scale):
        self.loc = loc
        self.scale = scale

    def _log_prob_torch(self, z):
        a = torch.abs(z[:, 0])
        eps = torch.abs(torch.tensor(self.loc))
        return (-0.5 * ((torch.norm(z, dim=1) - self.loc) / (2 * self.scale)) ** 2
                - 0.5 * ((a - eps) / (3 * self.scale)) ** 2
                + torch.log(1 + torch.exp(-2 * (a * eps) / (3 * self.scale) ** 2)))


class Sinusoidal(_Routed, PriorDistribution):
    """A sine ridge under a 4-norm envelope (prior.py:152-194)."""

    def __init__(self, scale, period):
        self.scale = scale
        self.period = period

    def _log_prob_torch(self, z):
        z_ = _last_first(z)
        w_1 = torch.sin(2 * np.pi / self.period * z_[0])
        return -0.5 * ((z_[1] - w_1) / self.scale) ** 2 - _envelope(z_, self.scale)


class Sinusoidal_gap(_Routed, PriorDistribution):
    """The sine ridge with a gap (prior.py:197-245)."""

    def __init__(self, scale, period):
        self.scale = scale
        self.period = period
        self.w2_scale = 0.6
        self.w2_amp = 3.0
        self.w2_mu = 1.0

    def _log_prob_torch(self, z):
        z_ = _last_first(z)
        w_1 = torch.sin(2 * np.pi / self.period * z_[0])
        w_2 = self.w2_amp * torch.exp(-0.5 * ((z_[0] - self.w2_mu) / self.w2_scale) ** 2)
        eps = torch.abs(w_2 / 2)
        a = torch.abs(z_[1] - w_1 + w_2 / 2)
        return _two_bumps(a, eps, self.scale) - _envelope(z_, self.scale)


class Sinusoidal_split(_Routed, PriorDistribution):
    """The sine ridge splitting in two (prior.py:248-296)."""

    def __init__(self, scale, period):
        self.scale = scale
        self.period = period
        self.w3_scale = 0.3
        self.w3_amp = 3.0
        self.w3_mu = 1.0

    def _log_prob_torch(self, z):
        z_ = _last_first(z)
        w_1 = torch.sin(2 * np.pi / self.period * z_[0])
        w_3 = self.w3_amp * torch.sigmoid((z_[0] - self.w3_mu) / self.w3_scale)
        eps = torch.abs(w_3 / 2)
        a = torch.abs(z_[1] - w_1 + w_3 / 2)
        return _two_bumps(a, eps, self.scale) - _envelope(z_, self.scale)


class Smiley(_Routed, PriorDistribution):
    """A smiley (prior.py:299-327)."""

    def __init__(self, scale):
        self.scale = scale
        self.loc = 2.0

    def _log_prob_torch(self, z):
        z_ = _last_first(z)
        return (-0.5 * ((torch.norm(z_, dim=0) - self.loc) / (2 * self.scale)) ** 2
                - 0.5 * ((torch.abs(z_[1] + 0.8) - 1.2) / (2 * self.scale)) ** 2)
